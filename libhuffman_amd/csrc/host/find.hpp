/* find.hpp - hufgpu_find_bytes, hufgpu_find_pattern and hufgpu_find_records: where the bytes of a set of byte values lie
   in the original data, where a pattern of bytes starts, and which records - the pieces between delimiters - hold the
   pattern; hufgpu_find_classes and hufgpu_find_records_classes: the same for a pattern whose every position is a set of
   byte values; hufgpu_find_any and hufgpu_find_records_any: the same for ANY of several such patterns, in the one walk
   (include/huffman_gpu.h, kernels/find.hpp); hufgpu_find_records_select: the records WITHOUT a match of any alternative,
   and the records' numbers.  All enqueue-only.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

static_assert(FIND_PAT_MAX == HUFGPU_FIND_PATTERN_MAX, "kernels/find.hpp and include/huffman_gpu.h");
static_assert(FIND_REC_NO_UNKNOWN == HUFGPU_REC_NO_UNKNOWN, "kernels/find.hpp and include/huffman_gpu.h");

/* what hufgpu_find_records has beyond the pattern call: d_pos / pos_cap are its d_rec_pos / rec_cap */
struct FindRecCall {
    const uint8_t *delim_set;
    uint32_t *d_len;
    uint32_t max_len;
};

/* what hufgpu_find_records_select has beyond the any-of records' call */
struct FindSelCall {
    uint32_t select;                        /* checked by the wrapper */
    uint64_t *d_rec_no;                     /* optional */
};

/* All eight calls: `who` words the errors, `key` is the set (plen = 0) or the pattern of plen bytes, `key_name` its name;
 * rec is NULL but for the records' calls.  cls is NULL but for the class calls: then `key` is the caller's array of plen
 * classes, which this function only checks for NULL and never reads - its wrapper has read it -, and cls is the table made
 * from it.  alt is NULL but for the any-of calls: then cls is alt's table (several alternatives in its 64 bits), plen is the
 * LONGEST alternative's length - what the edges workspace and the seam launch follow - and alt goes to the kernels.
 * sel is NULL but for the select call, which is the any-of records' call with up to three launches more: the seven other
 * calls enqueue what they always did. */
static int find_call(hufgpu_ctx_t *ctx, const char *who, const char *key_name, const uint8_t *key, uint32_t plen,
                     const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets, uint64_t nblocks,
                     const void *d_sub_index, uint64_t raw_size, uint64_t blocksize, uint64_t *d_pos, uint64_t pos_cap,
                     uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream,
                     const FindRecCall *rec = NULL, const FindClsTable *cls = NULL, FindAltArgs *alt = NULL,
                     const FindSelCall *sel = NULL)
{
    if (!key || !d_totals) {
        set_err(ctx, "%s: the %s and d_totals are required", who, key_name);
        return HUFE_ARGUMENT;
    }
    if (rec) {
        if (!rec->delim_set) {
            set_err(ctx, "%s: the delim_set is required (32 zero bytes: the data is one record)", who);
            return HUFE_ARGUMENT;
        }
        if (!cls) {                                                 /* (the classes' wrapper has looked at its classes) */
            for (uint32_t i = 0; i < plen; i++) {
                if ((rec->delim_set[key[i] >> 3] >> (key[i] & 7)) & 1) {
                    set_err(ctx, "%s: byte %u of the pattern (value %u) is a delimiter: a match lies inside one record", who, i, key[i]);
                    return HUFE_ARGUMENT;
                }
            }
        }
        if (pos_cap > 0 && (!d_pos || !rec->d_len)) {
            set_err(ctx, "%s: rec_cap %llu needs d_rec_pos and d_rec_len", who, (unsigned long long)pos_cap);
            return HUFE_ARGUMENT;
        }
    } else if (pos_cap > 0 && !d_pos) {
        set_err(ctx, "%s: pos_cap %llu needs d_pos", who, (unsigned long long)pos_cap);
        return HUFE_ARGUMENT;
    }
    if (nblocks == 0) {
        if (raw_size != 0) {
            set_err(ctx, "%s: (raw_size, blocksize) must be those of the encode that wrote these 0 blocks", who);
            return HUFE_ARGUMENT;
        }
        if (!ctx) {
            set_err(NULL, "%s: needs a context (there is no CPU path)", who);
            return HUFE_ARGUMENT;
        }
        HIP_OK(ctx, hipSetDevice(ctx->device));
        HIP_OK(ctx, hipMemsetAsync(d_totals, 0, 4 * sizeof(uint64_t), pick_stream(ctx, stream)));
        return HUFE_OK;
    }
    if (!d_stream || !d_block_offsets || !d_block_errs) {
        set_err(ctx, "%s: the stream, its block index and d_block_errs are required", who);
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "%s: needs the stream's sub-index in an 8-byte aligned buffer", who);
        return HUFE_ARGUMENT;
    }
    if (blocksize == 0) blocksize = raw_size;
    const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
    const uint64_t wpb = (blocksize + DSUB_SPL - 1) / DSUB_SPL, tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    if (raw_size == 0 || blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, blocksize) != nblocks ||
        nblocks > 0x7fffffffull || nblocks * tpb > 0x7fffffffull) {
        set_err(ctx, "%s: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks (at most 2^31 - 1 tiles)",
                who, (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "%s: needs a context (there is no CPU path)", who);
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    int rc = ensure_find_ws(ctx, nblocks * wpb, nblocks * tpb);
    if (!rc && plen > 1) rc = grow_ws(ctx, G_FIND_EDGES, nblocks * tpb);    /* (one byte has no seams: no edges) */
    if (!rc && rec) rc = grow_ws2(ctx, G_FIND_REC_WORDS, nblocks * wpb, G_FIND_REC_TILES, nblocks * tpb);
    const bool invert = sel && (sel->select & HUFGPU_SELECT_INVERT), numbers = sel && sel->d_rec_no && pos_cap > 0;
    if (!rc && numbers) rc = grow_ws(ctx, G_FIND_SEL, 1);
    if (rc) return rc;

    FindRecArgs ra;
    memset(&ra, 0, sizeof(ra));
    FindPatArgs &pa = ra.p;
    FindArgs &fa = pa.f;
    fa.s = sub_stream_args(d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize, flags);
    fa.cpb = (uint32_t)cpb;
    if (plen == 0) {
        for (int i = 0; i < 32; i++) fa.set[i >> 2] |= (uint32_t)key[i] << (8 * (i & 3));
    } else {
        if (!cls) {
            for (uint32_t i = 0; i < plen; i++) pa.pat[i >> 2] |= (uint32_t)key[i] << (8 * (i & 3));
        }
        pa.plen = plen;
        pa.edges = ctx->d_fedges;
    }
    fa.bitmap = ctx->d_fbitmap;
    fa.wpb = wpb;
    fa.tcnt = ctx->d_ftcnt;
    fa.tpb = tpb;
    fa.ntiles = nblocks * tpb;
    fa.scan = ctx->find_scan;
    fa.scan.total = d_totals;
    fa.pos = d_pos;
    fa.pos_cap = pos_cap;
    fa.block_counts = d_block_counts;
    fa.totals = d_totals;
    fa.errs = d_block_errs;
    HIP_OK(ctx, hipMemsetAsync(d_block_errs, 0, nblocks * sizeof(int32_t), s));
    HIP_OK(ctx, hipMemsetAsync(d_totals, 0, 4 * sizeof(uint64_t), s));
    if (rec) {
        /* one walk for both masks, the seams of the matches, then from the two masks to the records' starts and their
         * counts by tile; scan and finish take the records of a tile as they take its matches */
        for (int i = 0; i < 32; i++) fa.set[i >> 2] |= (uint32_t)rec->delim_set[i] << (8 * (i & 3));
        ra.dbits = ctx->d_frdbits;
        ra.dcnt = ctx->d_frdcnt;
        ra.rbits = ctx->d_frrbits;
        ra.rcnt = ctx->d_frrcnt;
        ra.dscan = ctx->frec_scan;
        ra.dscan.total = ctx->d_frdtotal;
        ra.len = rec->d_len;
        ra.clip = rec->max_len ? rec->max_len : 0xffffffffu;
        const uint64_t per = FIND_EMIT_THREADS / 64;
        const dim3 tiles((unsigned)((fa.ntiles + per - 1) / per)), groups((unsigned)((fa.ntiles + SCAN_GROUP - 1) / SCAN_GROUP));
        HIP_OK(ctx, hipMemsetAsync(ra.rbits, 0, nblocks * wpb * sizeof(uint32_t), s));
        HIP_OK(ctx, hipMemsetAsync(ra.rcnt, 0, fa.ntiles * sizeof(uint32_t), s));
        const uint64_t sper = FIND_SEAM_THREADS / 64;
        const dim3 seams((unsigned)((fa.ntiles + sper - 1) / sper));
        if (alt) {                                                  /* the table goes with the launches' own arguments */
            alt->r = ra;
            find_rec_alt_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(*alt);
            if (plen > 1) find_alt_seam_kernel<<<seams, dim3(FIND_SEAM_THREADS), 0, s>>>(*alt);
        } else if (cls) {
            const FindClsArgs ca = {ra, *cls};
            find_rec_cls_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(ca);
            if (plen > 1) find_cls_seam_kernel<<<seams, dim3(FIND_SEAM_THREADS), 0, s>>>(ca);
        } else {
            find_rec_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(ra);
            if (plen > 1) find_seam_kernel<<<seams, dim3(FIND_SEAM_THREADS), 0, s>>>(pa);
        }
        find_rec_dscan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(ra);
        find_rec_mark_kernel<<<tiles, dim3(FIND_EMIT_THREADS), 0, s>>>(ra);
        if (invert) find_rec_invert_kernel<<<tiles, dim3(FIND_EMIT_THREADS), 0, s>>>(ra);   /* over mark's words and counts */
        FindArgs fr = fa;                                           /* scan, finish and emit: the records of a tile in the place of its matches */
        fr.tcnt = ra.rcnt;
        ra.p.f = fr;
        find_scan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(fr);
        find_finish_kernel<<<dim3(grid256(nblocks)), dim3(256), 0, s>>>(fr);
        if (numbers) {                                              /* the numbers need the first block that is not served */
            const FindSelArgs sa = {ra, sel->d_rec_no, ctx->d_fsel_first};
            HIP_OK(ctx, hipMemsetAsync(sa.first_bad, 0xff, sizeof(uint64_t), s));
            find_rec_first_bad_kernel<<<dim3(grid256(nblocks)), dim3(256), 0, s>>>(sa);
            find_rec_emit_no_kernel<<<tiles, dim3(FIND_EMIT_THREADS), 0, s>>>(sa);
        } else if (pos_cap > 0) {
            find_rec_emit_kernel<<<tiles, dim3(FIND_EMIT_THREADS), 0, s>>>(ra);
        }
        HIP_OK(ctx, hipGetLastError());
        return HUFE_OK;
    }
    if (plen == 0) {
        find_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(fa);
    } else if (alt) {
        const uint64_t per = FIND_SEAM_THREADS / 64;
        alt->r = ra;
        find_alt_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(*alt);
        if (plen > 1) find_alt_seam_kernel<<<dim3((unsigned)((fa.ntiles + per - 1) / per)), dim3(FIND_SEAM_THREADS), 0, s>>>(*alt);
    } else if (cls) {
        const FindClsArgs ca = {ra, *cls};
        const uint64_t per = FIND_SEAM_THREADS / 64;
        find_cls_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(ca);
        if (plen > 1) find_cls_seam_kernel<<<dim3((unsigned)((fa.ntiles + per - 1) / per)), dim3(FIND_SEAM_THREADS), 0, s>>>(ca);
    } else {
        find_pat_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(pa);
        if (plen > 1) {
            const uint64_t per = FIND_SEAM_THREADS / 64;
            find_seam_kernel<<<dim3((unsigned)((fa.ntiles + per - 1) / per)), dim3(FIND_SEAM_THREADS), 0, s>>>(pa);
        }
    }
    find_scan_kernel<<<dim3((unsigned)((fa.ntiles + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(fa);
    find_finish_kernel<<<dim3(grid256(nblocks)), dim3(256), 0, s>>>(fa);
    if (pos_cap > 0) {
        const uint64_t per = FIND_EMIT_THREADS / 64;
        find_emit_kernel<<<dim3((unsigned)((fa.ntiles + per - 1) / per)), dim3(FIND_EMIT_THREADS), 0, s>>>(fa);
    }
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

extern "C" int hufgpu_find_bytes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                 uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                 const uint8_t set[32], uint64_t *d_pos, uint64_t pos_cap, uint64_t *d_block_counts,
                                 uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    return find_call(ctx, "find_bytes", "set", set, 0, d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size,
                     blocksize, d_pos, pos_cap, d_block_counts, d_totals, d_block_errs, flags, stream);
}

extern "C" int hufgpu_find_pattern(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t *pattern, uint32_t pattern_len, uint64_t *d_pos, uint64_t pos_cap,
                                   uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (pattern && (pattern_len == 0 || pattern_len > HUFGPU_FIND_PATTERN_MAX)) {
        set_err(ctx, "find_pattern: pattern_len %u is not 1 to %d", pattern_len, HUFGPU_FIND_PATTERN_MAX);
        return HUFE_ARGUMENT;
    }
    return find_call(ctx, "find_pattern", "pattern", pattern, pattern_len, d_stream, stream_len, d_block_offsets, nblocks,
                     d_sub_index, raw_size, blocksize, d_pos, pos_cap, d_block_counts, d_totals, d_block_errs, flags, stream);
}

extern "C" int hufgpu_find_records(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t delim_set[32], const uint8_t *pattern, uint32_t pattern_len, uint64_t *d_rec_pos,
                                   uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len, uint64_t *d_block_counts,
                                   uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (pattern && (pattern_len == 0 || pattern_len > HUFGPU_FIND_PATTERN_MAX)) {
        set_err(ctx, "find_records: pattern_len %u is not 1 to %d", pattern_len, HUFGPU_FIND_PATTERN_MAX);
        return HUFE_ARGUMENT;
    }
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    return find_call(ctx, "find_records", "pattern", pattern, pattern_len, d_stream, stream_len, d_block_offsets, nblocks,
                     d_sub_index, raw_size, blocksize, d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs, flags, stream, &rec);
}

/* The class calls' own checks - the length, no empty class, no class that holds a delimiter - and the transposed table
 * (kernels/find.hpp: position k at bit 63 - k of m[v]).  `classes` is not NULL; a NULL delim_set is find_call's to word. */
static int find_cls_table(hufgpu_ctx_t *ctx, const char *who, const uint8_t *classes, uint32_t plen, const uint8_t *delim_set,
                          FindClsTable *t)
{
    if (plen == 0 || plen > HUFGPU_FIND_PATTERN_MAX) {
        set_err(ctx, "%s: pattern_len %u is not 1 to %d", who, plen, HUFGPU_FIND_PATTERN_MAX);
        return HUFE_ARGUMENT;
    }
    memset(t, 0, sizeof(*t));
    for (uint32_t k = 0; k < plen; k++) {
        const uint8_t *cl = classes + 32u * k;
        bool any = false;
        for (uint32_t v = 0; v < 256; v++) {
            if (!((cl[v >> 3] >> (v & 7)) & 1)) continue;
            if (delim_set && ((delim_set[v >> 3] >> (v & 7)) & 1)) {
                set_err(ctx, "%s: class %u of the pattern holds a delimiter (value %u): a match lies inside one record", who, k, v);
                return HUFE_ARGUMENT;
            }
            any = true;
            t->m[v][k < 32 ? 1 : 0] |= 1u << (31u - (k & 31u));
        }
        if (!any) {
            set_err(ctx, "%s: class %u of the pattern is empty: it matches nothing", who, k);
            return HUFE_ARGUMENT;
        }
        t->full[k < 32 ? 1 : 0] |= 1u << (31u - (k & 31u));
    }
    t->first[plen <= 32 ? 1 : 0] = 1u << (31u - ((plen - 1u) & 31u));
    return HUFE_OK;
}

extern "C" int hufgpu_find_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t *classes, uint32_t pattern_len, uint64_t *d_pos, uint64_t pos_cap,
                                   uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindClsTable t;
    if (classes) {
        const int rc = find_cls_table(ctx, "find_classes", classes, pattern_len, NULL, &t);
        if (rc) return rc;
    }
    return find_call(ctx, "find_classes", "classes", classes, pattern_len, d_stream, stream_len, d_block_offsets, nblocks,
                     d_sub_index, raw_size, blocksize, d_pos, pos_cap, d_block_counts, d_totals, d_block_errs, flags, stream, NULL, &t);
}

extern "C" int hufgpu_find_records_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                           uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                           const uint8_t delim_set[32], const uint8_t *classes, uint32_t pattern_len,
                                           uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                                           uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindClsTable t;
    if (classes) {
        const int rc = find_cls_table(ctx, "find_records_classes", classes, pattern_len, delim_set, &t);
        if (rc) return rc;
    }
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    return find_call(ctx, "find_records_classes", "classes", classes, pattern_len, d_stream, stream_len, d_block_offsets, nblocks,
                     d_sub_index, raw_size, blocksize, d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs, flags, stream, &rec, &t);
}

/* The any-of calls' own checks - 1 to 64 alternatives, none of length 0, lengths that sum to at most 64, no empty class, no
 * class that holds a delimiter - and their table (kernels/find.hpp, FindAltArgs: alternative 0 at the bits 63 ... 64 - len_0,
 * alternative 1 below it, position k of alternative j at bit hi_j - k).  `classes` and `alt_lens` are not NULL; the total is
 * looked at before `classes` is read.  *maxlen: the longest alternative's length. */
static int find_alt_table(hufgpu_ctx_t *ctx, const char *who, const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                          const uint8_t *delim_set, FindAltArgs *t, uint32_t *maxlen)
{
    if (n_alts == 0 || n_alts > HUFGPU_FIND_PATTERN_MAX) {
        set_err(ctx, "%s: n_alts %u is not 1 to %d", who, n_alts, HUFGPU_FIND_PATTERN_MAX);
        return HUFE_ARGUMENT;
    }
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_alts; j++) {
        if (alt_lens[j] == 0) {
            set_err(ctx, "%s: alternative %u has length 0: it would match everywhere", who, j);
            return HUFE_ARGUMENT;
        }
        total += alt_lens[j];
    }
    if (total > HUFGPU_FIND_PATTERN_MAX) {
        set_err(ctx, "%s: the lengths of the %u alternatives sum to %llu, above %d", who, n_alts, (unsigned long long)total,
                HUFGPU_FIND_PATTERN_MAX);
        return HUFE_ARGUMENT;
    }
    memset(t, 0, sizeof(*t));
    t->n_alts = n_alts;
    *maxlen = 0;
    uint32_t hi = 63;
    const uint8_t *cl = classes;
    for (uint32_t j = 0; j < n_alts; j++) {
        const uint32_t len = alt_lens[j];
        for (uint32_t k = 0; k < len; k++, cl += 32) {
            const uint32_t bit = hi - k;
            bool any = false;
            for (uint32_t v = 0; v < 256; v++) {
                if (!((cl[v >> 3] >> (v & 7)) & 1)) continue;
                if (delim_set && ((delim_set[v >> 3] >> (v & 7)) & 1)) {
                    set_err(ctx, "%s: class %u of alternative %u holds a delimiter (value %u): a match lies inside one record", who, k, j, v);
                    return HUFE_ARGUMENT;
                }
                any = true;
                t->t.m[v][bit >> 5] |= 1u << (bit & 31u);
            }
            if (!any) {
                set_err(ctx, "%s: class %u of alternative %u is empty: it matches nothing", who, k, j);
                return HUFE_ARGUMENT;
            }
            t->t.full[bit >> 5] |= 1u << (bit & 31u);
        }
        const uint32_t last = hi - (len - 1u);
        t->starts[hi >> 5] |= 1u << (hi & 31u);
        t->t.first[last >> 5] |= 1u << (last & 31u);
        t->hl[j] = (uint16_t)(hi | (len << 8));
        if (len > *maxlen) *maxlen = len;
        hi -= len;                                                  /* (wraps behind the last alternative of a total of 64: not used again) */
    }
    return HUFE_OK;
}

extern "C" int hufgpu_find_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                               uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                               const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, uint64_t *d_pos, uint64_t pos_cap,
                               uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindAltArgs t;
    uint32_t maxlen = 0;
    const bool both = classes && alt_lens;
    if (both) {
        const int rc = find_alt_table(ctx, "find_any", classes, alt_lens, n_alts, NULL, &t, &maxlen);
        if (rc) return rc;
    }
    return find_call(ctx, "find_any", "classes, alt_lens", both ? classes : NULL, maxlen, d_stream, stream_len, d_block_offsets, nblocks,
                     d_sub_index, raw_size, blocksize, d_pos, pos_cap, d_block_counts, d_totals, d_block_errs, flags, stream, NULL, &t.t, &t);
}

extern "C" int hufgpu_find_records_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                       uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                       const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                       uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                                       uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindAltArgs t;
    uint32_t maxlen = 0;
    const bool both = classes && alt_lens;
    if (both) {
        const int rc = find_alt_table(ctx, "find_records_any", classes, alt_lens, n_alts, delim_set, &t, &maxlen);
        if (rc) return rc;
    }
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    return find_call(ctx, "find_records_any", "classes, alt_lens", both ? classes : NULL, maxlen, d_stream, stream_len, d_block_offsets,
                     nblocks, d_sub_index, raw_size, blocksize, d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs, flags, stream,
                     &rec, &t.t, &t);
}

extern "C" int hufgpu_find_records_select(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                          uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                          const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                          uint32_t select, uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint64_t rec_cap,
                                          uint32_t max_len, uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                          uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT) {
        set_err(ctx, "find_records_select: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
        return HUFE_ARGUMENT;
    }
    FindAltArgs t;
    uint32_t maxlen = 0;
    const bool both = classes && alt_lens;
    if (both) {
        const int rc = find_alt_table(ctx, "find_records_select", classes, alt_lens, n_alts, delim_set, &t, &maxlen);
        if (rc) return rc;
    }
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    return find_call(ctx, "find_records_select", "classes, alt_lens", both ? classes : NULL, maxlen, d_stream, stream_len, d_block_offsets,
                     nblocks, d_sub_index, raw_size, blocksize, d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs, flags, stream,
                     &rec, &t.t, &t, &sel);
}

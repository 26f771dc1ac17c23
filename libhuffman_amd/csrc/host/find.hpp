/* find.hpp - the search family of include/huffman_gpu.h: hufgpu_find_bytes, hufgpu_find_pattern, hufgpu_find_classes and
   hufgpu_find_any give the positions of a set of byte values, of a pattern, of a pattern of sets, of any of several such
   patterns; hufgpu_find_records, hufgpu_find_records_classes, hufgpu_find_records_any and hufgpu_find_records_select give
   the records - the pieces between delimiters - that hold one (or do not), and their numbers; hufgpu_find_records_context
   gives the records around them as well; hufgpu_find_any_anchored and hufgpu_find_records_anchored are hufgpu_find_any and
   the context call for the matches that begin or end at a record's or a word's edge; hufgpu_find_any_quant and
   hufgpu_find_records_quant are those two for patterns with optional positions; hufgpu_find_records_terms is the
   context call for the records that hold all of several terms, or all of them in order; hufgpu_find_any_expr and
   hufgpu_find_records_expr take anchors, terms and optional positions together; hufgpu_find_any_spans is the expr positions
   call with the length of the longest form at every start.  All enqueue-only.  A
   wrapper describes its call in three structs; find_call checks them (find_check, no HIP call), fills the kernels'
   arguments and grows the workspace (find_fill) and enqueues the chain of kernels/find.hpp (find_enqueue).
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

static_assert(FIND_PAT_MAX == HUFGPU_FIND_PATTERN_MAX, "kernels/find.hpp and include/huffman_gpu.h");
static_assert(FIND_REC_NO_UNKNOWN == HUFGPU_REC_NO_UNKNOWN, "kernels/find.hpp and include/huffman_gpu.h");
static_assert(FIND_TERMS_MAX == HUFGPU_FIND_TERMS_MAX, "kernels/find.hpp and include/huffman_gpu.h");

/* an argument is wrong: the words for it, and the status */
template <typename... A>
static int find_bad(hufgpu_ctx_t *ctx, const char *fmt, A... a)
{
    set_err(ctx, fmt, a...);
    return HUFE_ARGUMENT;
}

/* where the stream is */
struct FindStream {
    const void *d_stream;
    uint64_t stream_len;
    const uint64_t *d_block_offsets;
    uint64_t nblocks;
    const void *d_sub_index;
    uint64_t raw_size, blocksize;
};

/* where the answers go: the records' calls have their d_rec_pos / rec_cap in d_pos / cap */
struct FindOut {
    uint64_t *d_pos;
    uint64_t cap;
    uint64_t *d_block_counts, *d_totals;
    int32_t *d_block_errs;
};

/* what hufgpu_find_records has beyond the pattern call */
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

/* what hufgpu_find_records_context has beyond the select call */
struct FindCtxCall {
    uint32_t before, after;
    uint8_t *d_rec_sel;                     /* optional */
};

/* what hufgpu_find_any_anchored and hufgpu_find_records_anchored have beyond their older calls, with anchors != 0: the two
 * boundary sets that the anchors, delim_set and word_set come to (find_anc_sets) */
struct FindAncCall {
    uint32_t anchors;
    uint8_t front[32];                      /* BOL / WORD: the bytes that may stand in front of a match */
    uint8_t behind[32];                     /* EOL / WORD: ... and behind one */
};

/* what hufgpu_find_records_terms has beyond the context call, with two terms or more: the kernels' description of the terms
 * (find_term_split fills the host's part of it, find_fill the workspace's) and the mode */
struct FindTermCall {
    FindTerms t;
    bool ordered;
};

/* what hufgpu_find_any_spans has beyond the expr positions call: where the lengths and the flags go, and - filled by
 * find_span_tables once the call's own checks have passed - either the one length of all forms (`fixed`: find_emit_len_kernel in
 * the place of find_emit_kernel) or find_span_kernel's forward table */
struct FindSpanCall {
    uint32_t *d_len;
    uint8_t *d_open;                        /* optional */
    bool fixed;
    uint32_t value;
    FindSpanArgs args;
};

/* What is looked for: `who` words the errors, `key` is the set (plen = 0) or the pattern of plen bytes, `key_name` its name;
 * rec is NULL but for the records' calls.  cls is NULL but for the class calls: then `key` is the caller's array of plen
 * classes, which find_call only checks for NULL and never reads - its wrapper has read it -, and cls is the table made
 * from it.  alt is NULL but for the any-of calls: then cls is alt's table (several alternatives in its 64 bits), plen is the
 * LONGEST alternative's length - what the edges workspace and the seam launch follow - and alt goes to the kernels.
 * sel is NULL but for the select and the context call: the any-of records' call with up to three launches more.
 * cx is NULL but for the context call, which is the select call with a dilation of the selected records' mask.
 * anc is NULL but for the anchored calls with an anchor: then alt's table holds one position more an alternative when
 * the byte behind a match is tested, and find_anchor_kernel runs when the byte in front is.
 * term is NULL but for the terms' call with two terms or more: the walk and the seam kernel then keep a mask a term, and
 * find_rec_mark_kernel runs once a term in front of find_rec_all_kernel (and find_rec_seq_kernel).
 * opt is NULL but for the quant calls with an optional position: then alt is opt's table, plen the longest alternative's
 * position count, and the walk and the seam kernel close the state over the optional positions (find_opt_masks).
 * expr is NULL but for the expr calls where they cross those three: optional positions with a tested byte behind a match,
 * and two terms or more with an optional position or an anchor.  Then opt is expr's (its masks 0 without an optional
 * position), and the walk and the seam kernel are the ones with the closure, the seam kernel's with the data's end.
 * span is NULL but for the span call: the expr positions call with a length a start, written behind the whole chain. */
struct FindKey {
    const char *who, *key_name;
    const uint8_t *key;
    uint32_t plen;
    const FindRecCall *rec;
    const FindClsTable *cls;
    FindAltArgs *alt;
    const FindSelCall *sel;
    const FindCtxCall *cx;
    const FindAncCall *anc;
    FindTermCall *term;
    FindOptArgs *opt;
    FindExprArgs *expr;
    FindSpanCall *span;
};

/* does the context call widen the answer: with both distances 0 it is the select call, maybe with flags */
static bool find_widens(const FindKey &k) { return k.cx && (k.cx->before | k.cx->after) != 0u; }

/* is the byte in front of a match tested (find_anchor_kernel), the byte behind it (a table position and find_anc_seam_kernel),
 * and does the call need a third mask: the records' own delimiter mask cannot be the boundary mask of a word, and a records
 * walk has room for one set next to the table, so find_sub_kernel walks the stream once more with the boundary set */
static bool find_anc_front(const FindKey &k) { return k.anc && (k.anc->anchors & (HUFGPU_ANCHOR_BOL | HUFGPU_ANCHOR_WORD)) != 0u; }
static bool find_anc_behind(const FindKey &k) { return k.anc && (k.anc->anchors & (HUFGPU_ANCHOR_EOL | HUFGPU_ANCHOR_WORD)) != 0u; }
static bool find_anc_third(const FindKey &k) { return k.rec && k.anc && (k.anc->anchors & HUFGPU_ANCHOR_WORD) != 0u; }

/* the layout's blocks in chunks, mask words and tiles */
struct FindGeometry {
    uint64_t blocksize, cpb, wpb, tpb;
};
static FindGeometry find_geometry(const FindStream &in)
{
    const uint64_t bs = in.blocksize ? in.blocksize : in.raw_size;
    return {bs, (bs + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS, (bs + DSUB_SPL - 1) / DSUB_SPL, (bs + HUF_SUB_TILE - 1) / HUF_SUB_TILE};
}

/* the arguments' checks, in the order in which they speak; no HIP call */
static int find_check(hufgpu_ctx_t *ctx, const FindStream &in, const FindOut &out, const FindKey &k)
{
    const char *who = k.who;
    if (!k.key || !out.d_totals) return find_bad(ctx, "%s: the %s and d_totals are required", who, k.key_name);
    if (k.rec) {
        if (!k.rec->delim_set) return find_bad(ctx, "%s: the delim_set is required (32 zero bytes: the data is one record)", who);
        for (uint32_t i = 0; !k.cls && i < k.plen; i++) {           /* (the classes' wrapper has looked at its classes) */
            if ((k.rec->delim_set[k.key[i] >> 3] >> (k.key[i] & 7)) & 1)
                return find_bad(ctx, "%s: byte %u of the pattern (value %u) is a delimiter: a match lies inside one record", who, i, k.key[i]);
        }
        if (out.cap > 0 && (!out.d_pos || !k.rec->d_len))
            return find_bad(ctx, "%s: rec_cap %llu needs d_rec_pos and d_rec_len", who, (unsigned long long)out.cap);
    } else if (out.cap > 0 && !out.d_pos) {
        return find_bad(ctx, "%s: pos_cap %llu needs d_pos", who, (unsigned long long)out.cap);
    } else if (out.cap > 0 && k.span && !k.span->d_len) {
        return find_bad(ctx, "%s: pos_cap %llu needs d_len", who, (unsigned long long)out.cap);
    }
    if (in.nblocks == 0) {
        if (in.raw_size != 0)
            return find_bad(ctx, "%s: (raw_size, blocksize) must be those of the encode that wrote these 0 blocks", who);
    } else {
        if (!in.d_stream || !in.d_block_offsets || !out.d_block_errs)
            return find_bad(ctx, "%s: the stream, its block index and d_block_errs are required", who);
        if (!in.d_sub_index || ((uintptr_t)in.d_sub_index & 7u))
            return find_bad(ctx, "%s: needs the stream's sub-index in an 8-byte aligned buffer", who);
        const FindGeometry g = find_geometry(in);
        if (in.raw_size == 0 || g.blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(in.raw_size, g.blocksize) != in.nblocks ||
            in.nblocks > 0x7fffffffull || in.nblocks * g.tpb > 0x7fffffffull)
            return find_bad(ctx, "%s: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks (at most 2^31 - 1 tiles)",
                            who, (unsigned long long)in.nblocks);
    }
    if (!ctx) return find_bad(NULL, "%s: needs a context (there is no CPU path)", who);
    return HUFE_OK;
}

/* the workspace for this call's route, and the arguments of its kernels: ra as a whole for the records' kernels, ra.p and
 * ra.p.f for the others (a route that has no use for a member leaves it 0) */
static int find_fill(hufgpu_ctx_t *ctx, const FindStream &in, const FindOut &out, const FindKey &k, uint32_t flags, FindRecArgs &ra)
{
    const FindGeometry g = find_geometry(in);
    const uint64_t nwords = in.nblocks * g.wpb, ntiles = in.nblocks * g.tpb;
    int rc = ensure_find_ws(ctx, nwords, ntiles);
    if (!rc && k.plen > 1) rc = grow_ws(ctx, G_FIND_EDGES, ntiles);                 /* (one byte has no seams: no edges) */
    const bool front = find_anc_front(k);                           /* (the positions call then walks as a records call does) */
    if (!rc && (k.rec || front)) rc = grow_ws2(ctx, G_FIND_REC_WORDS, nwords, G_FIND_REC_TILES, ntiles);
    if (!rc && find_anc_third(k)) rc = grow_ws2(ctx, G_FIND_ANC_WORDS, nwords, G_FIND_ANC_TILES, ntiles);
    if (!rc && k.sel && k.sel->d_rec_no && out.cap > 0) rc = grow_ws(ctx, G_FIND_SEL, 1);
    if (!rc && find_widens(k)) rc = grow_ws2(ctx, G_FIND_CTX_WORDS, nwords, G_FIND_CTX_TILES, ntiles);
    if (!rc && k.term) rc = grow_ws2(ctx, G_FIND_TERM_WORDS, k.term->t.n_terms * nwords, G_FIND_TERM_TILES, k.term->t.n_terms * ntiles);
    for (uint32_t t = 0; !rc && k.term && k.term->ordered && t < k.term->t.n_terms; t++) rc = grow_ws(ctx, G_FIND_TERM_SCAN0 + (int)t, ntiles);
    if (rc) return rc;
    memset(&ra, 0, sizeof(ra));
    FindPatArgs &pa = ra.p;
    FindArgs &fa = pa.f;
    fa.s = sub_stream_args(in.d_stream, in.stream_len, in.d_block_offsets, in.nblocks, in.d_sub_index, in.raw_size, g.blocksize, flags);
    fa.cpb = (uint32_t)g.cpb;
    const uint8_t *set = k.rec ? k.rec->delim_set : front ? k.anc->front : k.plen == 0 ? k.key : NULL;  /* the delimiters, the boundary bytes, or the values looked for */
    for (int i = 0; set && i < 32; i++) fa.set[i >> 2] |= (uint32_t)set[i] << (8 * (i & 3));
    for (uint32_t i = 0; !k.cls && i < k.plen; i++) pa.pat[i >> 2] |= (uint32_t)k.key[i] << (8 * (i & 3));
    if (k.plen) {
        pa.plen = k.plen;
        pa.edges = ctx->d_fedges;
    }
    fa.bitmap = ctx->d_fbitmap;
    fa.wpb = g.wpb;
    fa.tcnt = ctx->d_ftcnt;
    fa.tpb = g.tpb;
    fa.ntiles = ntiles;
    fa.scan = ctx->find_scan;
    fa.scan.total = out.d_totals;
    fa.pos = out.d_pos;
    fa.pos_cap = out.cap;
    fa.block_counts = out.d_block_counts;
    fa.totals = out.d_totals;
    fa.errs = out.d_block_errs;
    if (k.rec) {
        ra.dbits = ctx->d_frdbits;
        ra.dcnt = ctx->d_frdcnt;
        ra.rbits = ctx->d_frrbits;
        ra.rcnt = ctx->d_frrcnt;
        ra.dscan = ctx->frec_scan;
        ra.dscan.total = ctx->d_frdtotal;
        ra.len = k.rec->d_len;
        ra.clip = k.rec->max_len ? k.rec->max_len : 0xffffffffu;
    } else if (front) {
        ra.dbits = ctx->d_frdbits;
        ra.dcnt = ctx->d_frdcnt;
    }
    if (k.term) {
        FindTerms &tm = k.term->t;
        tm.mbits = ctx->d_ftmbits;
        tm.mcnt = ctx->d_ftmcnt;
        tm.rbits = ctx->d_ftrbits;
        tm.rcnt = ctx->d_ftrcnt;
        tm.nwords = nwords;
    }
    return HUFE_OK;
}

/* the walk of the stream and, for a pattern of two bytes or more, the seams of its tiles: the one place where a route
 * chooses its kernels.  The any-of table goes with the launches' own arguments. */
static void find_enqueue_walk(hufgpu_ctx_t *ctx, const FindKey &k, const FindRecArgs &ra, dim3 walk, dim3 seams, dim3 tiles, hipStream_t s)
{
    const dim3 wt(FIND_THREADS), st(FIND_SEAM_THREADS);
    const bool rec = k.rec != NULL, seam = k.plen > 1;
    const bool front = find_anc_front(k), third = find_anc_third(k);
    /* the bytes' walk with the boundary set, into a mask and tile counts of its own: the same checks, so the same
     * statuses a second time, and no word of the first walk is touched */
    const auto third_walk = [&]() {
        FindArgs ba = ra.p.f;
        memset(ba.set, 0, sizeof(ba.set));
        for (int i = 0; i < 32; i++) ba.set[i >> 2] |= (uint32_t)k.anc->front[i] << (8 * (i & 3));
        ba.bitmap = ctx->d_fabits;
        ba.tcnt = ctx->d_fatcnt;
        find_sub_kernel<<<walk, wt, 0, s>>>(ba);
    };
    /* the byte in front of a match, over the mask and counts of `f` */
    const auto anchor = [&](const FindArgs &f) {
        const FindAnchorArgs fa = {f, third ? ctx->d_fabits : ra.dbits};
        find_anchor_kernel<<<tiles, dim3(FIND_EMIT_THREADS), 0, s>>>(fa);
    };
    if (k.term && k.expr) {
        /* the terms' walk with the closure; the anchors bind the outer edges: the byte behind a match is a position of the
         * LAST term's alternatives, the byte in front is looked at for term 0's mask and counts */
        FindExprArgs &x = *k.expr;
        x.qa.a.r = ra;
        x.t = k.term->t;
        if (x.t.n_terms == 2) find_rec_term_opt_sub_kernel<2><<<walk, wt, 0, s>>>(x);
        else if (x.t.n_terms == 3) find_rec_term_opt_sub_kernel<3><<<walk, wt, 0, s>>>(x);
        else find_rec_term_opt_sub_kernel<FIND_TERMS_MAX><<<walk, wt, 0, s>>>(x);
        if (third) third_walk();
        if (seam) find_term_opt_seam_kernel<<<seams, st, 0, s>>>(x);
        if (front) {
            FindArgs f0 = ra.p.f;
            f0.bitmap = x.t.mbits;
            f0.tcnt = x.t.mcnt;
            anchor(f0);
        }
    } else if (k.term) {
        /* a mask a term, and a kernel for each number of terms: a mask that is not needed still costs registers */
        k.alt->r = ra;
        const FindTermArgs ta = {*k.alt, k.term->t};
        if (ta.t.n_terms == 2) find_rec_term_sub_kernel<2><<<walk, wt, 0, s>>>(ta);
        else if (ta.t.n_terms == 3) find_rec_term_sub_kernel<3><<<walk, wt, 0, s>>>(ta);
        else find_rec_term_sub_kernel<FIND_TERMS_MAX><<<walk, wt, 0, s>>>(ta);
        if (seam) find_term_seam_kernel<<<seams, st, 0, s>>>(ta);
    } else if (k.opt) {
        k.opt->a.r = ra;
        /* (the expr calls, with an anchor: the records' form whenever the byte in front is tested, as below) */
        if (rec || front) find_rec_opt_sub_kernel<<<walk, wt, 0, s>>>(*k.opt);
        else find_opt_sub_kernel<<<walk, wt, 0, s>>>(*k.opt);
        if (third) third_walk();
        if (seam && k.expr) find_opt_anc_seam_kernel<<<seams, st, 0, s>>>(*k.expr);
        else if (seam) find_opt_seam_kernel<<<seams, st, 0, s>>>(*k.opt);
        if (front) anchor(ra.p.f);
    } else if (k.alt) {
        k.alt->r = ra;
        if (rec || front) find_rec_alt_sub_kernel<<<walk, wt, 0, s>>>(*k.alt);
        else find_alt_sub_kernel<<<walk, wt, 0, s>>>(*k.alt);
        if (third) third_walk();
        if (seam && find_anc_behind(k)) find_anc_seam_kernel<<<seams, st, 0, s>>>(*k.alt);
        else if (seam) find_alt_seam_kernel<<<seams, st, 0, s>>>(*k.alt);
        if (front) anchor(ra.p.f);
    } else if (k.cls) {
        const FindClsArgs ca = {ra, *k.cls};
        if (rec) find_rec_cls_sub_kernel<<<walk, wt, 0, s>>>(ca);
        else find_cls_sub_kernel<<<walk, wt, 0, s>>>(ca);
        if (seam) find_cls_seam_kernel<<<seams, st, 0, s>>>(ca);
    } else if (k.plen) {
        if (rec) find_rec_sub_kernel<<<walk, wt, 0, s>>>(ra);
        else find_pat_sub_kernel<<<walk, wt, 0, s>>>(ra.p);
        if (seam) find_seam_kernel<<<seams, st, 0, s>>>(ra.p);
    } else {
        find_sub_kernel<<<walk, wt, 0, s>>>(ra.p.f);
    }
}

/* the chain of kernels/find.hpp for this call */
static int find_enqueue(hufgpu_ctx_t *ctx, const FindOut &out, const FindKey &k, FindRecArgs &ra, hipStream_t s)
{
    FindArgs &fa = ra.p.f;
    const uint64_t nblocks = fa.s.nblocks, sper = FIND_SEAM_THREADS / 64, eper = FIND_EMIT_THREADS / 64;
    const dim3 walk((unsigned)(nblocks * fa.cpb)), seams((unsigned)((fa.ntiles + sper - 1) / sper));
    const dim3 tiles((unsigned)((fa.ntiles + eper - 1) / eper)), groups((unsigned)((fa.ntiles + SCAN_GROUP - 1) / SCAN_GROUP));
    const dim3 blocks(grid256(nblocks)), et(FIND_EMIT_THREADS);
    HIP_OK(ctx, hipMemsetAsync(out.d_block_errs, 0, nblocks * sizeof(int32_t), s));
    HIP_OK(ctx, hipMemsetAsync(out.d_totals, 0, 4 * sizeof(uint64_t), s));
    const bool widens = find_widens(k);
    if (k.rec) {
        /* the terms' call: mark writes a mask and counts a term, and find_rec_all_kernel stores every word of ra's */
        const uint64_t nt = k.term ? k.term->t.n_terms : 1;
        HIP_OK(ctx, hipMemsetAsync(k.term ? k.term->t.rbits : ra.rbits, 0, nt * nblocks * fa.wpb * sizeof(uint32_t), s));
        HIP_OK(ctx, hipMemsetAsync(k.term ? k.term->t.rcnt : ra.rcnt, 0, nt * fa.ntiles * sizeof(uint32_t), s));
        if (k.term && k.term->ordered) HIP_OK(ctx, hipMemsetAsync(ctx->d_fttotals, 0, 4 * FIND_TERMS_MAX * sizeof(uint64_t), s));
        if (widens) HIP_OK(ctx, hipMemsetAsync(ctx->d_fctotals, 0, 4 * sizeof(uint64_t), s));
    }
    find_enqueue_walk(ctx, k, ra, walk, seams, tiles, s);
    const uint32_t *sbits = ra.rbits;                               /* the selected records' mask, whatever the emit kernel reads */
    if (k.rec) {
        /* from the walk's two masks to the records' starts and their counts by tile; scan, finish and emit then take the
         * records of a tile as they take its matches */
        FindCtxArgs ca;
        if (widens) {                                               /* (a block that is not served lies farther away than either distance) */
            ca = {ra, ctx->d_fcbits, ctx->d_fccnt, ctx->fctx_scan, k.cx->before, k.cx->after};
            ca.rscan.total = ctx->d_fctotals;
            find_ctx_dscan_kernel<<<groups, dim3(64), 0, s>>>(ca);                      /* (a wave a group) */
        } else {
            find_rec_dscan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(ra);
        }
        if (k.term) {
            /* mark as it is, once a term, from term t's match words and counts into term t's record mask and counts; then
             * the records that every term marked, and of those - ordered - the ones that hold the terms one behind the other */
            const FindTerms &tm = k.term->t;
            FindSeqArgs qa = {ra, tm, {}};
            for (uint32_t t = 0; t < tm.n_terms; t++) {
                FindRecArgs ta = ra;
                ta.p.f.bitmap = tm.mbits + t * tm.nwords;
                ta.p.f.tcnt = tm.mcnt + t * fa.ntiles;
                ta.rbits = tm.rbits + t * tm.nwords;
                ta.rcnt = tm.rcnt + t * fa.ntiles;
                find_rec_mark_kernel<<<tiles, et, 0, s>>>(ta);
                if (k.term->ordered) {                              /* the term's match counts into a scan and totals of the workspace's own */
                    FindArgs sfa = ta.p.f;
                    sfa.scan = ctx->fterm_scan[t];
                    sfa.scan.total = sfa.totals = ctx->d_fttotals + 4 * t;
                    find_scan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(sfa);
                    qa.tscan[t] = sfa.scan;
                }
            }
            const FindAllArgs aa = {ra, tm};
            find_rec_all_kernel<<<tiles, et, 0, s>>>(aa);
            if (k.term->ordered) find_rec_seq_kernel<<<tiles, et, 0, s>>>(qa);
        } else {
            find_rec_mark_kernel<<<tiles, et, 0, s>>>(ra);
        }
        if (k.sel && (k.sel->select & HUFGPU_SELECT_INVERT)) find_rec_invert_kernel<<<tiles, et, 0, s>>>(ra);   /* over mark's words and counts */
        fa.tcnt = ra.rcnt;
        if (widens) {
            /* the selected records' counts into a scan of this call's own - find_scan_kernel, with four words of the
             * workspace as its totals -, then the records to report into the second mask, which the rest of the chain takes */
            FindArgs sfa = fa;
            sfa.scan = ca.rscan;
            sfa.totals = ctx->d_fctotals;
            find_scan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(sfa);
            find_rec_ctx_kernel<<<tiles, et, 0, s>>>(ca);
            ra.rbits = ca.cbits;
            fa.tcnt = ra.rcnt = ca.ccnt;
        }
    }
    find_scan_kernel<<<groups, dim3(SCAN_GROUP), 0, s>>>(fa);
    find_finish_kernel<<<blocks, dim3(256), 0, s>>>(fa);
    const bool numbers = k.sel && k.sel->d_rec_no && out.cap > 0, flags = k.cx && k.cx->d_rec_sel && out.cap > 0;
    const FindSelArgs sa = {ra, numbers ? k.sel->d_rec_no : NULL, ctx->d_fsel_first};
    if (numbers) {                                                  /* the numbers need the first block that is not served */
        HIP_OK(ctx, hipMemsetAsync(sa.first_bad, 0xff, sizeof(uint64_t), s));
        find_rec_first_bad_kernel<<<blocks, dim3(256), 0, s>>>(sa);
    }
    if (flags) {                                                    /* is a reported record one of the selected: its bit in sbits */
        const FindCtxEmitArgs ea = {sa, sbits, k.cx->d_rec_sel};
        if (numbers) find_ctx_emit_no_kernel<<<tiles, et, 0, s>>>(ea);
        else find_ctx_emit_kernel<<<tiles, et, 0, s>>>(ea);
    } else if (numbers) {
        find_rec_emit_no_kernel<<<tiles, et, 0, s>>>(sa);
    } else if (out.cap > 0 && k.rec) {
        find_rec_emit_kernel<<<tiles, et, 0, s>>>(ra);
    } else if (out.cap > 0 && k.span && k.span->fixed) {
        const FindEmitLenArgs ea = {fa, k.span->d_len, k.span->d_open, k.span->value};
        find_emit_len_kernel<<<tiles, et, 0, s>>>(ea);
    } else if (out.cap > 0) {
        find_emit_kernel<<<tiles, et, 0, s>>>(fa);
    }
    if (out.cap > 0 && k.span && !k.span->fixed) {
        /* the walk's grid once more: the tiles with a start below the cap are decoded again, the others cost a look */
        FindSpanArgs &sa = k.span->args;
        sa.qa.a.r = ra;
        sa.len = k.span->d_len;
        sa.open = k.span->d_open;
        find_span_kernel<<<walk, dim3(FIND_THREADS), 0, s>>>(sa);
    }
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

static int find_call(hufgpu_ctx_t *ctx, const FindStream &in, const FindOut &out, const FindKey &k, uint32_t flags, void *stream)
{
    int rc = find_check(ctx, in, out, k);
    if (rc) return rc;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    if (in.nblocks == 0) {
        HIP_OK(ctx, hipMemsetAsync(out.d_totals, 0, 4 * sizeof(uint64_t), s));
        return HUFE_OK;
    }
    FindRecArgs ra;
    rc = find_fill(ctx, in, out, k, flags, ra);
    return rc ? rc : find_enqueue(ctx, out, k, ra, s);
}

/* a pattern's length, as its call words it */
static int find_pattern_len(hufgpu_ctx_t *ctx, const char *who, uint32_t plen)
{
    if (plen >= 1 && plen <= HUFGPU_FIND_PATTERN_MAX) return HUFE_OK;
    return find_bad(ctx, "%s: pattern_len %u is not 1 to %d", who, plen, HUFGPU_FIND_PATTERN_MAX);
}

extern "C" int hufgpu_find_bytes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                 uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                 const uint8_t set[32], uint64_t *d_pos, uint64_t pos_cap, uint64_t *d_block_counts,
                                 uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    const FindKey k = {"find_bytes", "set", set, 0, NULL, NULL, NULL, NULL, NULL, NULL};
    return find_call(ctx, in, out, k, flags, stream);
}

extern "C" int hufgpu_find_pattern(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t *pattern, uint32_t pattern_len, uint64_t *d_pos, uint64_t pos_cap,
                                   uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (pattern && find_pattern_len(ctx, "find_pattern", pattern_len)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    const FindKey k = {"find_pattern", "pattern", pattern, pattern_len, NULL, NULL, NULL, NULL, NULL, NULL};
    return find_call(ctx, in, out, k, flags, stream);
}

extern "C" int hufgpu_find_records(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t delim_set[32], const uint8_t *pattern, uint32_t pattern_len, uint64_t *d_rec_pos,
                                   uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len, uint64_t *d_block_counts,
                                   uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (pattern && find_pattern_len(ctx, "find_records", pattern_len)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindKey k = {"find_records", "pattern", pattern, pattern_len, &rec, NULL, NULL, NULL, NULL, NULL};
    return find_call(ctx, in, out, k, flags, stream);
}

/* One alternative's `len` classes into the transposed table (kernels/find.hpp): position k at bit hi - k of m[v], for
 * every value v of the class; `full` gets every position's bit, `first` that of the LAST position.  No class may be empty
 * or hold a delimiter; `of` names the alternative in those errors ("the pattern": the class calls' only one).
 * `behind` (the anchored calls): one position more, at bit hi - len, with that class - an internal one, which may be empty
 * or hold a delimiter - and the automaton starts there. */
static int find_table_add(hufgpu_ctx_t *ctx, const char *who, const char *of, const uint8_t *cl, uint32_t len, uint32_t hi,
                          const uint8_t *delim_set, FindClsTable *t, const uint8_t *behind = NULL)
{
    for (uint32_t k = 0; k < len; k++, cl += 32) {
        const uint32_t bit = hi - k;
        bool any = false;
        for (uint32_t v = 0; v < 256; v++) {
            if (!((cl[v >> 3] >> (v & 7)) & 1)) continue;
            if (delim_set && ((delim_set[v >> 3] >> (v & 7)) & 1))
                return find_bad(ctx, "%s: class %u of %s holds a delimiter (value %u): a match lies inside one record", who, k, of, v);
            any = true;
            t->m[v][bit >> 5] |= 1u << (bit & 31u);
        }
        if (!any) return find_bad(ctx, "%s: class %u of %s is empty: it matches nothing", who, k, of);
        t->full[bit >> 5] |= 1u << (bit & 31u);
    }
    uint32_t last = hi - (len - 1u);
    if (behind) {
        last--;
        for (uint32_t v = 0; v < 256; v++) {
            if ((behind[v >> 3] >> (v & 7)) & 1) t->m[v][last >> 5] |= 1u << (last & 31u);
        }
        t->full[last >> 5] |= 1u << (last & 31u);
    }
    t->first[last >> 5] |= 1u << (last & 31u);
    return HUFE_OK;
}

/* The class calls' own checks - the length, and find_table_add's - and their table: one alternative at the bits
 * 63 ... 64 - plen.  `classes` is not NULL; a NULL delim_set is find_check's to word. */
static int find_cls_table(hufgpu_ctx_t *ctx, const char *who, const uint8_t *classes, uint32_t plen, const uint8_t *delim_set,
                          FindClsTable *t)
{
    if (find_pattern_len(ctx, who, plen)) return HUFE_ARGUMENT;
    memset(t, 0, sizeof(*t));
    return find_table_add(ctx, who, "the pattern", classes, plen, 63, delim_set, t);
}

extern "C" int hufgpu_find_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                   const uint8_t *classes, uint32_t pattern_len, uint64_t *d_pos, uint64_t pos_cap,
                                   uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindClsTable t;
    if (classes && find_cls_table(ctx, "find_classes", classes, pattern_len, NULL, &t)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    const FindKey k = {"find_classes", "classes", classes, pattern_len, NULL, &t, NULL, NULL, NULL, NULL};
    return find_call(ctx, in, out, k, flags, stream);
}

extern "C" int hufgpu_find_records_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                           uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                           const uint8_t delim_set[32], const uint8_t *classes, uint32_t pattern_len,
                                           uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                                           uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindClsTable t;
    if (classes && find_cls_table(ctx, "find_records_classes", classes, pattern_len, delim_set, &t)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindKey k = {"find_records_classes", "classes", classes, pattern_len, &rec, &t, NULL, NULL, NULL, NULL};
    return find_call(ctx, in, out, k, flags, stream);
}

/* The any-of calls' own checks - 1 to 64 alternatives, none of length 0, lengths that sum to at most 64, and
 * find_table_add's - and their table (kernels/find.hpp, FindAltArgs: alternative 0 at the bits 63 ... 64 - len_0,
 * alternative 1 below it).  `classes` and `alt_lens` are not NULL; the total is looked at before `classes` is read.
 * *maxlen: the longest alternative's length.  `behind` (the anchored calls): every alternative gets one position more, that
 * class, which takes a bit of the state and counts into *maxlen.  `bfrom` (the expr call's ordered terms): the alternatives
 * from that one on only - the last term's. */
static int find_alt_table(hufgpu_ctx_t *ctx, const char *who, const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                          const uint8_t *delim_set, FindAltArgs *t, uint32_t *maxlen, const uint8_t *behind = NULL, uint32_t bfrom = 0)
{
    if (n_alts == 0 || n_alts > HUFGPU_FIND_PATTERN_MAX)
        return find_bad(ctx, "%s: n_alts %u is not 1 to %d", who, n_alts, HUFGPU_FIND_PATTERN_MAX);
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_alts; j++) {
        if (alt_lens[j] == 0) return find_bad(ctx, "%s: alternative %u has length 0: it would match everywhere", who, j);
        total += alt_lens[j];
    }
    if (total > HUFGPU_FIND_PATTERN_MAX)
        return find_bad(ctx, "%s: the lengths of the %u alternatives sum to %llu, above %d", who, n_alts, (unsigned long long)total,
                        HUFGPU_FIND_PATTERN_MAX);
    if (behind && bfrom == 0 && total + n_alts > HUFGPU_FIND_PATTERN_MAX)
        return find_bad(ctx, "%s: the lengths of the %u alternatives and one boundary position each sum to %llu, above %d", who, n_alts,
                        (unsigned long long)(total + n_alts), HUFGPU_FIND_PATTERN_MAX);
    if (behind && bfrom != 0 && total + (n_alts - bfrom) > HUFGPU_FIND_PATTERN_MAX)
        return find_bad(ctx, "%s: the lengths of the %u alternatives and one boundary position for each of the last term's %u sum to %llu, above %d",
                        who, n_alts, n_alts - bfrom, (unsigned long long)(total + (n_alts - bfrom)), HUFGPU_FIND_PATTERN_MAX);
    memset(t, 0, sizeof(*t));
    t->n_alts = n_alts;
    *maxlen = 0;
    uint32_t hi = 63;
    for (uint32_t j = 0; j < n_alts; j++) {
        const uint8_t *bj = j >= bfrom ? behind : NULL;
        const uint32_t len = alt_lens[j], bits = len + (bj ? 1u : 0u);
        char of[32];
        snprintf(of, sizeof(of), "alternative %u", j);
        if (find_table_add(ctx, who, of, classes, len, hi, delim_set, &t->t, bj)) return HUFE_ARGUMENT;
        t->starts[hi >> 5] |= 1u << (hi & 31u);
        t->hl[j] = (uint16_t)(hi | (bits << 8));
        if (bits > *maxlen) *maxlen = bits;
        classes += 32u * len;
        hi -= bits;                                                 /* (wraps behind the last alternative of a total of 64: not used again) */
    }
    return HUFE_OK;
}

/* The terms of a table that find_alt_table has made, term_alts[t] alternatives each in the table's order: the start bits a
 * term, the term's index into bits 6 and 7 of its alternatives' hl (a hi is 0 to 63, a length sits from bit 8 on), and the
 * length of the term's first alternative - of all of them in an ordered call, which find_term_check has seen to. */
static void find_term_split(FindAltArgs *t, const uint32_t *alt_lens, const uint32_t *term_alts, FindTermCall *term)
{
    FindTerms &tm = term->t;
    uint32_t j = 0;
    for (uint32_t q = 0; q < tm.n_terms; q++) {
        tm.len[q] = alt_lens[j];
        for (const uint32_t end = j + term_alts[q]; j < end; j++) {
            const uint32_t hi = t->hl[j] & 63u;
            tm.starts[q][hi >> 5] |= 1u << (hi & 31u);
            t->hl[j] = (uint16_t)(t->hl[j] | (q << 6));
        }
    }
}

/* The quant calls' own checks, behind find_alt_table's: an `optional` byte that is neither 0 nor 1, an alternative whose
 * positions are all optional.  Then, next to the table that find_alt_table has made in q->a, the three masks of
 * kernels/find.hpp's FindOpt and the wider `first`; *any: is there an optional position at all - without one the call is
 * the any-of call.  `optional` has one byte a position, in the order of `classes`.  `bfrom` (the expr calls): the alternatives
 * from that one on have a boundary position behind their own, a required one that `optional` has no byte for - so no run of
 * optional positions ends such an alternative, and its bit in `first` is the boundary's alone. */
static int find_opt_masks(hufgpu_ctx_t *ctx, const char *who, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                          FindOptArgs *q, bool *any, uint32_t bfrom = ~0u)
{
    const uint8_t *op = optional;
    for (uint32_t j = 0; j < n_alts; op += alt_lens[j++]) {
        uint32_t required = 0;
        for (uint32_t k = 0; k < alt_lens[j]; k++) {
            if (op[k] > 1)
                return find_bad(ctx, "%s: optional is %u at position %u of alternative %u: 0 (required) or 1 (may be left out)", who, op[k], k, j);
            required += op[k] == 0;
            *any |= op[k] != 0;
        }
        if (required == 0)
            return find_bad(ctx, "%s: every position of alternative %u is optional: it would match everywhere", who, j);
    }
    uint64_t first = 0, O = 0, I = 0, F = 0;
    op = optional;
    for (uint32_t j = 0; j < n_alts; op += alt_lens[j++]) {
        const uint32_t hi = q->a.hl[j] & 63u, own = alt_lens[j], len = own + (j >= bfrom ? 1u : 0u);
        const auto opt = [&](uint32_t at) { return at < own && op[at] != 0; };
        uint32_t k = len - 1u;                                      /* the positions that may hold a form's last byte */
        first |= 1ull << (hi - k);
        while (opt(k)) first |= 1ull << (hi - --k);                 /* (a required position stops it) */
        for (k = 0; k < len; k++) {
            if (!opt(k)) continue;
            const uint32_t top = k;
            while (opt(k + 1u)) k++;
            uint32_t low = k;                                       /* the maximal run top ... low */
            if (low == len - 1u) {                                  /* it ends the alternative: its lowest bit is its i, set by `first` */
                if (top == low) continue;
                low--;
            }
            for (uint32_t b = top; b <= low; b++) O |= 1ull << (hi - b);
            I |= 1ull << (hi - low - 1u);
            F |= 1ull << (hi - top);
        }
    }
    q->a.t.first[0] = (uint32_t)first;
    q->a.t.first[1] = (uint32_t)(first >> 32);
    q->q = {{(uint32_t)O, (uint32_t)(O >> 32)}, {(uint32_t)I, (uint32_t)(I >> 32)}, {(uint32_t)F, (uint32_t)(F >> 32)}};
    return HUFE_OK;
}

/* hufgpu_find_any_spans, behind the expr call's checks of the alternatives (so: 1 to 64 of them, lengths that sum to at most
 * 64 - 63 with `behind` -, no empty class, no alternative that is all optional): without an optional position and with one
 * length for all alternatives that length is the answer.  Else the forward table of kernels/find.hpp's FindSpanArgs:
 * find_alt_table and find_opt_masks as they are, over every alternative's classes and `optional` bytes in reverse order, and
 * with `behind` bit 0 of every entry that may stand behind a form. */
static int find_span_tables(const char *who, const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                            bool quant, const uint8_t *behind, FindSpanCall *span)
{
    span->fixed = !quant;
    span->value = alt_lens[0];
    for (uint32_t j = 1; j < n_alts; j++) span->fixed &= alt_lens[j] == alt_lens[0];
    if (span->fixed) return HUFE_OK;
    uint8_t rcl[HUFGPU_FIND_PATTERN_MAX * 32], rop[HUFGPU_FIND_PATTERN_MAX];
    for (uint32_t j = 0, at = 0; j < n_alts; at += alt_lens[j++]) {
        for (uint32_t i = 0, len = alt_lens[j]; i < len; i++) {
            memcpy(rcl + 32u * (at + i), classes + 32u * (at + len - 1u - i), 32);
            rop[at + i] = optional ? optional[at + len - 1u - i] : 0;
        }
    }
    FindSpanArgs &sa = span->args;
    memset(&sa, 0, sizeof(sa));
    uint32_t maxform = 0;
    bool any = false;
    if (find_alt_table(NULL, who, rcl, alt_lens, n_alts, NULL, &sa.qa.a, &maxform) ||
        find_opt_masks(NULL, who, alt_lens, n_alts, rop, &sa.qa, &any))
        return HUFE_ARGUMENT;                                       /* (cannot be: the call's own tables have been made of the same) */
    sa.behind = behind != NULL;
    for (uint32_t v = 0; behind && v < 256; v++) sa.qa.a.t.m[v][0] |= (uint32_t)((behind[v >> 3] >> (v & 7)) & 1);
    return HUFE_OK;
}

/* the nine any-of wrappers' call: the table, when both arrays are there (find_check words a missing one), then find_call */
static int find_alt_call(hufgpu_ctx_t *ctx, const char *who, const FindStream &in, const FindOut &out, const uint8_t *classes,
                         const uint32_t *alt_lens, uint32_t n_alts, const FindRecCall *rec, const FindSelCall *sel, const FindCtxCall *cx,
                         uint32_t flags, void *stream, const FindAncCall *anc = NULL, FindTermCall *term = NULL,
                         const uint32_t *term_alts = NULL, const uint8_t *optional = NULL, FindSpanCall *span = NULL)
{
    FindExprArgs x;                         /* (the older calls use its FindOptArgs, or that one's FindAltArgs, and nothing else) */
    FindOptArgs &q = x.qa;
    FindAltArgs &t = q.a;
    uint32_t maxlen = 0;
    bool quant = false;
    const bool both = classes && alt_lens;
    const uint8_t *behind = anc && (anc->anchors & (HUFGPU_ANCHOR_EOL | HUFGPU_ANCHOR_WORD)) ? anc->behind : NULL;
    /* anchors bind the outer edges of ordered terms: the byte behind a match is the last term's */
    const uint32_t bfrom = behind && term && term_alts ? n_alts - term_alts[term->t.n_terms - 1u] : 0u;
    if (both && find_alt_table(ctx, who, classes, alt_lens, n_alts, rec ? rec->delim_set : NULL, &t, &maxlen, behind, bfrom)) return HUFE_ARGUMENT;
    if (both && term) find_term_split(&t, alt_lens, term_alts, term);
    q.q = {};
    if (both && optional && find_opt_masks(ctx, who, alt_lens, n_alts, optional, &q, &quant, behind ? bfrom : ~0u)) return HUFE_ARGUMENT;
    if (both && optional && term && term->ordered) {               /* find_rec_seq_kernel needs every term's end but the last one's */
        const uint8_t *op = optional;
        for (uint32_t tq = 0, j = 0; tq + 1u < term->t.n_terms; tq++) {
            for (const uint32_t end = j + term_alts[tq]; j < end; op += alt_lens[j++]) {
                for (uint32_t i = 0; i < alt_lens[j]; i++) {
                    if (op[i])
                        return find_bad(ctx, "%s: position %u of alternative %u, in term %u, is optional: an ordered call allows optional positions in its last term only",
                                        who, i, j, tq);
                }
            }
        }
    }
    /* where the call crosses what the older ones keep apart: the kernels with the closure and the data's end */
    const bool cross = both && (term ? (quant || anc) : (quant && behind));
    x.bnd[0] = x.bnd[1] = 0;
    for (uint32_t j = bfrom; cross && behind && j < n_alts; j++) {
        const uint32_t bit = (t.hl[j] & 63u) - alt_lens[j];
        x.bnd[bit >> 5] |= 1u << (bit & 31u);
    }
    if (both && span && find_span_tables(who, classes, alt_lens, n_alts, optional, quant, behind, span)) return HUFE_ARGUMENT;
    const FindKey k = {who, "classes, alt_lens", both ? classes : NULL, maxlen, rec, &t.t, &t, sel, cx, anc, term,
                       quant || cross ? &q : NULL, cross ? &x : NULL, span};
    return find_call(ctx, in, out, k, flags, stream);
}

extern "C" int hufgpu_find_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                               uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                               const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, uint64_t *d_pos, uint64_t pos_cap,
                               uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    return find_alt_call(ctx, "find_any", in, out, classes, alt_lens, n_alts, NULL, NULL, NULL, flags, stream);
}

extern "C" int hufgpu_find_records_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                       uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                       const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                       uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                                       uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    return find_alt_call(ctx, "find_records_any", in, out, classes, alt_lens, n_alts, &rec, NULL, NULL, flags, stream);
}

extern "C" int hufgpu_find_records_select(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                          uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                          const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                          uint32_t select, uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint64_t rec_cap,
                                          uint32_t max_len, uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                          uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT)
        return find_bad(ctx, "find_records_select: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    return find_alt_call(ctx, "find_records_select", in, out, classes, alt_lens, n_alts, &rec, &sel, NULL, flags, stream);
}

extern "C" int hufgpu_find_records_context(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                           uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                           const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                           uint32_t select, uint32_t before, uint32_t after, uint64_t *d_rec_pos, uint32_t *d_rec_len,
                                           uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                                           uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT)
        return find_bad(ctx, "find_records_context: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    const FindCtxCall cx = {before, after, d_rec_sel};
    const bool plain = (before | after) == 0u && !d_rec_sel;        /* the select call, by its launches */
    return find_alt_call(ctx, "find_records_context", in, out, classes, alt_lens, n_alts, &rec, &sel, plain ? NULL : &cx, flags, stream);
}

extern "C" int hufgpu_find_any_quant(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                     uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                     const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                                     uint64_t *d_pos, uint64_t pos_cap, uint64_t *d_block_counts, uint64_t *d_totals,
                                     int32_t *d_block_errs, uint32_t flags, void *stream)
{
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    return find_alt_call(ctx, "find_any_quant", in, out, classes, alt_lens, n_alts, NULL, NULL, NULL, flags, stream, NULL, NULL, NULL, optional);
}

extern "C" int hufgpu_find_records_quant(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                         uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                         const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                         const uint8_t *optional, uint32_t select, uint32_t before, uint32_t after, uint64_t *d_rec_pos,
                                         uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                                         uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT)
        return find_bad(ctx, "find_records_quant: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    const FindCtxCall cx = {before, after, d_rec_sel};
    const bool plain = (before | after) == 0u && !d_rec_sel;        /* the select call, by its launches */
    return find_alt_call(ctx, "find_records_quant", in, out, classes, alt_lens, n_alts, &rec, &sel, plain ? NULL : &cx, flags, stream, NULL,
                         NULL, NULL, optional);
}

/* The anchored calls' own checks, behind the `select` check and in front of the older calls': a bit that is no anchor, BOL or
 * EOL without delimiters (the positions call; a records call without them is find_check's to word), WORD without word bytes.
 * Then the two boundary sets: in front of a match BOL asks for a delimiter and WORD for a byte that is no word byte, both
 * for a byte of both kinds; behind it EOL and WORD ask for the same.  A set that no anchor asks for is not used. */
static int find_anc_sets(hufgpu_ctx_t *ctx, const char *who, uint32_t anchors, const uint8_t *delim_set, const uint8_t *word_set, bool rec,
                         FindAncCall *anc)
{
    const uint32_t all = HUFGPU_ANCHOR_BOL | HUFGPU_ANCHOR_EOL | HUFGPU_ANCHOR_WORD;
    if (anchors & ~all)
        return find_bad(ctx, "%s: anchors 0x%x has a bit other than HUFGPU_ANCHOR_BOL, HUFGPU_ANCHOR_EOL and HUFGPU_ANCHOR_WORD", who, anchors);
    if (!rec && (anchors & (HUFGPU_ANCHOR_BOL | HUFGPU_ANCHOR_EOL)) && !delim_set)
        return find_bad(ctx, "%s: HUFGPU_ANCHOR_BOL and HUFGPU_ANCHOR_EOL need the delim_set (anchors 0x%x)", who, anchors);
    if ((anchors & HUFGPU_ANCHOR_WORD) && !word_set)
        return find_bad(ctx, "%s: HUFGPU_ANCHOR_WORD needs the word_set (anchors 0x%x)", who, anchors);
    anc->anchors = anchors;
    for (int i = 0; i < 32; i++) {
        const uint8_t d = delim_set ? delim_set[i] : 0, nw = (anchors & HUFGPU_ANCHOR_WORD) ? (uint8_t)~word_set[i] : 0xff;
        anc->front[i] = (uint8_t)(((anchors & HUFGPU_ANCHOR_BOL) ? d : 0xff) & nw);
        anc->behind[i] = (uint8_t)(((anchors & HUFGPU_ANCHOR_EOL) ? d : 0xff) & nw);
    }
    return HUFE_OK;
}

extern "C" int hufgpu_find_any_anchored(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                        uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                        const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t delim_set[32],
                                        const uint8_t word_set[32], uint32_t anchors, uint64_t *d_pos, uint64_t pos_cap,
                                        uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindAncCall anc;
    if (anchors && find_anc_sets(ctx, "find_any_anchored", anchors, delim_set, word_set, false, &anc)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    return find_alt_call(ctx, "find_any_anchored", in, out, classes, alt_lens, n_alts, NULL, NULL, NULL, flags, stream, anchors ? &anc : NULL);
}

extern "C" int hufgpu_find_records_anchored(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                            uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                            const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                            const uint8_t word_set[32], uint32_t anchors, uint32_t select, uint32_t before, uint32_t after,
                                            uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap,
                                            uint32_t max_len, uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                            uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT)
        return find_bad(ctx, "find_records_anchored: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
    FindAncCall anc;
    if (anchors && find_anc_sets(ctx, "find_records_anchored", anchors, delim_set, word_set, true, &anc)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    const FindCtxCall cx = {before, after, d_rec_sel};
    const bool plain = (before | after) == 0u && !d_rec_sel;        /* the select call, by its launches */
    return find_alt_call(ctx, "find_records_anchored", in, out, classes, alt_lens, n_alts, &rec, &sel, plain ? NULL : &cx, flags, stream,
                         anchors ? &anc : NULL);
}

/* hufgpu_find_records_terms' own checks, behind the `select` check and in front of the older calls': the mode, the array,
 * the number of terms, a term without alternatives, counts that do not sum to n_alts and - ordered - a term whose
 * alternatives differ in length (last_free, the expr call: but for the last term, whose end no kernel needs).  The lengths are looked at only where the older checks would read them too: both arrays
 * there and n_alts within its bounds; whatever else is wrong with them is the older checks' to word. */
static int find_term_check(hufgpu_ctx_t *ctx, const char *who, const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                           const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode, bool last_free = false)
{
    if (terms_mode > HUFGPU_TERMS_ORDERED)
        return find_bad(ctx, "%s: terms_mode %u is neither HUFGPU_TERMS_ALL (0) nor HUFGPU_TERMS_ORDERED (1)", who, terms_mode);
    if (!term_alts) return find_bad(ctx, "%s: term_alts is required (one term: an array of the one count, n_alts)", who);
    if (n_terms == 0 || n_terms > HUFGPU_FIND_TERMS_MAX)
        return find_bad(ctx, "%s: n_terms %u is not 1 to %d", who, n_terms, HUFGPU_FIND_TERMS_MAX);
    uint64_t total = 0;
    for (uint32_t t = 0; t < n_terms; t++) {
        if (term_alts[t] == 0) return find_bad(ctx, "%s: term %u has no alternative: no record would hold it", who, t);
        total += term_alts[t];
    }
    if (total != n_alts)
        return find_bad(ctx, "%s: the %u terms have %llu alternatives, and n_alts is %u", who, n_terms, (unsigned long long)total, n_alts);
    if (terms_mode != HUFGPU_TERMS_ORDERED || !classes || !alt_lens || n_alts > HUFGPU_FIND_PATTERN_MAX) return HUFE_OK;
    for (uint32_t t = 0, j = 0; t + (last_free ? 1u : 0u) < n_terms; j += term_alts[t++]) {
        for (uint32_t i = 1; i < term_alts[t]; i++) {
            if (alt_lens[j + i] != alt_lens[j])
                return find_bad(ctx, "%s: the alternatives of term %u have the lengths %u and %u: an ordered call needs one length a term",
                                who, t, alt_lens[j], alt_lens[j + i]);
        }
    }
    return HUFE_OK;
}

extern "C" int hufgpu_find_records_terms(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                         uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                         const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                         const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode, uint32_t select,
                                         uint32_t before, uint32_t after, uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no,
                                         uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len, uint64_t *d_block_counts,
                                         uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (select & ~HUFGPU_SELECT_INVERT)
        return find_bad(ctx, "find_records_terms: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", select);
    if (find_term_check(ctx, "find_records_terms", classes, alt_lens, n_alts, term_alts, n_terms, terms_mode)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    const FindCtxCall cx = {before, after, d_rec_sel};
    const bool plain = (before | after) == 0u && !d_rec_sel;        /* the select call, by its launches */
    FindTermCall term;
    memset(&term, 0, sizeof(term));
    term.t.n_terms = n_terms;
    term.ordered = terms_mode == HUFGPU_TERMS_ORDERED;
    return find_alt_call(ctx, "find_records_terms", in, out, classes, alt_lens, n_alts, &rec, &sel, plain ? NULL : &cx, flags, stream, NULL,
                         n_terms > 1 ? &term : NULL, term_alts);              /* (one term: the context call, by its launches) */
}

extern "C" int hufgpu_find_any_expr(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                    uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                    const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                                    const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors, uint64_t *d_pos,
                                    uint64_t pos_cap, uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                    uint32_t flags, void *stream)
{
    FindAncCall anc;
    if (anchors && find_anc_sets(ctx, "find_any_expr", anchors, delim_set, word_set, false, &anc)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    return find_alt_call(ctx, "find_any_expr", in, out, classes, alt_lens, n_alts, NULL, NULL, NULL, flags, stream, anchors ? &anc : NULL, NULL,
                         NULL, optional);
}

/* hufgpu_find_any_spans: hufgpu_find_any_expr with d_len and d_open behind d_pos */
extern "C" int hufgpu_find_any_spans(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                     uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                     const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                                     const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors, uint64_t *d_pos,
                                     uint32_t *d_len, uint8_t *d_open, uint64_t pos_cap, uint64_t *d_block_counts, uint64_t *d_totals,
                                     int32_t *d_block_errs, uint32_t flags, void *stream)
{
    FindAncCall anc;
    if (anchors && find_anc_sets(ctx, "find_any_spans", anchors, delim_set, word_set, false, &anc)) return HUFE_ARGUMENT;
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_pos, pos_cap, d_block_counts, d_totals, d_block_errs};
    FindSpanCall span;
    span.d_len = d_len;
    span.d_open = d_open;
    span.fixed = true;
    span.value = 0;
    return find_alt_call(ctx, "find_any_spans", in, out, classes, alt_lens, n_alts, NULL, NULL, NULL, flags, stream, anchors ? &anc : NULL, NULL,
                         NULL, optional, &span);
}

/* hufgpu_find_records_expr: the `select` check, the anchored calls' checks, the terms call's - an ordered call's last term
 * may have alternatives of several lengths -, then anchors with ALL of several terms; find_alt_call has the rest. */
extern "C" int hufgpu_find_records_expr(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                        uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                        const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                        const uint8_t *optional, const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode,
                                        const uint8_t word_set[32], uint32_t anchors, uint32_t select, uint32_t before, uint32_t after,
                                        uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap,
                                        uint32_t max_len, uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                        uint32_t flags, void *stream)
{
    const char *who = "find_records_expr";
    if (select & ~HUFGPU_SELECT_INVERT) return find_bad(ctx, "%s: select 0x%x has a bit other than HUFGPU_SELECT_INVERT", who, select);
    FindAncCall anc;
    if (anchors && find_anc_sets(ctx, who, anchors, delim_set, word_set, true, &anc)) return HUFE_ARGUMENT;
    if (find_term_check(ctx, who, classes, alt_lens, n_alts, term_alts, n_terms, terms_mode, true)) return HUFE_ARGUMENT;
    if (terms_mode == HUFGPU_TERMS_ALL && n_terms > 1 && anchors)
        return find_bad(ctx, "%s: anchors 0x%x with HUFGPU_TERMS_ALL of %u terms: anchors need one term or HUFGPU_TERMS_ORDERED", who, anchors, n_terms);
    const FindStream in = {d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize};
    const FindOut out = {d_rec_pos, rec_cap, d_block_counts, d_totals, d_block_errs};
    const FindRecCall rec = {delim_set, d_rec_len, max_len};
    const FindSelCall sel = {select, d_rec_no};
    const FindCtxCall cx = {before, after, d_rec_sel};
    const bool plain = (before | after) == 0u && !d_rec_sel;        /* the select call, by its launches */
    FindTermCall term;
    memset(&term, 0, sizeof(term));
    term.t.n_terms = n_terms;
    term.ordered = terms_mode == HUFGPU_TERMS_ORDERED;
    return find_alt_call(ctx, who, in, out, classes, alt_lens, n_alts, &rec, &sel, plain ? NULL : &cx, flags, stream, anchors ? &anc : NULL,
                         n_terms > 1 ? &term : NULL, term_alts, optional);
}

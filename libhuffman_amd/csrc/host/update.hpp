/* update.hpp - hufgpu_update_ranges: byte ranges of the original data overwritten in one indexed stream
   (include/huffman_gpu.h, kernels/update.hpp), and the row encoders it shares with hufgpu_append / hufgpu_truncate.
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* Counts + trees, and pack, of a compact list of rows (kernels/update.hpp) by the kernels encode_impl picks for blocks
 * of `longest` bytes: every one is bit-exact, the route only decides speed.  hufgpu_update_ranges and hufgpu_append /
 * hufgpu_truncate share them, so the thresholds stand in one place. */
static void launch_pairs_trees(hufgpu_ctx *ctx, const uint8_t *base, uint64_t rows, uint64_t longest, const TwoLevel &sizes, hipStream_t s)
{
    static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;
    if (longest >= HL_MIN_BLOCK && !fused_only) {
        hist_lanes_pairs_kernel<HL_THREADS><<<dim3((unsigned)rows), dim3(HL_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_hist);
        tree_wave_kernel<<<dim3((unsigned)rows), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    } else if (longest <= HT_PACKED_MAX_BLOCK) {
        hist_tree_pairs_kernel<HIST_THREADS, true><<<dim3((unsigned)rows), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    } else {
        hist_tree_pairs_kernel<HIST_THREADS, false><<<dim3((unsigned)rows), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    }
}

static void launch_pairs_pack(hufgpu_ctx *ctx, const uint8_t *base, uint64_t rows, uint64_t longest, uint64_t *offsets, uint64_t nblocks,
                              uint64_t out_cap, uint8_t *out, const HufSubIndex &sub, hipStream_t s)
{
    if (longest <= 121392ull)            /* deepest possible code <= 24 bits: 32-bit code path only, as in encode_impl */
        pack_pairs_kernel<PACK_THREADS, true><<<dim3((unsigned)rows), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub);
    else
        pack_pairs_kernel<PACK_THREADS, false><<<dim3((unsigned)rows), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub);
}

static bool spans_overlap(const void *a, uint64_t an, const void *b, uint64_t bn)
{
    if (!a || !b || !an || !bn) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

struct UpdRangeOrder {
    uint64_t lo, hi, i;
};
static int upd_range_cmp(const void *a, const void *b)
{
    const UpdRangeOrder *x = (const UpdRangeOrder *)a, *y = (const UpdRangeOrder *)b;
    return x->lo < y->lo ? -1 : (x->lo > y->lo ? 1 : (x->i < y->i ? -1 : 1));
}

extern "C" int hufgpu_update_ranges(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                    const uint64_t *d_block_offsets, uint64_t nblocks, uint64_t nranges,
                                    const uint64_t *range_lo, const uint64_t *range_hi, const uint64_t *src_offsets,
                                    const void *d_src, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                    void *d_out, uint64_t out_cap, uint64_t *d_out_block_offsets, void *d_out_sub_index,
                                    uint32_t flags, uint64_t *out_len, uint64_t *blocks_reencoded, void *stream)
{
    if (out_len) *out_len = 0;
    if (blocks_reencoded) *blocks_reencoded = 0;
    if (nranges > 0x7fffffffull || (nranges && (!range_lo || !range_hi))) {
        set_err(ctx, "update_ranges: range_lo and range_hi are required (at most 2^31 - 1 ranges)");
        return HUFE_ARGUMENT;
    }
    uint64_t nfull = 0, src_extent = 0, src_total = 0;
    for (uint64_t i = 0; i < nranges; i++) {
        if (range_lo[i] > range_hi[i]) {
            set_err(ctx, "update_ranges: range %llu ends in front of its start", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
        const uint64_t len = range_hi[i] - range_lo[i];
        if (len == 0) continue;
        nfull++;
        const uint64_t at = src_offsets ? src_offsets[i] : src_total;
        if (at + len < at) {
            set_err(ctx, "update_ranges: the new bytes of range %llu wrap around the address space", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
        if (at + len > src_extent) src_extent = at + len;
        src_total += len;
    }
    if (nfull > 1) {                                  /* an overwrite has one value per byte: the ranges must not overlap */
        UpdRangeOrder *ord = (UpdRangeOrder *)malloc(nfull * sizeof(UpdRangeOrder));
        if (!ord) return HUFE_MEMORY;
        uint64_t k = 0;
        for (uint64_t i = 0; i < nranges; i++)
            if (range_lo[i] < range_hi[i]) { ord[k].lo = range_lo[i]; ord[k].hi = range_hi[i]; ord[k].i = i; k++; }
        qsort(ord, nfull, sizeof(UpdRangeOrder), upd_range_cmp);
        for (k = 1; k < nfull; k++) {
            if (ord[k - 1].hi > ord[k].lo) {
                set_err(ctx, "update_ranges: ranges %llu and %llu overlap", (unsigned long long)ord[k - 1].i, (unsigned long long)ord[k].i);
                free(ord);
                return HUFE_ARGUMENT;
            }
        }
        free(ord);
    }
    uint64_t sub_bytes = 0;
    if (d_sub_index || d_out_sub_index) {
        if (blocksize == 0) blocksize = raw_size;
        const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
        if ((((uintptr_t)d_sub_index | (uintptr_t)d_out_sub_index) & 7u) || raw_size == 0 ||
            hufgpu_block_count(raw_size, blocksize) != nblocks || nblocks * cpb > 0x7fffffffull) {
            set_err(ctx, "update_ranges: a sub-index needs an 8-byte aligned buffer and the (raw_size, blocksize) that give the layout of these %llu blocks",
                    (unsigned long long)nblocks);
            return HUFE_ARGUMENT;
        }
        if (d_out_sub_index && blocksize >= HUF_CHUNKED_FROM) {
            set_err(ctx, "update_ranges: a new sub-index needs blocks below %llu bytes", (unsigned long long)HUF_CHUNKED_FROM);
            return HUFE_ARGUMENT;
        }
        sub_bytes = hufgpu_sub_index_bytes(raw_size, blocksize);
    }
    if ((uintptr_t)d_out & 3u) {                      /* pack writes whole words of the destination, as in hufgpu_encode */
        set_err(ctx, "update_ranges: the output must be 4-byte aligned");
        return HUFE_ARGUMENT;
    }
    const uint64_t index_bytes = (nblocks + 1) * sizeof(uint64_t);
    if (spans_overlap(d_out, out_cap, d_stream, stream_len) || spans_overlap(d_out, out_cap, d_block_offsets, index_bytes) ||
        spans_overlap(d_out, out_cap, d_src, src_extent) || spans_overlap(d_out, out_cap, d_sub_index, sub_bytes) ||
        spans_overlap(d_out, out_cap, d_out_block_offsets, index_bytes) || spans_overlap(d_out, out_cap, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_block_offsets, index_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_src, src_extent) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_sub_index, sub_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_block_offsets, index_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_src, src_extent)) {
        set_err(ctx, "update_ranges: the output buffers overlap the input (the call works out of place) or one another");
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "update_ranges: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    const uint64_t nb = nblocks;
    if (nb > 0x7fffffffull || (nb && stream_len && (!d_stream || !d_block_offsets)) || (stream_len && !d_out) || (src_total && !d_src)) {
        set_err(ctx, "update_ranges: the stream, its block index, the new bytes or the output is missing, or more than 2^31 - 1 blocks");
        return HUFE_ARGUMENT;
    }
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    ctx->last_stream = s;
    const uint8_t *st = (const uint8_t *)d_stream;

    if (nfull == 0) {                                 /* nothing to write: the stream, its index and its sub-index as they are */
        if (stream_len > out_cap) {
            set_err(ctx, "update_ranges: the stream of %llu bytes does not fit the output of %llu", (unsigned long long)stream_len, (unsigned long long)out_cap);
            return HUFE_MEMORY;
        }
        if (stream_len) HIP_OK(ctx, hipMemcpyAsync(d_out, d_stream, stream_len, hipMemcpyDeviceToDevice, s));
        if (d_out_block_offsets && d_block_offsets) HIP_OK(ctx, hipMemcpyAsync(d_out_block_offsets, d_block_offsets, index_bytes, hipMemcpyDeviceToDevice, s));
        if (d_out_sub_index && d_sub_index && nblocks && stream_len && d_block_offsets) {
            /* the rows as the general path copies them - the entries the encoder writes, nothing else: every block is a copy block */
            int rc0 = ensure_decode_ws(ctx, nblocks);
            if (!rc0) rc0 = ensure_batch_ws(ctx, nblocks, 1);
            if (rc0) return rc0;
            const TwoLevel lens0 = decode_lens(ctx, nblocks);
            launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nblocks, max_tree_of(flags), lens0, s);
            upd_positions_kernel<<<dim3(grid256(nblocks + 1)), dim3(256), 0, s>>>(lens0, nblocks, ctx->d_bprefix, ctx->d_blk_item);
            const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize), to = sub_index_view(d_out_sub_index, raw_size, blocksize);
            upd_sub_rows_kernel<<<dim3((unsigned)nblocks), dim3(256), 0, s>>>(from, to, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
            HIP_OK(ctx, hipGetLastError());
        }
        HIP_OK(ctx, hipStreamSynchronize(s));
        if (out_len) *out_len = stream_len;
        return HUFE_OK;
    }
    if (nb == 0 || stream_len == 0) {
        set_err(ctx, "update_ranges: the stream holds no data, every range lies behind its end");
        return HUFE_ARGUMENT;
    }

    int rc = ensure_decode_ws(ctx, nb);
    if (rc) return rc;
    rc = ensure_batch_ws(ctx, nb, nranges);
    if (rc) return rc;
    rc = ensure_range_ws(ctx, nb, nranges);
    if (rc) return rc;
    rc = ensure_update_ws(ctx, nb, 0);
    if (rc) return rc;
    uint64_t *h = NULL;
    rc = batch_stage(ctx, 4 * nranges + 1, &h);
    if (rc) return rc;
    memcpy(h, range_lo, nranges * sizeof(uint64_t));
    memcpy(h + nranges, range_hi, nranges * sizeof(uint64_t));
    {
        uint64_t acc = 0;
        for (uint64_t i = 0; i < nranges; i++) {
            h[2 * nranges + i] = acc;                 /* the plan's slot check: every range has room for itself */
            h[3 * nranges + 1 + i] = src_offsets ? src_offsets[i] : acc;
            acc += range_hi[i] - range_lo[i];
        }
        h[3 * nranges] = acc;
    }
    rc = batch_upload(ctx, 4 * nranges + 1, s);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_ucount, 0, UPD_WORDS * sizeof(unsigned long long), s));

    const TwoLevel lens = decode_lens(ctx, nb);
    launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nb, max_tree_of(flags), lens, s);

    uint64_t *offs_new = d_out_block_offsets ? d_out_block_offsets : ctx->d_unew;
    UpdateArgs ua;
    memset(&ua, 0, sizeof(ua));
    DecRangeArgs &ra = ua.r;
    const unsigned mark_y = fill_range_args(ctx, ra, nranges, nb, lens);
    ua.src_offsets = ctx->d_bstage + 3 * nranges + 1;
    ua.old_offsets = d_block_offsets;
    ua.new_offsets = offs_new;
    ua.stream_len = stream_len;
    ua.row_of = ctx->d_urow_of;
    ua.row_blk = ctx->d_urow_blk;
    ua.pairs = ctx->d_upairs;
    ua.ucount = ctx->d_ucount;
    const unsigned plan_grid = grid256((nb + 1 > nranges ? nb + 1 : nranges));
    drange_plan_kernel<<<dim3(plan_grid), dim3(256), 0, s>>>(ra);
    drange_mark_kernel<<<dim3((unsigned)nranges, mark_y), dim3(256), 0, s>>>(ra);
    upd_class_kernel<<<dim3(plan_grid), dim3(256), 0, s>>>(ua);
    HIP_OK(ctx, hipGetLastError());
    /* the one wait in front of the work: how many blocks are touched and staged and how long they are decides the rows,
     * the scratch area and the kernels; a range that cannot be served ends the call here */
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_rcounters, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 10, ctx->d_ucount, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const uint64_t nstaged = ctx->h_result[8], longest_staged = ctx->h_result[9];
    const uint64_t ntouched = ctx->h_result[10], longest = ctx->h_result[11];
    if (ctx->h_result[12]) {
        const uint64_t key = ~ctx->h_result[12];
        const int err = (int)(key & 0xffu);
        set_err(ctx, err == HUFE_ARGUMENT ? "update_ranges: range %llu reaches past the end of the data"
                                          : "update_ranges: range %llu reaches a block whose header does not parse", (unsigned long long)(key >> 8));
        return err;
    }
    if (d_out_sub_index && longest > blocksize) {
        set_err(ctx, "update_ranges: a touched block of %llu bytes is longer than the sub-index rows of %llu", (unsigned long long)longest,
                (unsigned long long)blocksize);
        return HUFE_ARGUMENT;
    }
    const bool big = longest >= HUF_CHUNKED_FROM;      /* blocks of 2 MiB and more: one at a time through the chunked path */
    const uint64_t stride = (longest_staged + 15u) & ~15ull;
    const uint64_t enc_cap = big ? ((hufgpu_encode_bound(longest, longest) + 15u) & ~15ull) : 0;
    uint64_t staged_bytes = 0, scratch_bytes = 0;
    if (__builtin_mul_overflow(nstaged, stride, &staged_bytes) || __builtin_add_overflow(staged_bytes, enc_cap, &scratch_bytes)) scratch_bytes = ~0ull;
    if (scratch_bytes) {
        rc = grow_range_scratch(ctx, scratch_bytes);
        if (rc == HUFE_MEMORY) set_err(ctx, "update_ranges: no room for %llu staged blocks of up to %llu bytes", (unsigned long long)nstaged, (unsigned long long)longest_staged);
        if (rc) return rc;
    }
    rc = ensure_encode_ws(ctx, ntouched ? ntouched : 1);
    if (rc) return rc;
    ua.meta = ctx->d_meta;

    /* the rows' sources: one base, the lower of the new bytes and the scratch area, and 64-bit offsets */
    uint8_t *scr = ctx->d_rscratch;
    const uint8_t *base = (const uint8_t *)d_src;
    if (nstaged && (!base || (uintptr_t)scr < (uintptr_t)base)) base = scr;
    ua.src_off = d_src ? (uint64_t)((uintptr_t)d_src - (uintptr_t)base) : 0;
    ua.scratch_off = nstaged ? (uint64_t)((uintptr_t)scr - (uintptr_t)base) : 0;
    ua.src = (const uint8_t *)d_src;
    ua.scratch_w = scr;
    ra.stride = stride;
    ra.scratch = scr;
    upd_place_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ua);
    if (nstaged) {
        /* the staged blocks through the indexed decoders as they are, into their scratch entries: zeros + the placed offsets */
        TwoLevel blens = lens;
        blens.gprefix = ctx->d_bzero;
        blens.local = ctx->d_bobase;
        const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
        const IndexedDecode job = {st, stream_len, d_block_offsets, nb, blens, scr, staged_bytes, &sub, blocksize};
        rc = launch_indexed_decoders(ctx, job, s);
        if (rc) return rc;
        const unsigned overlay_y = nranges >= 1024 ? 2u : (nranges >= 64 ? 4u : 16u);
        upd_overlay_kernel<<<dim3((unsigned)nranges, overlay_y), dim3(256), 0, s>>>(ua);
        upd_fail_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ua);
    }
    HIP_OK(ctx, hipGetLastError());

    UpdCopyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.stream = st;
    ca.out = (uint8_t *)d_out;
    ca.old_offsets = d_block_offsets;
    ca.new_offsets = offs_new;
    ca.kind = ctx->d_blk_item;
    ca.nblocks = nb;
    ca.out_cap = out_cap;
    ca.align = (uint64_t)((uintptr_t)d_out & 15u);
    /* pieces for all of the output: the new length is known on the device only, and a piece behind it returns at once */
    ca.npieces = (out_cap + ca.align) / UPD_PIECE + 1;
    rc = ensure_update_ws(ctx, nb, ca.npieces);
    if (rc) return rc;
    ca.piece_first = ctx->d_upiece;

    int err = HUFE_OK;
    if (!big) {
        if (ntouched) {
            TwoLevel sizes = ctx->enc_sizes;
            sizes.total = (uint64_t *)ctx->d_ucount + 5;         /* (the rows' sum: not used, the index is summed over all blocks below) */
            launch_pairs_trees(ctx, base, ntouched, longest, sizes, s);
        }
        upd_index_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ua);
        if (ntouched) {
            const HufSubIndex sub = sub_index_view(d_out_sub_index, raw_size, blocksize);
            launch_pairs_pack(ctx, base, ntouched, longest, offs_new, nb, out_cap, (uint8_t *)d_out, sub, s);
        }
        upd_piece_kernel<<<dim3(grid256(ca.npieces)), dim3(256), 0, s>>>(ca);
        update_copy_kernel<<<dim3((unsigned)ca.npieces), dim3(256), 0, s>>>(ca);
        if (d_sub_index && d_out_sub_index) {
            const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize), to = sub_index_view(d_out_sub_index, raw_size, blocksize);
            upd_sub_rows_kernel<<<dim3((unsigned)nb), dim3(256), 0, s>>>(from, to, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
        }
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_ucount, UPD_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
    } else {
        /* every block's place is worked out here, a touched block is encoded by encode_impl as a stream of one block into
         * the end of the scratch area and copied to its place; the untouched records then move as above */
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_ucount, UPD_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        uint8_t *enc = scr + staged_bytes;
        uint32_t *h_kind = (uint32_t *)malloc(nb * sizeof(uint32_t)), *h_row = (uint32_t *)malloc(nb * sizeof(uint32_t));
        uint64_t *h_pairs = (uint64_t *)malloc(2 * ntouched * sizeof(uint64_t)), *h_old = (uint64_t *)malloc(index_bytes), *h_new = (uint64_t *)malloc(index_bytes);
        hipError_t he = hipSuccess;
        if (!h_kind || !h_row || !h_pairs || !h_old || !h_new) err = HUFE_MEMORY;
        if (!err && !ctx->h_result[8 + UPD_FAILED]) {
            if (he == hipSuccess) he = hipMemcpyAsync(h_kind, ctx->d_blk_item, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_row, ctx->d_urow_of, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_pairs, ctx->d_upairs, 2 * ntouched * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_old, d_block_offsets, index_bytes, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);
            uint64_t pos = 0;
            for (uint64_t b = 0; b < nb && he == hipSuccess && !err; b++) {
                h_new[b] = pos;
                if (h_kind[b] == UPD_COPY) {
                    pos += h_old[b + 1] - h_old[b];
                } else if (h_kind[b] != UPD_VOID) {
                    const uint64_t *pr = h_pairs + 2 * (uint64_t)h_row[b];
                    uint64_t got = 0;
                    err = encode_impl(ctx, base + pr[0], pr[1], 0, enc, enc_cap, NULL, NULL, &got, s);
                    if (!err && (got > out_cap || pos > out_cap - got)) err = HUFE_MEMORY;
                    if (!err) he = hipMemcpyAsync((uint8_t *)d_out + pos, enc, got, hipMemcpyDeviceToDevice, s);
                    pos += got;
                }
                if (!err && pos > out_cap) err = HUFE_MEMORY;
            }
            h_new[nb] = pos;
            ctx->h_result[8 + UPD_TOTAL] = err ? ~0ull : pos;
            if (!err && he == hipSuccess) he = hipMemcpyAsync(offs_new, h_new, index_bytes, hipMemcpyHostToDevice, s);
            if (!err && he == hipSuccess) {
                upd_piece_kernel<<<dim3(grid256(ca.npieces)), dim3(256), 0, s>>>(ca);
                update_copy_kernel<<<dim3((unsigned)ca.npieces), dim3(256), 0, s>>>(ca);
                he = hipGetLastError();
            }
            if (he == hipSuccess) he = hipStreamSynchronize(s);
        }
        free(h_kind); free(h_row); free(h_pairs); free(h_old); free(h_new);
        HIP_OK(ctx, he);
        if (err == HUFE_MEMORY) set_err(ctx, "update_ranges: the new stream does not fit the output of %llu bytes", (unsigned long long)out_cap);
        if (err) return err;
    }
    if (ctx->h_result[8 + UPD_FAILED]) {
        /* a staged block that does not decode: what hufgpu_decode() says of it, the first in stream order */
        const uint64_t f = ~ctx->h_result[8 + UPD_FAILED];
        int32_t serr = HUFE_FATAL;
        HIP_OK(ctx, hipMemcpyAsync(&serr, ctx->d_status + f, sizeof(serr), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        set_err(ctx, "update_ranges: block %llu, which a range cuts, does not decode (error %d)", (unsigned long long)f, (int)serr);
        return serr ? serr : HUFE_FATAL;
    }
    const uint64_t total = ctx->h_result[8 + UPD_TOTAL];
    if (total > out_cap) {
        set_err(ctx, "update_ranges: the new stream of %llu bytes does not fit the output of %llu", (unsigned long long)total, (unsigned long long)out_cap);
        return HUFE_MEMORY;
    }
    if (out_len) *out_len = total;
    if (blocks_reencoded) *blocks_reencoded = ntouched;
    return HUFE_OK;
}

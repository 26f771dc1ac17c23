/* scatter.hpp - hufgpu_scatter: records at device-resident positions overwritten in one indexed stream (include/huffman_gpu.h,
   kernels/scatter.hpp), enqueue-only - hufgpu_update_ranges' pipeline (host/update.hpp) with host-known bounds in the
   place of its plan.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* (record, block) parts a record of up to max_len bytes can have in blocks of `blocksize` (never 0); a record of no
 * bytes has none, and counts as one so that the bound stays a count of records */
static uint64_t scatter_parts_per_record(uint64_t nblocks, uint64_t blocksize, uint32_t max_len)
{
    if (max_len == 0) return 1;
    const uint64_t per_record = ((uint64_t)max_len + blocksize - 2) / blocksize + 1;
    return per_record > nblocks ? nblocks : per_record;
}

extern "C" uint64_t hufgpu_scatter_touched_bound(uint64_t nblocks, uint64_t blocksize, uint64_t nrecords, uint32_t max_len)
{
    if (nblocks == 0 || nrecords == 0) return 0;
    if (blocksize == 0) return 1;                      /* one block */
    const uint64_t per_record = max_len ? scatter_parts_per_record(nblocks, blocksize, max_len) : 1;
    uint64_t all = 0;
    if (__builtin_mul_overflow(nrecords, per_record, &all) || all > nblocks) all = nblocks;
    return all;
}

/* the counts + trees and the pack of launch_pairs_trees / launch_pairs_pack (host/update.hpp) in grids `cap` wide, guarded
 * by the device's row count: the same thresholds, the same bodies */
static void launch_scatter_trees(hufgpu_ctx *ctx, const uint8_t *base, uint64_t cap, uint64_t longest, const TwoLevel &sizes,
                                 const unsigned long long *rows, hipStream_t s)
{
    static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;
    if (longest >= HL_MIN_BLOCK && !fused_only) {
        scat_hist_lanes_kernel<HL_THREADS><<<dim3((unsigned)cap), dim3(HL_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_hist, rows);
        scat_tree_wave_kernel<<<dim3((unsigned)cap), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes, rows);
    } else if (longest <= HT_PACKED_MAX_BLOCK) {
        scat_hist_tree_kernel<HIST_THREADS, true><<<dim3((unsigned)cap), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes, rows);
    } else {
        scat_hist_tree_kernel<HIST_THREADS, false><<<dim3((unsigned)cap), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes, rows);
    }
}

static void launch_scatter_pack(hufgpu_ctx *ctx, const uint8_t *base, uint64_t cap, uint64_t longest, uint64_t *offsets, uint64_t nblocks,
                                uint64_t out_cap, uint8_t *out, const HufSubIndex &sub, const unsigned long long *rows, hipStream_t s)
{
    if (longest <= 121392ull)            /* deepest possible code <= 24 bits: 32-bit code path only, as in encode_impl */
        scat_pack_rows_kernel<PACK_THREADS, true><<<dim3((unsigned)cap), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub, rows);
    else
        scat_pack_rows_kernel<PACK_THREADS, false><<<dim3((unsigned)cap), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub, rows);
}

extern "C" int hufgpu_scatter(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                              const uint64_t *d_block_offsets, uint64_t nblocks,
                              const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                              uint64_t nrecords, const uint64_t *d_pos, const uint32_t *d_len, uint32_t max_len,
                              const void *d_src, uint64_t src_stride, uint8_t fill,
                              uint64_t touched_cap,
                              void *d_out, uint64_t out_cap, uint64_t *d_out_block_offsets, void *d_out_sub_index,
                              uint64_t *d_result, uint32_t flags, void *stream)
{
    const bool fill_on = (flags & HUFGPU_SCATTER_FILL) != 0;
    /* ---- the argument errors, in the order of the header; nothing is enqueued and the context is not looked at ---- */
    if (!d_stream || !d_block_offsets || !d_pos || !d_out || !d_out_block_offsets || !d_result) {
        set_err(ctx, "scatter: the stream, its block index, d_pos, d_out, d_out_block_offsets and d_result are required");
        return HUFE_ARGUMENT;
    }
    if (!fill_on && !d_src) {
        set_err(ctx, "scatter: d_src is required without HUFGPU_SCATTER_FILL");
        return HUFE_ARGUMENT;
    }
    if (!fill_on && src_stride < max_len) {
        set_err(ctx, "scatter: src_stride %llu is less than max_len %u", (unsigned long long)src_stride, max_len);
        return HUFE_ARGUMENT;
    }
    if (blocksize == 0) blocksize = raw_size;
    if (raw_size == 0 || blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, blocksize) != nblocks || nblocks > 0x7fffffffull) {
        set_err(ctx, "scatter: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks", (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    if (blocksize >= HUF_CHUNKED_FROM) {
        set_err(ctx, "scatter: needs blocks below %llu bytes (the chunked encoder waits once per block)", (unsigned long long)HUF_CHUNKED_FROM);
        return HUFE_ARGUMENT;
    }
    if (touched_cap == 0 || touched_cap > nblocks) {
        set_err(ctx, "scatter: touched_cap %llu must be between 1 and the %llu blocks", (unsigned long long)touched_cap, (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    const uint64_t per_record = scatter_parts_per_record(nblocks, blocksize, max_len);
    /* (records of no bytes have no parts: max_len = 0 is the plain copy below, however many records it names) */
    const uint64_t nparts = max_len == 0 ? 0 : (nrecords > 0x7fffffffull ? ~0ull : nrecords * per_record);
    if (nparts > 0xffffffffull) {
        set_err(ctx, "scatter: %llu records of up to %u bytes are more than 2^32 - 1 (record, block) parts", (unsigned long long)nrecords, max_len);
        return HUFE_ARGUMENT;
    }
    if ((uintptr_t)d_out & 3u) {                      /* pack writes whole words of the destination, as in hufgpu_encode */
        set_err(ctx, "scatter: the output must be 4-byte aligned");
        return HUFE_ARGUMENT;
    }
    if (((uintptr_t)d_sub_index | (uintptr_t)d_out_sub_index) & 7u) {
        set_err(ctx, "scatter: a sub-index needs an 8-byte aligned buffer");
        return HUFE_ARGUMENT;
    }
    const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
    if ((d_sub_index || d_out_sub_index) && nblocks * cpb > 0x7fffffffull) {
        set_err(ctx, "scatter: a sub-index of %llu blocks of %llu bytes has more rows of chunks than the decoders' grid holds",
                (unsigned long long)nblocks, (unsigned long long)blocksize);
        return HUFE_ARGUMENT;
    }
    const uint64_t sub_bytes = (d_sub_index || d_out_sub_index) ? hufgpu_sub_index_bytes(raw_size, blocksize) : 0;
    const uint64_t index_bytes = (nblocks + 1) * sizeof(uint64_t), res_bytes = 4 * sizeof(uint64_t);
    uint64_t src_extent = 0;
    if (!fill_on && __builtin_mul_overflow(nrecords, src_stride, &src_extent)) src_extent = ~0ull - (uintptr_t)d_src;
    if (spans_overlap(d_out, out_cap, d_stream, stream_len) || spans_overlap(d_out, out_cap, d_block_offsets, index_bytes) ||
        spans_overlap(d_out, out_cap, d_src, src_extent) || spans_overlap(d_out, out_cap, d_sub_index, sub_bytes) ||
        spans_overlap(d_out, out_cap, d_out_block_offsets, index_bytes) || spans_overlap(d_out, out_cap, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_block_offsets, index_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_src, src_extent) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_sub_index, sub_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_block_offsets, index_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_src, src_extent) ||
        spans_overlap(d_result, res_bytes, d_out, out_cap) || spans_overlap(d_result, res_bytes, d_out_block_offsets, index_bytes) ||
        spans_overlap(d_result, res_bytes, d_out_sub_index, sub_bytes)) {
        set_err(ctx, "scatter: the output buffers overlap the input (the call works out of place) or one another");
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "scatter: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    ctx->last_stream = s;
    const uint8_t *st = (const uint8_t *)d_stream;
    const uint64_t nb = nblocks;

    int rc = ensure_decode_ws(ctx, nb);
    if (!rc) rc = ensure_batch_ws(ctx, nb, 1);
    if (rc) return rc;
    const TwoLevel lens = decode_lens(ctx, nb);

    if (nrecords == 0 || max_len == 0) {              /* no records: the stream, its index and its sub-index as they are */
        if (stream_len > out_cap) {
            scat_copy_result_kernel<<<dim3(1), dim3(64), 0, s>>>(d_result, (uint64_t)HUFE_MEMORY, 0);
            HIP_OK(ctx, hipGetLastError());
            return HUFE_OK;
        }
        if (stream_len) HIP_OK(ctx, hipMemcpyAsync(d_out, d_stream, stream_len, hipMemcpyDeviceToDevice, s));
        HIP_OK(ctx, hipMemcpyAsync(d_out_block_offsets, d_block_offsets, index_bytes, hipMemcpyDeviceToDevice, s));
        if (d_out_sub_index && d_sub_index && stream_len) {
            launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nb, max_tree_of(flags), lens, s);
            upd_positions_kernel<<<dim3(grid256(nb + 1)), dim3(256), 0, s>>>(lens, nb, ctx->d_bprefix, ctx->d_blk_item);
            const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize), to = sub_index_view(d_out_sub_index, raw_size, blocksize);
            upd_sub_rows_kernel<<<dim3((unsigned)nb), dim3(256), 0, s>>>(from, to, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
        }
        scat_copy_result_kernel<<<dim3(1), dim3(64), 0, s>>>(d_result, (uint64_t)HUFE_OK, stream_len);
        HIP_OK(ctx, hipGetLastError());
        return HUFE_OK;
    }

    /* ---- everything that sizes a buffer or a grid is known here: the layout, the cap, the bound of the parts ---- */
    const uint64_t longest = blocksize < raw_size ? blocksize : raw_size;
    const uint64_t stride = (longest + 15u) & ~15ull;
    UpdCopyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.align = (uint64_t)((uintptr_t)d_out & 15u);
    ca.npieces = (out_cap + ca.align) / UPD_PIECE + 1;      /* pieces for all of the output: a piece behind the new length returns at once */
    rc = ensure_gather_ws(ctx, nb, nparts);
    if (!rc) rc = ensure_update_ws(ctx, nb, ca.npieces);
    if (!rc) rc = ensure_encode_ws(ctx, touched_cap);
    if (rc) return rc;
    rc = grow_range_scratch(ctx, touched_cap * stride);
    if (rc == HUFE_MEMORY) set_err(ctx, "scatter: no room for %llu staged blocks of %llu bytes", (unsigned long long)touched_cap, (unsigned long long)longest);
    if (rc) return rc;
    uint8_t *scr = ctx->d_rscratch;

    ScatterArgs sa;
    memset(&sa, 0, sizeof(sa));
    GatherArgs &ga = sa.g;
    ga.s = sub_stream_args(d_stream, stream_len, d_block_offsets, nb, d_sub_index, raw_size, blocksize, flags);
    ga.max_len = max_len;
    ga.nrecords = nrecords;
    ga.pos = d_pos;
    ga.len = d_len;
    ga.stride = fill_on ? 0 : src_stride;             /* a part's dst: where its new bytes start, from d_src */
    ga.cnt = ctx->d_gcnt;
    ga.cur = ctx->d_gcnt + nb;
    ga.scan = ctx->gat_scan;
    ga.scan.total = ctx->d_gtotal;
    ga.list = ctx->d_glist;
    ga.parts = (GatherPart *)ctx->d_gparts;
    sa.dmeta = ctx->d_dmeta;
    sa.status = ctx->d_status;
    sa.lens = lens;
    sa.old_offsets = d_block_offsets;
    sa.stream_len = stream_len;
    sa.bprefix = ctx->d_bprefix;
    sa.obase = ctx->d_bobase;
    sa.kind = ctx->d_blk_item;
    sa.row_of = ctx->d_urow_of;
    sa.row_blk = ctx->d_urow_blk;
    sa.pairs = ctx->d_upairs;
    sa.ucount = ctx->d_ucount;
    sa.scount = ctx->d_scount;
    sa.touched_cap = touched_cap;
    sa.stride = stride;
    sa.scratch = scr;
    sa.src = (const uint8_t *)d_src;
    sa.fill_on = fill_on ? 1u : 0u;
    sa.fill = fill;
    sa.out_cap = out_cap;
    sa.result = d_result;
    /* the overlay's deal: 16-byte lines a part can have bytes in, the threads that share a part, the groups a part needs */
    const uint64_t part_max = (uint64_t)max_len < longest ? (uint64_t)max_len : longest;
    const uint64_t lines = (part_max + 15u) / 16u + 1u;
    while (sa.group_log2 < 8u && (1ull << sa.group_log2) < lines) sa.group_log2++;
    sa.smax = (uint32_t)((lines + (1ull << sa.group_log2) - 1) >> sa.group_log2);
    const uint64_t per_step = 256u >> sa.group_log2;
    /* the overlay's grid, as hufgpu_gather sizes its serving grid: no wider than the touched blocks can be, a few
     * workgroups a compute unit; where the stream has fewer blocks than that a block's parts go to several workgroups */
    const uint64_t width = 4ull * (uint64_t)ctx->cus;
    uint64_t shares = 1;
    if (nb < width) {
        shares = (nparts * sa.smax + per_step - 1) / per_step;
        if (shares > width / nb) shares = width / nb;
        if (shares < 1) shares = 1;
    }
    uint64_t blocks_max = nb < nparts ? nb : nparts;
    if (blocks_max > touched_cap) blocks_max = touched_cap;
    uint64_t overlay_grid = blocks_max * shares;
    if (overlay_grid > width) overlay_grid = width;
    sa.shares = (uint32_t)shares;

    scat_zero_kernel<<<dim3(grid256(2 * nb + UPD_WORDS)), dim3(256), 0, s>>>(sa);
    scat_mark_kernel<<<dim3(grid256(nrecords)), dim3(256), 0, s>>>(sa);
    launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nb, max_tree_of(flags), lens, s);
    gather_scan_kernel<<<dim3((unsigned)((nb + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(ga);
    gather_place_kernel<<<dim3(grid256(nb > nrecords ? nb : nrecords)), dim3(256), 0, s>>>(ga);
    scat_class_kernel<<<dim3(grid256(nb + 1)), dim3(256), 0, s>>>(sa);
    HIP_OK(ctx, hipGetLastError());
    {
        /* the staged blocks through the indexed decoders as they are, into their scratch entries: zeros + the placed offsets */
        TwoLevel blens = lens;
        blens.gprefix = ctx->d_bzero;
        blens.local = ctx->d_bobase;
        const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
        const IndexedDecode job = {st, stream_len, d_block_offsets, nb, blens, scr, touched_cap * stride, &sub, blocksize};
        rc = launch_indexed_decoders(ctx, job, s);
        if (rc) return rc;
    }
    scat_overlay_kernel<<<dim3((unsigned)overlay_grid), dim3(256), 0, s>>>(sa);
    scat_fail_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(sa);
    HIP_OK(ctx, hipGetLastError());

    UpdateArgs ua;                                    /* what upd_index_kernel reads */
    memset(&ua, 0, sizeof(ua));
    ua.r.nblocks = nb;
    ua.r.kind = ctx->d_blk_item;
    ua.old_offsets = d_block_offsets;
    ua.new_offsets = d_out_block_offsets;
    ua.stream_len = stream_len;
    ua.row_of = ctx->d_urow_of;
    ua.meta = ctx->d_meta;
    ua.ucount = ctx->d_ucount;
    ca.stream = st;
    ca.out = (uint8_t *)d_out;
    ca.old_offsets = d_block_offsets;
    ca.new_offsets = d_out_block_offsets;
    ca.kind = ctx->d_blk_item;
    ca.nblocks = nb;
    ca.out_cap = out_cap;
    ca.piece_first = ctx->d_upiece;

    const unsigned long long *rows = ctx->d_ucount + UPD_N_TOUCHED;
    TwoLevel sizes = ctx->enc_sizes;
    sizes.total = (uint64_t *)ctx->d_ucount + 5;      /* (the rows' sum: not used, the index is summed over all blocks below) */
    launch_scatter_trees(ctx, scr, touched_cap, longest, sizes, rows, s);
    upd_index_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ua);
    const HufSubIndex out_sub = sub_index_view(d_out_sub_index, raw_size, blocksize);
    launch_scatter_pack(ctx, scr, touched_cap, longest, d_out_block_offsets, nb, out_cap, (uint8_t *)d_out, out_sub, rows, s);
    upd_piece_kernel<<<dim3(grid256(ca.npieces)), dim3(256), 0, s>>>(ca);
    update_copy_kernel<<<dim3((unsigned)ca.npieces), dim3(256), 0, s>>>(ca);
    if (d_sub_index && d_out_sub_index) {
        const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize);
        upd_sub_rows_kernel<<<dim3((unsigned)nb), dim3(256), 0, s>>>(from, out_sub, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
    }
    scat_result_kernel<<<dim3(1), dim3(64), 0, s>>>(sa);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

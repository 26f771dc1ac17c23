/* gather.hpp - hufgpu_gather: records at device-resident positions (include/huffman_gpu.h, kernels/gather.hpp),
   enqueue-only.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

extern "C" int hufgpu_gather(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                             uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                             uint64_t nrecords, const uint64_t *d_pos, const uint32_t *d_len, uint32_t max_len, void *d_out,
                             uint64_t out_stride, int32_t *d_errs, uint32_t *d_raw_lens, uint32_t flags, void *stream)
{
    if (nrecords == 0 || max_len == 0) return HUFE_OK;
    if (!d_stream || !d_block_offsets || !d_pos || !d_out || !d_errs) {
        set_err(ctx, "gather: the stream, its block index, d_pos, d_out and d_errs are required");
        return HUFE_ARGUMENT;
    }
    if (out_stride < max_len) {
        set_err(ctx, "gather: out_stride %llu is less than max_len %u", (unsigned long long)out_stride, max_len);
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "gather: needs the stream's sub-index in an 8-byte aligned buffer");
        return HUFE_ARGUMENT;
    }
    if (blocksize == 0) blocksize = raw_size;
    if (raw_size == 0 || blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, blocksize) != nblocks || nblocks > 0x7fffffffull) {
        set_err(ctx, "gather: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks", (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    /* what the host knows of the records: how many, and how long at most - the parts a record can have, the tiles a part */
    uint64_t per_record = ((uint64_t)max_len + blocksize - 2) / blocksize + 1;
    if (per_record > nblocks) per_record = nblocks;
    const uint64_t nparts = nrecords > 0x7fffffffull ? ~0ull : nrecords * per_record;
    if (nparts > 0xffffffffull) {
        set_err(ctx, "gather: %llu records of up to %u bytes are more than 2^32 - 1 (record, block) parts", (unsigned long long)nrecords, max_len);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "gather: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int rc = ensure_gather_ws(ctx, nblocks, nparts);
    if (rc) return rc;

    const uint64_t tiles_per_block = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    uint64_t tmax = ((uint64_t)max_len + HUF_SUB_TILE - 2) / HUF_SUB_TILE + 1;
    if (tmax > tiles_per_block) tmax = tiles_per_block;
    /* The serving grid: no wider than the touched blocks can be, and a few workgroups a compute unit (three fit its LDS).
     * Where the stream has fewer blocks than that, a block's items are dealt to several workgroups - one item a wave,
     * as far as the grid goes: with blocksize = 0 every record lies in the one block. */
    const uint64_t width = 4ull * (uint64_t)ctx->cus;
    uint64_t shares = 1;
    if (nblocks < width) {
        shares = (nparts * tmax + GATHER_WAVES - 1) / GATHER_WAVES;
        if (shares > width / nblocks) shares = width / nblocks;
        if (shares < 1) shares = 1;
    }
    uint64_t grid = (nblocks < nparts ? nblocks : nparts) * shares;
    if (grid > width) grid = width;

    GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.s = sub_stream_args(d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize, flags);
    ga.max_len = max_len;
    ga.nrecords = nrecords;
    ga.pos = d_pos;
    ga.len = d_len;
    ga.out = (uint8_t *)d_out;
    ga.stride = out_stride;
    ga.errs = d_errs;
    ga.raw_lens = d_raw_lens;
    ga.cnt = ctx->d_gcnt;
    ga.cur = ctx->d_gcnt + nblocks;
    ga.scan = ctx->gat_scan;
    ga.scan.total = ctx->d_gtotal;
    ga.list = ctx->d_glist;
    ga.parts = (GatherPart *)ctx->d_gparts;
    ga.shares = (uint32_t)shares;
    ga.tmax = (uint32_t)tmax;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_gcnt, 0, 2 * nblocks * sizeof(uint32_t), s));
    gather_mark_kernel<<<dim3(grid256(nrecords)), dim3(256), 0, s>>>(ga);
    gather_scan_kernel<<<dim3((unsigned)((nblocks + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(ga);
    gather_place_kernel<<<dim3(grid256(nblocks > nrecords ? nblocks : nrecords)), dim3(256), 0, s>>>(ga);
    gather_serve_kernel<<<dim3((unsigned)grid), dim3(GATHER_THREADS), 0, s>>>(ga);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

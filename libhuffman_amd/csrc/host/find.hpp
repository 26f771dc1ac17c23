/* find.hpp - hufgpu_find_bytes: where the bytes of a set of byte values lie in the original data
   (include/huffman_gpu.h, kernels/find.hpp), enqueue-only.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

extern "C" int hufgpu_find_bytes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                 uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                 const uint8_t set[32], uint64_t *d_pos, uint64_t pos_cap, uint64_t *d_block_counts,
                                 uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (!set || !d_totals) {
        set_err(ctx, "find_bytes: the set and d_totals are required");
        return HUFE_ARGUMENT;
    }
    if (pos_cap > 0 && !d_pos) {
        set_err(ctx, "find_bytes: pos_cap %llu needs d_pos", (unsigned long long)pos_cap);
        return HUFE_ARGUMENT;
    }
    if (nblocks == 0) {
        if (raw_size != 0) {
            set_err(ctx, "find_bytes: (raw_size, blocksize) must be those of the encode that wrote these 0 blocks");
            return HUFE_ARGUMENT;
        }
        if (!ctx) {
            set_err(NULL, "find_bytes: needs a context (there is no CPU path)");
            return HUFE_ARGUMENT;
        }
        HIP_OK(ctx, hipSetDevice(ctx->device));
        HIP_OK(ctx, hipMemsetAsync(d_totals, 0, 4 * sizeof(uint64_t), pick_stream(ctx, stream)));
        return HUFE_OK;
    }
    if (!d_stream || !d_block_offsets || !d_block_errs) {
        set_err(ctx, "find_bytes: the stream, its block index and d_block_errs are required");
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "find_bytes: needs the stream's sub-index in an 8-byte aligned buffer");
        return HUFE_ARGUMENT;
    }
    if (blocksize == 0) blocksize = raw_size;
    const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
    const uint64_t wpb = (blocksize + DSUB_SPL - 1) / DSUB_SPL, tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    if (raw_size == 0 || blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, blocksize) != nblocks ||
        nblocks > 0x7fffffffull || nblocks * tpb > 0x7fffffffull) {
        set_err(ctx, "find_bytes: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks (at most 2^31 - 1 tiles)",
                (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "find_bytes: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int rc = ensure_find_ws(ctx, nblocks * wpb, nblocks * tpb);
    if (rc) return rc;

    FindArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.s = sub_stream_args(d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize, flags);
    fa.cpb = (uint32_t)cpb;
    for (int i = 0; i < 32; i++) fa.set[i >> 2] |= (uint32_t)set[i] << (8 * (i & 3));
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
    find_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(fa);
    find_scan_kernel<<<dim3((unsigned)((fa.ntiles + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(fa);
    find_finish_kernel<<<dim3(grid256(nblocks)), dim3(256), 0, s>>>(fa);
    if (pos_cap > 0) {
        const uint64_t per = FIND_EMIT_THREADS / 64;
        find_emit_kernel<<<dim3((unsigned)((fa.ntiles + per - 1) / per)), dim3(FIND_EMIT_THREADS), 0, s>>>(fa);
    }
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

/* sub_build.hpp - the sub-index of a stream that came without one (include/huffman_gpu.h, kernels/sub_build.hpp):
   hufgpu_sub_index_from_raw, hufgpu_decode_build_sub and hufgpu_build_sub_index.
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* hufgpu_build_sub_index decodes this many bytes of whole blocks at a time into the context's scratch area (one block
 * when a block is longer): half of the 256 MiB Infinity Cache, so the builder reads what the decoder has just written
 * from there, and 2 048 blocks of 64 KiB - eight for each of the 256 CUs - a slab */
#define SUB_SLAB_BYTES (128ull << 20)

/* what the three entry points check alike, before the context is looked at; blocksize 0 becomes raw_size */
static int sub_build_check(hufgpu_ctx *ctx, const char *who, const void *d_stream, const uint64_t *d_block_offsets, uint64_t raw_size,
                           uint64_t *blocksize, const void *d_sub_index)
{
    if (!d_stream || !d_block_offsets) {
        set_err(NULL, "%s: the stream or its block index is missing", who);
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(NULL, "%s: the sub-index buffer must be there and 8-byte aligned", who);
        return HUFE_ARGUMENT;
    }
    if (*blocksize == 0) *blocksize = raw_size;
    const uint64_t cpb = *blocksize >= HUF_CHUNKED_FROM ? (*blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS : 1;
    if (*blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, *blocksize) * cpb > 0x7fffffffull) {
        set_err(NULL, "%s: blocks of more than %llu bytes, or more than 2^31 - 1 blocks or chunks", who, (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "%s: needs a context (there is no CPU path)", who);
        return HUFE_ARGUMENT;
    }
    return HUFE_OK;
}

/* one launch sequence: the rows of blocks blk0 .. blk0 + nblk - 1, whose decoded bytes start at `raw` */
static int sub_build_enqueue(hufgpu_ctx *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                             const void *raw, uint64_t raw_avail, uint64_t raw_size, uint64_t blocksize, uint64_t blk0, uint64_t nblk,
                             void *d_sub_index, uint32_t flags, const int32_t *dec_status, hipStream_t s)
{
    const uint64_t cpb = blocksize >= HUF_CHUNKED_FROM ? (blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS : 1;
    int rc = ensure_sub_build_ws(ctx, nblk, cpb > 1 ? nblk * cpb : 0);
    if (rc) return rc;
    SubBuildArgs a;
    memset(&a, 0, sizeof(a));
    a.stream = (const uint8_t *)d_stream;
    a.stream_len = stream_len;
    a.offsets = d_block_offsets;
    a.raw = (const uint8_t *)raw;
    a.raw_avail = raw_avail;
    a.n = raw_size;
    a.blocksize = blocksize;
    a.blk0 = blk0;
    a.nblk = (uint32_t)nblk;
    a.cpb = (uint32_t)cpb;
    a.max_tree = max_tree_of(flags);
    a.dec_status = dec_status;
    a.sub = sub_index_view(d_sub_index, raw_size, blocksize);
    a.state = ctx->d_sb_state;
    a.pay_bytes = ctx->d_sb_pay;
    a.chunk_tot = ctx->d_sb_chunk_tot;
    a.chunk_bits = ctx->d_sb_chunk_bits;
    a.unbuilt = ctx->d_sb_unbuilt;
    static const bool wide_table = getenv("HUF_GPU_SUB_TABLE") && atoi(getenv("HUF_GPU_SUB_TABLE")) == 1;   /* (measurements: the 8-byte table reads) */
    sub_lens_kernel<<<dim3((unsigned)nblk), dim3(SB_THREADS), 0, s>>>(a);
    if (wide_table) sub_groups_kernel<1><<<dim3((unsigned)(nblk * cpb)), dim3(SB_THREADS), 0, s>>>(a);
    else sub_groups_kernel<0><<<dim3((unsigned)(nblk * cpb)), dim3(SB_THREADS), 0, s>>>(a);
    if (cpb > 1) {
        sub_chunk_scan_kernel<SCAN_THREADS><<<dim3((unsigned)nblk), dim3(SCAN_THREADS), 0, s>>>(a);
        sub_tile_add_kernel<<<dim3((unsigned)(nblk * cpb)), dim3(HUF_CHUNK_SYMS / HUF_SUB_TILE), 0, s>>>(a);
    }
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

static int sub_build_count(hufgpu_ctx *ctx, uint64_t *unbuilt, hipStream_t s)
{
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 10, ctx->d_sb_unbuilt, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    *unbuilt = ctx->h_result[10];
    return HUFE_OK;
}

extern "C" int hufgpu_sub_index_from_raw(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                         const void *d_raw, uint64_t raw_size, uint64_t blocksize, void *d_sub_index, uint32_t flags,
                                         uint64_t *unbuilt, void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) return HUFE_OK;
    if (!d_raw) {
        set_err(NULL, "sub_index_from_raw: the decoded data is missing");
        return HUFE_ARGUMENT;
    }
    int rc = sub_build_check(ctx, "sub_index_from_raw", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, d_raw, raw_size, raw_size, blocksize, 0, nb, d_sub_index, flags, NULL, s);
    if (rc) return rc;
    return unbuilt ? sub_build_count(ctx, unbuilt, s) : HUFE_OK;
}

extern "C" int hufgpu_decode_build_sub(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                       uint64_t raw_size, uint64_t blocksize, void *d_out, uint64_t out_cap, void *d_sub_index,
                                       uint32_t flags, uint64_t *raw_len, uint64_t *unbuilt, void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) {
        if (ctx) ctx->decode_pending = 0;
        if (raw_len) *raw_len = 0;
        return HUFE_OK;
    }
    if (!d_out && out_cap) {
        set_err(NULL, "decode_build_sub: the output buffer is missing");
        return HUFE_ARGUMENT;
    }
    int rc = sub_build_check(ctx, "decode_build_sub", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    rc = decode_impl(ctx, d_stream, stream_len, d_block_offsets, nb, NULL, 0, d_out, out_cap, flags, NULL, stream);
    if (rc) return rc;
    if (!ctx->decode_pending) {                    /* an empty stream: nothing was decoded, no row can be built */
        if (raw_len) *raw_len = 0;
        if (unbuilt) *unbuilt = nb;
        return HUFE_OK;
    }
    hipStream_t s = pick_stream(ctx, stream);
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    /* the rows come from the output just written: a block that did not decode (d_status) is unbuilt */
    rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, d_out, out_cap < raw_size ? out_cap : raw_size, raw_size, blocksize, 0, nb,
                           d_sub_index, flags, ctx->d_status, s);
    if (rc) return rc;
    if (unbuilt) {                                 /* (read first: hufgpu_decode_result may go on to decode a failing block again) */
        rc = sub_build_count(ctx, unbuilt, s);
        if (rc) return rc;
    }
    return raw_len ? hufgpu_decode_result(ctx, raw_len) : HUFE_OK;
}

extern "C" int hufgpu_build_sub_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                      uint64_t raw_size, uint64_t blocksize, void *d_sub_index, uint32_t flags, uint64_t *unbuilt,
                                      void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) return HUFE_OK;
    int rc = sub_build_check(ctx, "build_sub_index", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    if (stream_len == 0) {                         /* an empty stream: no row can be built */
        if (unbuilt) *unbuilt = nb;
        return HUFE_OK;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t slab_blocks = blocksize >= SUB_SLAB_BYTES ? 1 : (nb < SUB_SLAB_BYTES / blocksize ? nb : SUB_SLAB_BYTES / blocksize);
    const uint64_t need = slab_blocks * blocksize < raw_size ? slab_blocks * blocksize : raw_size;
    rc = grow_range_scratch(ctx, need);           /* the staging area of hufgpu_decode_ranges */
    if (rc == HUFE_MEMORY)
        set_err(ctx, "build_sub_index: no room for %llu decoded blocks of %llu bytes", (unsigned long long)slab_blocks,
                (unsigned long long)blocksize);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    for (uint64_t b0 = 0; b0 < nb; b0 += slab_blocks) {
        const uint64_t k = nb - b0 < slab_blocks ? nb - b0 : slab_blocks;
        const uint64_t bytes = b0 + k == nb ? raw_size - b0 * blocksize : k * blocksize;
        rc = decode_impl(ctx, d_stream, stream_len, d_block_offsets + b0, k, NULL, 0, ctx->d_rscratch, bytes, flags, NULL, stream);
        if (rc == HUFE_OK)
            rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, ctx->d_rscratch, bytes, raw_size, blocksize, b0, k, d_sub_index,
                                   flags, ctx->d_status, s);
        if (rc) break;
    }
    /* the slabs' decodes were this call's own: nothing of them is left for hufgpu_decode_result() */
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    uint64_t cnt = 0;
    const int rc2 = sub_build_count(ctx, &cnt, s);
    if (rc) return rc;
    if (rc2) return rc2;
    if (unbuilt) *unbuilt = cnt;
    return HUFE_OK;
}

/* encode.hpp - hufgpu_encode and its kin: the block and sub-index geometry (hufgpu_block_count, hufgpu_encode_bound,
   sub_index_view, hufgpu_sub_index_bytes), hufgpu_histogram, encode_impl behind hufgpu_encode / hufgpu_encode_sub, and
   the one-wait hufgpu_encode_small.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

extern "C" uint64_t hufgpu_block_count(uint64_t n, uint64_t blocksize)
{
    if (n == 0) return 0;
    if (blocksize == 0) blocksize = n;            /* src/encoder.c:163-165 */
    return (n + blocksize - 1) / blocksize;
}

extern "C" uint64_t hufgpu_encode_bound(uint64_t n, uint64_t blocksize)
{
    /* per block: 10 + 2*1025 header; payload <= 9 bits per byte (an optimal prefix code never
     * costs more than the 8-bit fixed code, plus the wrap-root bit), +1 byte of padding */
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    return nb * (HUF_HEADER_FIXED + 2ull * HUF_TREE_MAX + 1) + (n * 9 + 7) / 8 + 16;
}

static int check_block_args(hufgpu_ctx *c, uint64_t n, uint64_t *blocksize)
{
    if (*blocksize == 0) *blocksize = n;
    if (*blocksize > HUFGPU_MAX_BLOCK) {
        set_err(c, "blocksize %llu exceeds the kernel limit of %llu bytes", (unsigned long long)*blocksize,
                (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUFE_ARGUMENT;
    }
    return HUFE_OK;
}

extern "C" int hufgpu_histogram(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                                uint32_t *d_hist, void *stream)
{
    if (!ctx || (!d_in && n) || !d_hist) return HUFE_ARGUMENT;
    if (n == 0) return HUFE_OK;
    int rc = check_block_args(ctx, n, &blocksize);
    if (rc) return rc;
    if (blocksize > 0xffffffffull) {
        set_err(ctx, "hufgpu_histogram returns 32-bit counts: blocks of 2^32 bytes and more are not taken");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    hist256_kernel<HIST_THREADS><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>((const uint8_t *)d_in, n, blocksize, d_hist);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

/* where the two arrays of a sub-index live inside the caller's buffer */
static HufSubIndex sub_index_view(void *d_sub, uint64_t n, uint64_t blocksize)
{
    HufSubIndex v;
    memset(&v, 0, sizeof(v));
    if (!d_sub || n == 0) return v;
    if (blocksize == 0) blocksize = n;
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    v.gpb = ((blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;   /* rows of 16-byte multiples */
    v.tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    v.tile_bits = (uint64_t *)d_sub;
    v.group_bits = (uint16_t *)((uint64_t *)d_sub + nb * v.tpb);
    v.lens = (uint8_t *)(v.group_bits + nb * v.gpb);        /* gpb is a multiple of 8: 16-byte aligned */
    return v;
}

extern "C" uint64_t hufgpu_sub_index_bytes(uint64_t n, uint64_t blocksize)
{
    if (n == 0) return 0;
    if (blocksize == 0) blocksize = n;
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    const uint64_t gpb = ((blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;
    const uint64_t tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    return nb * tpb * sizeof(uint64_t) + nb * gpb * sizeof(uint16_t) + nb * HUF_NSYM;
}

static int encode_impl(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                       void *d_out, uint64_t out_cap, uint64_t *d_block_offsets, void *d_sub_index,
                       uint64_t *out_len, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (n == 0) {                                  /* src/encoder.c:288: nothing to do */
        if (out_len) *out_len = 0;
        if (d_block_offsets) {                     /* the index of an empty stream: its length, 0 */
            HIP_OK(ctx, hipSetDevice(ctx->device));
            HIP_OK(ctx, hipMemsetAsync(d_block_offsets, 0, sizeof(uint64_t), pick_stream(ctx, stream)));
        }
        return HUFE_OK;
    }
    if (!d_in || !d_out) return HUFE_ARGUMENT;
    int rc = check_block_args(ctx, n, &blocksize);
    if (rc) return rc;
    if (out_cap < hufgpu_encode_bound(n, blocksize)) {
        set_err(ctx, "output capacity %llu below hufgpu_encode_bound() = %llu", (unsigned long long)out_cap,
                (unsigned long long)hufgpu_encode_bound(n, blocksize));
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    if (nb > 0x7fffffffull) {
        set_err(ctx, "too many blocks (%llu)", (unsigned long long)nb);
        return HUFE_ARGUMENT;
    }
    rc = ensure_encode_ws(ctx, nb);
    if (rc) return rc;
    hipStream_t s = pick_stream(ctx, stream);
    uint64_t *offs = d_block_offsets ? d_block_offsets : ctx->d_offsets;
    const uint8_t *in = (const uint8_t *)d_in;
    if (d_sub_index && ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "the sub-index buffer must be 8-byte aligned");
        return HUFE_ARGUMENT;
    }
    const HufSubIndex sub = sub_index_view(d_sub_index, n, blocksize);

    STAGE_BEGIN(ctx, s, PROF_ENCODE);
    TwoLevel sizes = ctx->enc_sizes;
    static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;   /* (measurements: the one-launch form) */
    if (blocksize < HUF_CHUNKED_FROM) {
        /* counts, tree and the sums of the encoded sizes in one launch (the profile's "tree" and
         * "scan_sizes" stages are then empty) */
        sizes.total = offs + nb;
        if (blocksize >= HL_MIN_BLOCK && !fused_only) {
            /* counts with lane-private counters at the rate HBM delivers, then the trees as a launch of their
             * own (kernels/hist_lanes.hpp): 0.19 + 0.13 ms per GiB on zipf255 where the fused kernel takes 0.44 */
            hist_lanes_kernel<HL_THREADS><<<dim3((unsigned)nb), dim3(HL_THREADS), 0, s>>>(in, n, blocksize, ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_wave_kernel<<<dim3((unsigned)nb), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
        } else
        if (blocksize <= HT_PACKED_MAX_BLOCK)
            hist_tree_kernel<HIST_THREADS, true><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        else
            hist_tree_kernel<HIST_THREADS, false><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        if (!(blocksize >= HL_MIN_BLOCK && !fused_only)) {
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
        }
    } else {
        /* blocks of HUF_BIG_BLOCK bytes and more are cut into chunks, one workgroup each (blocksize = 0:
         * the whole input is ONE block, src/encoder.c:163-165 - the reference's default) */
        const uint64_t cpb = (blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS;
        const uint64_t nchunks = nb * cpb;
        if (nchunks > 0x7fffffffull) return HUFE_ARGUMENT;
        rc = ensure_chunk_ws(ctx, nchunks);
        if (rc) return rc;
        ChunkGeom geo;
        geo.n = n;
        geo.blocksize = blocksize;
        geo.cpb = (uint32_t)cpb;
        chunk_hist_kernel<HL_THREADS><<<dim3((unsigned)nchunks), dim3(HL_THREADS), 0, s>>>(in, geo, ctx->d_chunk_hist);
        if (blocksize < HUF_BIG_BLOCK) {
            /* rates below 2^23: the wave-per-block tree with 32-bit keys (its sums of the encoded sizes are not used
             * here: scan_sizes_kernel writes the index below) */
            sizes.total = offs + nb;
            block_hist32_kernel<<<dim3((unsigned)nb), dim3(HUF_NSYM), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_wave_kernel<<<dim3((unsigned)nb), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        } else {
            block_hist_kernel<<<dim3((unsigned)nb), dim3(HUF_NSYM), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, (uint64_t *)ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_kernel<uint64_t, uint64_t><<<dim3((unsigned)nb), dim3(64), 0, s>>>((const uint64_t *)ctx->d_hist, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta);
        }
        STAGE_MARK(ctx, s);
        scan_sizes_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ctx->d_meta, nb, offs);
        chunk_total_kernel<<<dim3((unsigned)nchunks), dim3(64), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, ctx->d_codetab, ctx->d_meta, ctx->d_chunk_tot);
        chunk_scan_kernel<SCAN_THREADS><<<dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s>>>(ctx->d_chunk_tot, (uint32_t)cpb, ctx->d_chunk_bits);
        STAGE_MARK(ctx, s);
        sizes.local = NULL;              /* pack reads the finished index */
        PackChunk ck;
        ck.chunk_bits = ctx->d_chunk_bits;
        ck.chunk_syms = HUF_CHUNK_SYMS;
        ck.cpb = (uint32_t)cpb;
        pack_chunk_kernel<PACK_THREADS, false><<<dim3((unsigned)nchunks), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub, ck);
    }
    if (blocksize >= HUF_CHUNKED_FROM) {
        /* (packed above) */
    } else if (blocksize <= 121392ull)   /* deepest possible code <= 24 bits: 32-bit code path only */
        pack_kernel<PACK_THREADS, true><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
    else
        pack_kernel<PACK_THREADS, false><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
    STAGE_MARK(ctx, s);
    HIP_OK(ctx, hipGetLastError());

    if (out_len) {
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, offs + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        *out_len = ctx->h_result[0];
    }
    return HUFE_OK;
}

extern "C" int hufgpu_encode(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                             void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                             uint64_t *out_len, void *stream)
{
    return encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, d_block_offsets, NULL, out_len, stream);
}

extern "C" int hufgpu_encode_sub(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                                 void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                                 void *d_sub_index, uint64_t *out_len, void *stream)
{
    return encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, d_block_offsets, d_sub_index, out_len, stream);
}

/* One small encode with ONE synchronisation (include/huffman_gpu.h): input from pinned host memory, the stream and its
 * length back into pinned host memory.  A call through the general entry points waits three times (input up, the length,
 * the stream back); for inputs of a few KiB those waits are most of the call. */
extern "C" int hufgpu_encode_small(hufgpu_ctx_t *ctx, const void *h_in_pinned, uint64_t n, uint64_t blocksize, void *d_in,
                                   void *d_out, uint64_t out_cap, void *h_out_pinned, uint64_t h_out_cap, uint64_t *out_len)
{
    if (!ctx || !h_in_pinned || !d_in || !d_out || !h_out_pinned || !out_len || n == 0) return HUFE_ARGUMENT;
    const uint64_t bound = hufgpu_encode_bound(n, blocksize);
    const uint64_t len_at = (bound + 7u) & ~7ull;
    if (h_out_cap < len_at + 8u || out_cap < bound) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(d_in, h_in_pinned, n, hipMemcpyHostToDevice, s));
    const int rc = encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, NULL, NULL, NULL, (void *)s);
    if (rc != HUFE_OK) return rc;
    const uint64_t nb = hufgpu_block_count(n, blocksize ? blocksize : n);
    HIP_OK(ctx, hipMemcpyAsync(h_out_pinned, d_out, bound, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipMemcpyAsync((char *)h_out_pinned + len_at, ctx->d_offsets + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    *out_len = *(const uint64_t *)((const char *)h_out_pinned + len_at);
    return (*out_len <= bound) ? HUFE_OK : HUFE_FATAL;
}

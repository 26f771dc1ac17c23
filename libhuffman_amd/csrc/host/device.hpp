/* device.hpp - what the ABI offers besides the codec: device memory and copies, the data generator, the bandwidth
   calibration, and the counters of diagnostic builds.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* What the routes that serve straight from the sub-index are told of the stream and its layout (kernels/sub_tile.hpp):
 * hufgpu_gather, hufgpu_find_bytes and the tile route of hufgpu_decode_ranges.  blocksize: the layout's, never 0. */
static SubStream sub_stream_args(const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets, uint64_t nblocks,
                                 const void *d_sub_index, uint64_t raw_size, uint64_t blocksize, uint32_t flags)
{
    return {(const uint8_t *)d_stream, stream_len, d_block_offsets, nblocks, sub_index_view((void *)d_sub_index, raw_size, blocksize),
            raw_size, blocksize, max_tree_of(flags)};
}

extern "C" int hufgpu_fill(hufgpu_ctx_t *ctx, void *d_out, uint64_t n, int kind, uint64_t seed,
                           uint64_t first, void *stream)
{
    if (!ctx || (!d_out && n) || kind < 0 || kind > 3) return HUFE_ARGUMENT;
    if (n == 0) return HUFE_OK;
    if (kind == 1 && (first & 7)) {
        set_err(ctx, "uniform256 shards must start on an 8-byte boundary");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    fill_kernel<<<dim3(4096), dim3(256), 0, s>>>((uint8_t *)d_out, n, kind, seed, first, ctx->d_zipf);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

extern "C" int hufgpu_malloc(hufgpu_ctx_t *ctx, void **d_ptr, uint64_t bytes)
{
    if (!ctx || !d_ptr) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_err(ctx, "hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
        return HUFE_MEMORY;
    }
    return HUFE_OK;
}

extern "C" int hufgpu_free(hufgpu_ctx_t *ctx, void *d_ptr)
{
    if (!ctx) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipFree(d_ptr));
    return HUFE_OK;
}

extern "C" int hufgpu_memcpy_h2d(hufgpu_ctx_t *ctx, void *d_dst, const void *h_src, uint64_t bytes)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (!bytes) return HUFE_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return HUFE_OK;
}

extern "C" int hufgpu_memcpy_d2h(hufgpu_ctx_t *ctx, void *h_dst, const void *d_src, uint64_t bytes)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (!bytes) return HUFE_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return HUFE_OK;
}

extern "C" int hufgpu_memcpy_d2d(hufgpu_ctx_t *ctx, void *d_dst, const void *d_src, uint64_t bytes)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (!bytes) return HUFE_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return HUFE_OK;
}

extern "C" int hufgpu_synchronize(hufgpu_ctx_t *ctx)
{
    if (!ctx) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    HIP_OK(ctx, hipStreamSynchronize(ctx->stream));
    return HUFE_OK;
}

/* Bandwidth calibration (include/huffman_gpu.h): one launch of a kernel that only moves bytes. */
template <int KIND>
static int calib_launch(int variant, const uint8_t *a, uint8_t *b, uint64_t bytes, uint32_t *flag, hipStream_t s)
{
#define CALIB_CASE(V, T, P, NTL, NTS) case V: calib_bw_kernel<T, P, KIND, NTL, NTS><<<dim3((unsigned)(bytes / P)), dim3(T), 0, s>>>(a, b, flag); return P;
    switch (variant) {
        CALIB_CASE(0, 256, 16384, true, true)
        CALIB_CASE(1, 256, 16384, true, false)
        CALIB_CASE(2, 256, 16384, false, false)
        CALIB_CASE(3, 512, 65536, true, true)
        CALIB_CASE(4, 512, 65536, true, false)
        CALIB_CASE(5, 256, 4096, true, true)
        CALIB_CASE(6, 256, 4096, false, false)
        CALIB_CASE(7, 1024, 65536, true, true)
    }
#undef CALIB_CASE
    return 0;
}
extern "C" int hufgpu_calib_bandwidth(hufgpu_ctx_t *ctx, int kind, int variant, const void *d_a, void *d_b, uint64_t bytes, void *stream)
{
    if (!ctx || kind < 0 || kind > 2 || variant < 0 || variant >= HUFGPU_CALIB_VARIANTS) return HUFE_ARGUMENT;
    if ((kind != 2 && !d_a) || (kind != 1 && !d_b) || bytes == 0 || (bytes & 65535u) || (((uintptr_t)d_a | (uintptr_t)d_b) & 15u)) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    uint32_t *flag = (uint32_t *)ctx->d_result;          /* (a word nobody reads: the read-only kernel's "result") */
    int per = 0;
    if (kind == 0) per = calib_launch<0>(variant, (const uint8_t *)d_a, (uint8_t *)d_b, bytes, flag + 6, s);
    else if (kind == 1) per = calib_launch<1>(variant, (const uint8_t *)d_a, (uint8_t *)d_b, bytes, flag + 6, s);
    else per = calib_launch<2>(variant, (const uint8_t *)d_a, (uint8_t *)d_b, bytes, flag + 6, s);
    HIP_OK(ctx, hipGetLastError());
    return per ? HUFE_OK : HUFE_ARGUMENT;
}

#ifdef DFAST_DEBUG
extern "C" int hufgpu_debug_dfast(unsigned long long *out32, int reset)     /* DFAST_DBG_SLOTS counters */
{
    if (reset) { unsigned long long z[DFAST_DBG_SLOTS] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(hufgpu::g_dfast_dbg), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out32, HIP_SYMBOL(hufgpu::g_dfast_dbg), DFAST_DBG_SLOTS * sizeof(unsigned long long));
}
#endif
#ifdef TREE_DEBUG
extern "C" int hufgpu_debug_tree(unsigned long long *out, int reset)        /* TREE_DBG_SLOTS counters (kernels/tree.hpp) */
{
    if (reset) { unsigned long long z[TREE_DBG_SLOTS] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(hufgpu::g_tree_dbg), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(hufgpu::g_tree_dbg), TREE_DBG_SLOTS * sizeof(unsigned long long));
}
#endif

#ifdef DEC_PHASE_PROF
/* diagnostic builds only: cycle sums of the decode phases (thread 0 of every workgroup) */
extern "C" int hufgpu_debug_phase_cycles(hufgpu_ctx_t *ctx, unsigned long long *out16, int reset)
{
    if (!ctx || !out16) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipDeviceSynchronize());
    HIP_OK(ctx, hipMemcpyFromSymbol(out16, HIP_SYMBOL(hufgpu::g_dec_prof), 16 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[16] = {0};
        HIP_OK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(hufgpu::g_dec_prof), z, sizeof(z)));
    }
    return HUFE_OK;
}
#endif

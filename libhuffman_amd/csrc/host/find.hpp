/* find.hpp - hufgpu_find_bytes and hufgpu_find_pattern: where the bytes of a set of byte values lie in the original
   data, and where a pattern of bytes starts (include/huffman_gpu.h, kernels/find.hpp), enqueue-only.  Part of
   hufgpu_api.hip (one translation unit). */
#pragma once

static_assert(FIND_PAT_MAX == HUFGPU_FIND_PATTERN_MAX, "kernels/find.hpp and include/huffman_gpu.h");

/* Both calls: `who` words the errors, `key` is the set (plen = 0) or the pattern of plen bytes, `key_name` its name. */
static int find_call(hufgpu_ctx_t *ctx, const char *who, const char *key_name, const uint8_t *key, uint32_t plen,
                     const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets, uint64_t nblocks,
                     const void *d_sub_index, uint64_t raw_size, uint64_t blocksize, uint64_t *d_pos, uint64_t pos_cap,
                     uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs, uint32_t flags, void *stream)
{
    if (!key || !d_totals) {
        set_err(ctx, "%s: the %s and d_totals are required", who, key_name);
        return HUFE_ARGUMENT;
    }
    if (pos_cap > 0 && !d_pos) {
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
    if (rc) return rc;

    FindPatArgs pa;
    memset(&pa, 0, sizeof(pa));
    FindArgs &fa = pa.f;
    fa.s = sub_stream_args(d_stream, stream_len, d_block_offsets, nblocks, d_sub_index, raw_size, blocksize, flags);
    fa.cpb = (uint32_t)cpb;
    if (plen == 0) {
        for (int i = 0; i < 32; i++) fa.set[i >> 2] |= (uint32_t)key[i] << (8 * (i & 3));
    } else {
        for (uint32_t i = 0; i < plen; i++) pa.pat[i >> 2] |= (uint32_t)key[i] << (8 * (i & 3));
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
    if (plen == 0) {
        find_sub_kernel<<<dim3((unsigned)(nblocks * cpb)), dim3(FIND_THREADS), 0, s>>>(fa);
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

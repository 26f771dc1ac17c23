/* decode.hpp - decodes with a known block index: the in-order chain (decode_chain), hufgpu_decode_result, the ONE place
   that launches decode_prepare_kernel and the indexed decoders (decode_sub_kernel or decode_fast_kernel, then
   decode_fix_kernel) for every feature that decodes blocks by their index, decode_impl behind hufgpu_decode /
   hufgpu_decode_sub, and the one-wait hufgpu_decode_small.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

static inline int max_tree_of(uint32_t flags) { return (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT; }

/* The exact sequential decoder (one workgroup, blocks in order). */
static int decode_chain(hufgpu_ctx *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint8_t *out,
                        uint64_t out_cap, int max_tree, hipStream_t s, uint64_t *raw, uint64_t *used,
                        uint64_t *good_used, uint64_t *good_raw)
{
    decode_chain_kernel<DEC_THREADS><<<dim3(1), dim3(DEC_THREADS), 0, s>>>(st, avail, length, max_tree, out, out_cap, ctx->d_result, NULL, 0);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_result, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    *raw = ctx->h_result[1];
    *used = ctx->h_result[2];
    *good_used = ctx->h_result[4];
    *good_raw = ctx->h_result[5];
    return (int)ctx->h_result[0];
}

extern "C" int hufgpu_decode_result(hufgpu_ctx_t *ctx, uint64_t *raw_len)
{
    if (!ctx) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (!ctx->decode_pending) {
        if (raw_len) *raw_len = 0;
        return HUFE_OK;
    }
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_result, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->last_stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->last_stream));
    ctx->decode_pending = 0;
    const uint8_t *last_st = ctx->last_st;
    ctx->last_st = NULL;                           /* the caller's buffers are not looked at again after this call */
    const uint64_t failing = ctx->h_result[2];
    ctx->last_failing = failing;
    if (failing == ~0ull) {                        /* every block decoded */
        if (raw_len) *raw_len = ctx->h_result[1];
        return HUFE_OK;
    }
    /* first failing block in stream order: its error code, and the bytes of the blocks before it */
    int32_t err = HUFE_FATAL;
    uint64_t before = 0;
    HIP_OK(ctx, hipMemcpyAsync(&err, ctx->d_status + failing, sizeof(err), hipMemcpyDeviceToHost, ctx->last_stream));
    HIP_OK(ctx, hipMemcpyAsync(&before, ctx->d_out_offsets + failing, sizeof(before), hipMemcpyDeviceToHost, ctx->last_stream));
    HIP_OK(ctx, hipStreamSynchronize(ctx->last_stream));
    if ((err == HUFE_RW || err == HUFE_CORRUPTED) && last_st && failing < ctx->last_nblocks && before <= ctx->last_out_cap) {
        /* src/decoder.c:69-91 delivers the symbols in front of the failure: the failing block once more by the
         * exact in-order decoder, its record [o0, o1) as the whole input (a walk that needs more fails like the
         * reference's reader at the end of its input) */
        uint64_t o[2] = {0, 0};
        HIP_OK(ctx, hipMemcpyAsync(o, ctx->last_offsets + failing, sizeof(o), hipMemcpyDeviceToHost, ctx->last_stream));
        HIP_OK(ctx, hipStreamSynchronize(ctx->last_stream));
        if (o[1] > ctx->last_stream_len) o[1] = ctx->last_stream_len;
        if (o[0] < o[1]) {
            uint64_t raw = 0, used = 0, gu = 0, gr = 0;
            const int rc = decode_chain(ctx, last_st + o[0], o[1] - o[0], 1, ctx->last_out + before, ctx->last_out_cap - before,
                                        ctx->last_max_tree, ctx->last_stream, &raw, &used, &gu, &gr);
            if (rc == err) before += raw;
        }
    }
    if (raw_len) *raw_len = before;
    if (err == HUFE_ARGUMENT) set_err(ctx, "block %llu is longer than the kernels support", (unsigned long long)failing);
    if (err == HUFE_MEMORY) set_err(ctx, "output buffer too small (block %llu)", (unsigned long long)failing);
    return err;
}

/* How many blocks of the last enqueued decode were handed on: counters[0] = to the exact decoder
 * (decode_fix_kernel), counters[1] = 0 (round 4's one-pass decoder, gone with round 5's clean-up).  Synchronises. */
extern "C" int hufgpu_decode_counters(hufgpu_ctx_t *ctx, uint32_t *counters)
{
    if (!ctx || !counters) return HUFE_ARGUMENT;
    counters[0] = counters[1] = 0;
    if (!ctx->d_fix_count) return HUFE_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (ctx->last_stream || ctx->decode_pending) HIP_OK(ctx, hipStreamSynchronize(ctx->last_stream));
    HIP_OK(ctx, hipMemcpy(counters, ctx->d_fix_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HUFE_OK;
}

/* ---- the indexed decoders: prepare the block headers, then decode blocks by their index (the text after "decode:" in
 * the header of hufgpu_kernels.hip).  Every feature that decodes by an index goes through the two routines below, so
 * what the three launches of one call must agree on is stated once, by the caller, in one IndexedDecode. ---- */

/* the context's two-level sums of the lengths of nb blocks: their total goes to result[1] and behind the nb output
 * offsets, the first failing block to result[2] */
static TwoLevel decode_lens(hufgpu_ctx *ctx, uint64_t nb)
{
    TwoLevel lens = ctx->dec_lens;
    lens.total = ctx->d_result + 1;
    lens.total2 = ctx->d_out_offsets + nb;
    lens.min_out = ctx->d_result + 2;
    return lens;
}

/* header parse + two-level sums of the block lengths (`lens`: decode_lens() of the same nb); also (re)initialises
 * result[1] and [2] and the list of blocks for decode_fix_kernel */
static void launch_decode_prepare(hufgpu_ctx *ctx, const uint8_t *st, uint64_t stream_len, const uint64_t *offsets, uint64_t nb,
                                  int max_tree, const TwoLevel &lens, hipStream_t s)
{
    decode_prepare_kernel<<<dim3((unsigned)((nb + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, offsets, nb, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);
}

struct IndexedDecode {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *offsets;      /* the index of the nb blocks launch_decode_prepare() was given */
    uint64_t nb;
    TwoLevel lens;                /* where a block's output starts: decode_lens(), or a caller's view of it with offsets of its own */
    uint8_t *out;
    uint64_t out_cap;
    const HufSubIndex *sub;       /* NULL or tile_bits == 0: no sub-index */
    uint64_t sub_blocksize;       /* the symbols a row of the sub-index covers */
};

/* Behind launch_decode_prepare(): with the encoder's sub-index one table pass per symbol, verified (decode_sub_kernel);
 * without it the lean self-synchronising decoder (kernels/decode_fast.hpp).  What either cannot vouch for - a damaged
 * stream, an unusual tree - is decoded again by the exact decoder (decode_fix_kernel), which also reports the
 * reference's error.  Enqueues only. */
static int launch_indexed_decoders(hufgpu_ctx *ctx, const IndexedDecode &job, hipStream_t s)
{
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    DecFixList fix;
    fix.count = ctx->d_fix_count;
    fix.blocks = ctx->d_fix_blocks;
    fix.flag = ctx->d_fix_flag;
    if (job.sub && job.sub->tile_bits) {
        const uint64_t cpb = (job.sub_blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
        if (job.nb * cpb > 0x7fffffffull) return HUFE_ARGUMENT;
        decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)(job.nb * cpb)), dim3(DSUB_THREADS), 0, s>>>(job.stream, job.stream_len, job.offsets, ctx->d_dmeta, ctx->d_out_offsets, job.lens, job.out, job.out_cap, ctx->d_status, res, *job.sub, job.sub_blocksize, (uint32_t)cpb, fix);
    } else {
        DecodeFastArgs fa;
        fa.stream = job.stream; fa.stream_len = job.stream_len; fa.offsets = job.offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
        fa.lens = job.lens; fa.out = job.out; fa.out_cap = job.out_cap; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
        decode_fast_kernel<DEC_THREADS><<<dim3((unsigned)job.nb), dim3(DEC_THREADS), 0, s>>>(fa);
    }
    const unsigned fix_grid = (unsigned)(job.nb < 1024 ? job.nb : 1024);
    decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(job.stream, job.stream_len, job.offsets, ctx->d_dmeta, job.lens, job.out, job.out_cap, ctx->d_status, res, fix);
    return HUFE_OK;
}

/* (measurements: the exact decoder for every block of a decode without a sub-index) */
static bool exact_decode_only(void)
{
    static const bool exact_only = getenv("HUF_GPU_EXACT_DECODE") && atoi(getenv("HUF_GPU_EXACT_DECODE")) != 0;
    return exact_only;
}

static int decode_impl(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                       const uint64_t *d_block_offsets, uint64_t nblocks, const HufSubIndex *sub, uint64_t blocksize,
                       void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (nblocks == 0 || stream_len == 0) {         /* src/decoder.c:218, test/decode_test.c:32-36 */
        ctx->decode_pending = 0;
        if (raw_len) *raw_len = 0;
        return HUFE_OK;
    }
    if (!d_stream || !d_block_offsets || (!d_out && out_cap)) return HUFE_ARGUMENT;
    if (nblocks > 0x7fffffffull) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_decode_ws(ctx, nblocks);
    if (rc) return rc;
    hipStream_t s = pick_stream(ctx, stream);
    const int max_tree = max_tree_of(flags);
    const uint8_t *st = (const uint8_t *)d_stream;

    STAGE_BEGIN(ctx, s, PROF_DECODE);
    const TwoLevel lens = decode_lens(ctx, nblocks);
    launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nblocks, max_tree, lens, s);
    STAGE_MARK(ctx, s);
    if (!(sub && sub->tile_bits) && exact_decode_only()) {
        decode_kernel<DEC_THREADS><<<dim3((unsigned)nblocks), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, lens, (uint8_t *)d_out, out_cap, ctx->d_status, (unsigned long long *)ctx->d_result);
    } else {
        const IndexedDecode job = {st, stream_len, d_block_offsets, nblocks, lens, (uint8_t *)d_out, out_cap, sub, blocksize};
        rc = launch_indexed_decoders(ctx, job, s);
        if (rc) return rc;
    }
    STAGE_MARK(ctx, s);
    HIP_OK(ctx, hipGetLastError());
    ctx->decode_pending = 1;
    ctx->last_stream = s;
    ctx->last_st = st;
    ctx->last_stream_len = stream_len;
    ctx->last_offsets = d_block_offsets;
    ctx->last_nblocks = nblocks;
    ctx->last_out = (uint8_t *)d_out;
    ctx->last_out_cap = out_cap;
    ctx->last_max_tree = max_tree;
    if (raw_len) return hufgpu_decode_result(ctx, raw_len);
    return HUFE_OK;
}

extern "C" int hufgpu_decode(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                             const uint64_t *d_block_offsets, uint64_t nblocks, void *d_out,
                             uint64_t out_cap, uint32_t flags, uint64_t *raw_len, void *stream)
{
    return decode_impl(ctx, d_stream, stream_len, d_block_offsets, nblocks, NULL, 0, d_out, out_cap, flags, raw_len, stream);
}

extern "C" int hufgpu_decode_sub(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                 const uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                                 const void *d_sub_index, void *d_out, uint64_t out_cap, uint32_t flags,
                                 uint64_t *raw_len, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (blocksize == 0) blocksize = raw_size;
    const uint64_t nblocks = hufgpu_block_count(raw_size, blocksize);
    if (d_sub_index && ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "the sub-index buffer must be 8-byte aligned");
        return HUFE_ARGUMENT;
    }
    const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
    return decode_impl(ctx, d_stream, stream_len, d_block_offsets, nblocks, &sub, blocksize, d_out, out_cap, flags, raw_len, stream);
}

/* One small decode with ONE synchronisation (include/huffman_gpu.h), hufgpu_encode_small's twin: the raw stream from pinned
 * host memory, the in-order chain (decode_chain_lean_kernel: the block loop of src/decoder.c:218-276, one workgroup, the lean decoders in
 * front of the exact one), the output and the kernel's six
 * result words back into pinned host memory behind one another.  A call through the general entry points waits three
 * times (stream up, the result words, the output back): 62-140 microseconds where the kernel takes twenty. */
extern "C" int hufgpu_decode_small(hufgpu_ctx_t *ctx, const void *h_in_pinned, uint64_t avail, uint64_t length, uint32_t flags,
                                   void *d_in, void *d_out, uint64_t out_cap, void *h_out_pinned, uint64_t h_out_cap,
                                   uint64_t *raw_len, uint64_t *consumed)
{
    if (!ctx || !h_in_pinned || !d_in || !d_out || !h_out_pinned || !raw_len || !consumed || avail == 0) return HUFE_ARGUMENT;
    const uint64_t bound = out_cap < avail * 8u + 64u ? out_cap : avail * 8u + 64u;         /* (a symbol takes a bit at least) */
    /* what comes back with the result words: twice the stream and a bit - all of the output unless the stream is less than half
     * of it (round 6; until then the whole bound, eight times the stream, came back every time: 0.5 MiB for a call of 64 KiB).
     * The rest, if there is one, follows in a second copy. */
    const uint64_t first = 2u * avail + 4096u;
    const uint64_t copy = bound < first ? bound : first;
    const uint64_t res_at = (bound + 7u) & ~7ull;
    if (h_out_cap < res_at + 6u * sizeof(uint64_t)) return HUFE_ARGUMENT;
    *raw_len = *consumed = 0;
    if (length == 0) return HUFE_OK;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int max_tree = max_tree_of(flags);
    HIP_OK(ctx, hipMemcpyAsync(d_in, h_in_pinned, avail, hipMemcpyHostToDevice, s));
    decode_chain_lean_kernel<DEC_THREADS><<<dim3(1), dim3(DEC_THREADS), 0, s>>>((const uint8_t *)d_in, avail, length, max_tree, (uint8_t *)d_out, out_cap, ctx->d_result);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipMemcpyAsync(h_out_pinned, d_out, copy, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipMemcpyAsync((char *)h_out_pinned + res_at, ctx->d_result, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const uint64_t *r = (const uint64_t *)((const char *)h_out_pinned + res_at);
    *raw_len = r[1];
    *consumed = r[2];
    ctx->complete_used = r[4];
    ctx->complete_raw = r[5];
    if (r[1] > bound) return HUFE_FATAL;                                                      /* (cannot be: more symbols than bits) */
    if (r[1] > copy) {
        HIP_OK(ctx, hipMemcpyAsync((char *)h_out_pinned + copy, (const char *)d_out + copy, r[1] - copy, hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
    }
    return (int)r[0];
}

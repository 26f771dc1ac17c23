/* stream.hpp - decodes of a raw stream, whose block index is not known: the discovery of the block chain
   (kernels/discover.hpp), the sub-index built for leading blocks of many MiB (kernels/spec_index.hpp), the general path
   behind both, hufgpu_block_index and hufgpu_decode_stream.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* The block chain of a raw stream (kernels/discover.hpp): candidates, probes, links, walk.  On return
 * ctx->d_chain holds the header offsets of the *m blocks the walk validated (+ the offset behind them),
 * *resume = the stream offset behind the validated blocks, *complete = the chain ends the stream exactly
 * as src/decoder.c:218 would, *in_place = output bytes the probes already put where they belong (~0: none;
 * only when `out` has room for every candidate).  *m = 0: nothing validated. */
static int discover_chain(hufgpu_ctx_t *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint64_t scan_len, int max_tree,
                          uint8_t *out, uint64_t out_cap, hipStream_t s, uint64_t *m_out, uint64_t *resume_out,
                          bool *complete_out, uint64_t *in_place_out)
{
    *m_out = 0; *resume_out = 0; *complete_out = false; *in_place_out = ~0ull;
    ctx->scounters[0] = 1;                                               /* (hufgpu_stream_counters; the rest is 0 from the entry point) */
    ctx->scounters[6] = ~0ull;                                           /* nothing in place, also when no candidate is found */
    const uint64_t nwg = (scan_len + DISC_CHUNK - 1) / DISC_CHUNK;
    const uint64_t ngroups = (nwg + DISC_SCAN_GROUP - 1) / DISC_SCAN_GROUP;
    int rc = grow_ws(ctx, G_DISC_WGS, nwg);
    if (rc) return rc;
    uint64_t *const group_base = ctx->d_wg_base + ctx->disc_wgs + 1;     /* (the layout of d_wg_base: ctx.hpp, WS_DISC_WGS) */
    uint64_t *const group_total = group_base + DISC_GCAP(ctx->disc_wgs);
    /* Round 6: ONE wait per call.  Everything that needs the number of candidates - the probes' launch, the sums, the links,
     * the walk - reads it on the device (ctx->d_walk, DISC_NCAND) and is launched as wide as the candidate arrays are:
     * surplus workgroups leave at once.  Only when there are no arrays yet (the context's first raw stream), or when the
     * stream turns out to hold more candidates than they take (the walk's result says so), does the host wait for the
     * count, make room and go again - what every call did until round 5. */
    for (int attempt = 0; attempt < 2; attempt++) {
        ctx->scounters[7] = (uint64_t)attempt + 1;
        HIP_OK(ctx, hipMemsetAsync(ctx->d_walk, 0, DISC_WORDS * sizeof(uint64_t), s));
        discover_kernel<<<dim3((unsigned)nwg), dim3(DISC_THREADS), 0, s>>>(st, avail, scan_len, max_tree, ctx->d_wg_counts, (DiscSlot *)ctx->d_disc_slots, ctx->d_disc_masks);
        scan_counts_kernel<SCAN_THREADS><<<dim3((unsigned)ngroups), dim3(SCAN_THREADS), 0, s>>>(ctx->d_wg_counts, nwg, ctx->d_wg_base, group_base, group_total, ctx->d_walk, ctx->disc_cands);
        HIP_OK(ctx, hipGetLastError());
        if (ctx->disc_cands == 0 || attempt == 1) {
            HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_walk + DISC_FOUND, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            const uint64_t found = ctx->h_result[0];
            ctx->scounters[1] = found;
            if (found == 0 || found >= 0x7fffffffull) return HUFE_OK;
            rc = grow_ws(ctx, G_DISC_CANDS, found);
            if (rc) return rc;
            /* (the count kernel clamped DISC_NCAND to the capacity it was given: all of them now; h_result[0] is pinned and not
             *  written again before this copy has run - the next one into it is behind it on the stream) */
            HIP_OK(ctx, hipMemcpyAsync(ctx->d_walk + DISC_NCAND, ctx->h_result, sizeof(uint64_t), hipMemcpyHostToDevice, s));
        }
        const uint64_t width = ctx->disc_cands;                          /* launches are as wide as the arrays */
        /* (the candidates' block_len fields pass through d_cand_end, which the probes then overwrite with the ends) */
        place_cands_kernel<<<dim3((unsigned)((nwg + 255) / 256)), dim3(256), 0, s>>>(st, ctx->d_wg_counts, nwg, ctx->d_wg_base, group_base, (const DiscSlot *)ctx->d_disc_slots, ctx->d_disc_masks, ctx->d_cand, ctx->d_cand_end, width);
        cand_lens_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ctx->d_cand_end, ctx->d_walk, ctx->d_spec_off);
        /* (the list of candidates for the exact decoder lives in d_nxt, which link_kernel writes behind the probes; its count in DISC_REDO) */
        probe_kernel<DEC_THREADS><<<dim3((unsigned)width), dim3(DEC_THREADS), 0, s>>>(st, avail, ctx->d_cand, ctx->d_cand_end, ctx->d_cand_status, ctx->d_spec_off, out, out_cap, ctx->d_nxt, ctx->d_walk);
        /* (two forms, each at the lean probe's register budget; the one whose mode it is not leaves at once.  Count-only - every
         *  candidate on the list: hufgpu_block_index - takes a workgroup per candidate) */
        const unsigned exact_grid = (unsigned)(width < 1024 || !out ? width : 1024);
        probe_exact_kernel<DEC_THREADS, true><<<dim3(exact_grid), dim3(DEC_THREADS), 0, s>>>(st, avail, ctx->d_cand, ctx->d_cand_end, ctx->d_cand_status, ctx->d_spec_off, out, out_cap, ctx->d_nxt, ctx->d_walk);
        probe_exact_kernel<DEC_THREADS, false><<<dim3(exact_grid), dim3(DEC_THREADS), 0, s>>>(st, avail, ctx->d_cand, ctx->d_cand_end, ctx->d_cand_status, ctx->d_spec_off, out, out_cap, ctx->d_nxt, ctx->d_walk);
        link_kernel<<<dim3((unsigned)((width + 255) / 256)), dim3(256), 0, s>>>(ctx->d_cand, ctx->d_cand_end, ctx->d_cand_status, ctx->d_walk, length, ctx->d_nxt);
        walk_kernel<<<dim3(1), dim3(WALK_THREADS), 0, s>>>(ctx->d_cand, ctx->d_cand_end, ctx->d_nxt, ctx->d_chain, ctx->d_walk, ctx->d_spec_off, out_cap);
        HIP_OK(ctx, hipGetLastError());
        static_assert(DISC_NCAND < 10 && DISC_ODD_LINKS < 10 && DISC_REDO < 10, "the copy below brings the read-out's words");
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_walk, 10 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        ctx->scounters[1] = ctx->h_result[DISC_FOUND];
        ctx->scounters[2] = ctx->h_result[DISC_NCAND];
        ctx->scounters[3] = ctx->h_result[DISC_REDO];
        ctx->scounters[4] = ctx->h_result[DISC_ODD_LINKS];
        ctx->scounters[5] = ctx->h_result[0];
        ctx->scounters[6] = ctx->h_result[0] ? ctx->h_result[4] : ~0ull;     /* (no block validated: nothing counts as in place) */
        if (ctx->h_result[DISC_FOUND] > width) continue;                 /* more candidates than the arrays took: once more, with room */
        *m_out = ctx->h_result[0];
        *in_place_out = ctx->h_result[4];   /* bytes the probe already decoded into `out` for these m blocks */
        *complete_out = ctx->h_result[2] != 0;
        *resume_out = *complete_out ? ctx->h_result[3] : ctx->h_result[1];
        return HUFE_OK;
    }
    return HUFE_OK;
}

/* Leading blocks of HUF_BIG_BLOCK symbols and more (blocksize = 0 makes the whole input ONE block,
 * src/encoder.c:163-165): one workgroup per block would leave the device idle, so a sub-index is
 * built for each such block (kernels/spec_index.hpp) and decode_sub_kernel decodes - and verifies -
 * it chunk by chunk.  Stops at the first block this does not apply to or does not work for; the
 * caller's general path takes over at *pos / *rawpos and reports whatever is wrong there. */
static int decode_big_blocks(hufgpu_ctx *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint8_t *out,
                             uint64_t out_cap, uint32_t flags, hipStream_t s, void *stream, uint64_t *pos_io,
                             uint64_t *rawpos_io)
{
    const int max_tree = max_tree_of(flags);
    uint64_t pos = *pos_io, rawpos = *rawpos_io;
    unsigned long long *d_status = (unsigned long long *)ctx->d_big_offs;
    uint64_t *d_offs = ctx->d_big_offs + SPEC_WORDS;
    while (pos < length && avail - pos >= HUF_HEADER_FIXED) {
        spec_head_kernel<<<dim3(1), dim3(64), 0, s>>>(st, avail, pos, d_status);
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, d_status, SPEC_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        const uint64_t block_len = ctx->h_result[SPEC_BLOCK_LEN];
        const long long tl = (long long)ctx->h_result[SPEC_TREE_LEN];
        const long long leaf = (long long)ctx->h_result[SPEC_LEAF];
        if (ctx->h_result[SPEC_FAIL] || block_len < HUF_BIG_BLOCK || block_len > HUFGPU_MAX_BLOCK) break;
        if (tl < 1 || tl > max_tree || block_len > out_cap - rawpos) break;
        const uint64_t pay_off = pos + HUF_HEADER_FIXED + 2ull * (uint64_t)tl;
        if (pay_off > avail) break;
        const uint64_t pay_bytes = avail - pay_off;

        const uint64_t sub_bytes = hufgpu_sub_index_bytes(block_len, block_len);
        /* (workspace that cannot be had - a block of many GiB needs a quarter of its size - is no
         * error: the general path takes the block) */
        if (grow_ws(ctx, G_BIG_SUB, sub_bytes)) break;
        const HufSubIndex sub = sub_index_view(ctx->d_big_sub, block_len, block_len);
        uint64_t o1;
        if (leaf >= 0) {
            /* one 0 bit per symbol: nothing to find out */
            o1 = pay_off + ((block_len + 7) >> 3);
            if (o1 > avail) break;
            const uint64_t h_offs[2] = {pos, o1};
            HIP_OK(ctx, hipMemcpyAsync(d_offs, h_offs, sizeof(h_offs), hipMemcpyHostToDevice, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
        } else {
            /* an encoder-made payload has at most 9 bits per symbol (8 + the wrap root's) */
            uint64_t max_bits = pay_bytes * 8;
            if (max_bits > 9 * block_len + 64) max_bits = 9 * block_len + 64;
            const uint64_t nlanes = (max_bits + SPEC_LANE_BITS - 1) / SPEC_LANE_BITS;
            if (nlanes == 0) break;
            if (grow_ws(ctx, G_BIG_LANES, nlanes)) break;
            SpecJob j;
            j.tree = st + pos + HUF_HEADER_FIXED;
            j.tree_len = (int)tl;
            j.pay = st + pay_off;
            j.pay_bytes = pay_bytes;
            j.max_bits = max_bits;
            j.block_len = block_len;
            j.nlanes = nlanes;
            j.entry = ctx->d_big_entry;
            j.exitp = ctx->d_big_exit;
            j.cnt = ctx->d_big_cnt;
            j.pre = ctx->d_big_pre;
            j.wg_pre = ctx->d_big_wgpre;
            j.first_pos = ctx->d_big_first_pos;
            j.first_g = ctx->d_big_first_g;
            j.last_pos = ctx->d_big_last_pos;
            j.status = d_status;
            const unsigned lane_wgs = (unsigned)((nlanes + DEC_THREADS - 1) / DEC_THREADS);
            spec_scan_kernel<DEC_THREADS><<<dim3(lane_wgs), dim3(DEC_THREADS), 0, s>>>(j, sub.lens);
            bool chain_ok = false;
            for (int attempt = 0; attempt < 2; attempt++) {
                spec_prefix_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(j, (uint64_t)lane_wgs, ctx->d_big_wgscratch);
                spec_mark_kernel<DEC_THREADS><<<dim3(lane_wgs), dim3(DEC_THREADS), 0, s>>>(j, sub);
                spec_groups_kernel<<<dim3((unsigned)((nlanes + 8 + 255) / 256)), dim3(256), 0, s>>>(j, sub, pos, pay_off, d_offs);
                HIP_OK(ctx, hipGetLastError());
                HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, d_status, SPEC_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                HIP_OK(ctx, hipStreamSynchronize(s));
                if (getenv("HUF_GPU_TRACE"))
                    fprintf(stderr, "big block at %llu: attempt %d chain %llu fail %llu found %llu end_bits %llu lanes %llu\n", (unsigned long long)pos, attempt,
                            (unsigned long long)ctx->h_result[SPEC_CHAIN], (unsigned long long)ctx->h_result[SPEC_FAIL],
                            (unsigned long long)ctx->h_result[SPEC_FOUND], (unsigned long long)ctx->h_result[SPEC_END_BITS], (unsigned long long)nlanes);
                if (!ctx->h_result[SPEC_CHAIN] || ctx->h_result[SPEC_FAIL] || attempt == 1) {
                    chain_ok = !ctx->h_result[SPEC_CHAIN] && !ctx->h_result[SPEC_SHORT];
                    break;
                }
                /* some share did not fall into step before its first bit (a run of one byte value is
                 * a periodic bit string: a decoder can lock onto it one bit off): mend the chain, one
                 * share further per round, then sum and mark again.  A run of more than
                 * SPEC_REPAIR_ROUNDS shares (512 KiB of payload) is left to the general path. */
                bool mended = false;
                for (int round = 0; round < SPEC_REPAIR_ROUNDS && !mended; round += SPEC_REPAIR_BATCH) {
                    HIP_OK(ctx, hipMemsetAsync(d_status + SPEC_REPAIRED, 0, sizeof(uint64_t), s));
                    for (int k = 0; k < SPEC_REPAIR_BATCH; k++)      /* (a round that finds nothing to mend costs a few microseconds) */
                        spec_repair_kernel<DEC_THREADS><<<dim3(lane_wgs), dim3(DEC_THREADS), 0, s>>>(j);
                    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + SPEC_REPAIRED, d_status + SPEC_REPAIRED, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                    HIP_OK(ctx, hipStreamSynchronize(s));
                    mended = ctx->h_result[SPEC_REPAIRED] == 0;
                    if (getenv("HUF_GPU_TRACE")) fprintf(stderr, "  repair rounds %d..: %llu shares\n", round, (unsigned long long)ctx->h_result[SPEC_REPAIRED]);
                }
                if (!mended) break;
                HIP_OK(ctx, hipMemsetAsync(d_status + SPEC_CHAIN, 0, sizeof(uint64_t), s));
                HIP_OK(ctx, hipMemsetAsync(d_status + SPEC_SHORT, 0, sizeof(uint64_t), s));
                HIP_OK(ctx, hipMemsetAsync(d_status + SPEC_FOUND, 0, sizeof(uint64_t), s));
                spec_sum_kernel<DEC_THREADS><<<dim3(lane_wgs), dim3(DEC_THREADS), 0, s>>>(j);
            }
            if (!chain_ok) break;
            if (ctx->h_result[SPEC_FAIL] || !ctx->h_result[SPEC_FOUND]) break;
            o1 = pay_off + ((ctx->h_result[SPEC_END_BITS] + 7) >> 3);
            if (o1 > avail) break;
        }
        uint64_t got = 0;
        const int err = decode_impl(ctx, st, o1, d_offs, 1, &sub, block_len, out + rawpos, out_cap - rawpos, flags, &got, stream);
        if (getenv("HUF_GPU_TRACE")) {
            uint32_t nfix = 0;
            (void)hipMemcpy(&nfix, ctx->d_fix_count, sizeof(nfix), hipMemcpyDeviceToHost);
            fprintf(stderr, "big block at %llu: decode err %d, %llu bytes, blocks decoded again without the sub-index: %u\n", (unsigned long long)pos, err,
                    (unsigned long long)got, nfix);
        }
        if (err != HUFE_OK || got != block_len) break;   /* the general path decodes it again and says what is wrong */
        pos = o1;
        rawpos += block_len;
    }
    *pos_io = pos;
    *rawpos_io = rawpos;
    return HUFE_OK;
}

/* The block index of a raw stream without decoding it into anything: see include/huffman_gpu.h. */
extern "C" int hufgpu_block_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length, uint32_t flags,
                                  const uint64_t **d_index, uint64_t *nblocks, uint64_t *consumed, void *stream)
{
    if (!ctx || !d_index || !nblocks || !consumed) return HUFE_ARGUMENT;
    *d_index = NULL; *nblocks = 0; *consumed = 0;
    memset(ctx->scounters, 0, sizeof(ctx->scounters));
    if (length == 0) return HUFE_OK;
    if (!d_stream || ((uintptr_t)d_stream & 15u)) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int max_tree = max_tree_of(flags);
    const uint64_t scan_len = length < avail ? length : avail;
    if (scan_len < 4096) return HUFE_OK;
    uint64_t m = 0, resume = 0, in_place = ~0ull;
    bool complete = false;
    const int rc = discover_chain(ctx, (const uint8_t *)d_stream, avail, length, scan_len, max_tree, NULL, 0, s, &m, &resume,
                                  &complete, &in_place);
    if (rc != HUFE_OK) return rc;
    if (m == 0) return HUFE_OK;
    *d_index = ctx->d_chain;
    *nblocks = m;
    *consumed = resume;
    return HUFE_OK;
}

static int decode_stream_general(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                                 void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                                 uint64_t *consumed, void *stream)
{
    hipStream_t s = pick_stream(ctx, stream);
    const int max_tree = max_tree_of(flags);
    const uint8_t *st = (const uint8_t *)d_stream;
    uint8_t *out = (uint8_t *)d_out;
    uint64_t raw = 0, used = 0;
    int err = HUFE_OK;
    ctx->complete_used = 0;              /* also what an early return (a failed HIP call) leaves behind */
    ctx->complete_raw = 0;

    /* ---- parallel path: discover the block chain, decode the validated prefix ---- */
    uint64_t prefix_raw = 0, resume = 0;
    bool complete = false;
    const uint64_t scan_len = length < avail ? length : avail;
    /* (below 64 KiB of stream the in-order chain is the faster of the two: one launch, 50-60 us a call where the discovery's
     *  launches and its two host round trips take 100-130 - tools/time_stream_small.py) */
    const bool try_parallel = (((uintptr_t)st & 15u) == 0) && scan_len >= 65536 && !(flags & HUFGPU_SEQUENTIAL);
    if (try_parallel) {
        uint64_t m = 0, in_place = ~0ull;
        const int drc = discover_chain(ctx, st, avail, length, scan_len, max_tree, out, out_cap, s, &m, &resume, &complete, &in_place);
        if (drc != HUFE_OK) return drc;
        {
            if (m > 0 && in_place != ~0ull) {
                prefix_raw = in_place;                 /* every candidate was a block: nothing to decode again */
            } else if (m > 0) {
                ctx->last_failing = ~0ull;
                err = hufgpu_decode(ctx, st, resume, ctx->d_chain, m, out, out_cap, flags, &prefix_raw, stream);
                if (err == HUFE_MEMORY && ctx->last_failing < m) {
                    /* the block that does not fit (hufgpu_decode_result) and what follows go to the in-order decoder, which
                     * delivers what fits of it, as src/decoder.c does - not just the whole blocks in front of it */
                    HIP_OK(ctx, hipMemcpyAsync(&resume, ctx->d_chain + ctx->last_failing, sizeof(resume), hipMemcpyDeviceToHost, s));
                    HIP_OK(ctx, hipStreamSynchronize(s));
                    complete = false;
                    err = HUFE_OK;
                } else if (err != HUFE_OK) {           /* cannot happen for probed blocks except for lack of room */
                    prefix_raw = 0; resume = 0; complete = false;   /* start over, sequentially */
                }
            } else {
                resume = 0; complete = false;
            }
        }
    }
    ctx->complete_used = 0;
    ctx->complete_raw = 0;
    if (complete) {
        raw = prefix_raw;
        used = resume;
        err = HUFE_OK;
        ctx->complete_used = used;
        ctx->complete_raw = raw;
    } else {
        /* ---- exact sequential decoder for what is left (all of it when nothing was validated) ---- */
        uint64_t raw2 = 0, used2 = 0;
        STAGE_BEGIN(ctx, s, PROF_DECODE);
        uint64_t good_used = 0, good_raw = 0;
        err = decode_chain(ctx, st + resume, avail - resume, length - resume, out + prefix_raw,
                           out_cap - prefix_raw, max_tree, s, &raw2, &used2, &good_used, &good_raw);
        STAGE_MARK(ctx, s);
        raw = prefix_raw + raw2;
        used = resume + used2;
        ctx->complete_used = resume + good_used;
        ctx->complete_raw = prefix_raw + good_raw;
    }
    if (raw_len) *raw_len = raw;
    if (consumed) *consumed = used;
    if (err == HUFE_ARGUMENT) set_err(ctx, "a block is longer than the kernels support");
    if (err == HUFE_MEMORY) set_err(ctx, "output buffer too small");
    return err;
}

extern "C" int hufgpu_decode_stream(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                                    void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                                    uint64_t *consumed, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (raw_len) *raw_len = 0;
    if (consumed) *consumed = 0;
    memset(ctx->scounters, 0, sizeof(ctx->scounters));
    if (length == 0) return HUFE_OK;                  /* src/decoder.c:218 */
    if ((!d_stream && avail) || (!d_out && out_cap)) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    uint64_t pos = 0, rawpos = 0;
    if (!(flags & HUFGPU_SEQUENTIAL) && avail >= HUF_BIG_BLOCK / 8) {
        const int rc = decode_big_blocks(ctx, (const uint8_t *)d_stream, avail, length, (uint8_t *)d_out, out_cap, flags,
                                         pick_stream(ctx, stream), stream, &pos, &rawpos);
        if (rc != HUFE_OK) return rc;
    }
    ctx->complete_used = pos;
    ctx->complete_raw = rawpos;
    if (pos >= length) {
        if (raw_len) *raw_len = rawpos;
        if (consumed) *consumed = pos;
        return HUFE_OK;
    }
    uint64_t raw2 = 0, used2 = 0;
    const int err = decode_stream_general(ctx, (const uint8_t *)d_stream + pos, avail - pos, length - pos,
                                          (uint8_t *)d_out + rawpos, out_cap - rawpos, flags, &raw2, &used2, stream);
    /* the general path reports ITS complete blocks (0 / 0 when it returned before decoding anything): the
     * totals are formed here, in one place */
    ctx->complete_used = pos + ctx->complete_used;
    ctx->complete_raw = rawpos + ctx->complete_raw;
    if (raw_len) *raw_len = rawpos + raw2;
    if (consumed) *consumed = pos + used2;
    return err;
}

/* What the discovery of the last hufgpu_decode_stream / hufgpu_block_index did (include/huffman_gpu.h): host values that
 * discover_chain took from its last copy of d_walk, no GPU is touched. */
extern "C" int hufgpu_stream_counters(hufgpu_ctx_t *ctx, uint64_t counters[8])
{
    if (!ctx || !counters) return HUFE_ARGUMENT;
    memcpy(counters, ctx->scounters, sizeof(ctx->scounters));
    return HUFE_OK;
}

extern "C" int hufgpu_decode_stream_complete(hufgpu_ctx_t *ctx, uint64_t *raw_len, uint64_t *consumed)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (raw_len) *raw_len = ctx->complete_raw;
    if (consumed) *consumed = ctx->complete_used;
    return HUFE_OK;
}

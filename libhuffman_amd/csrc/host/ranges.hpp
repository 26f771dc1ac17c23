/* ranges.hpp - hufgpu_decode_ranges: byte ranges of the original data out of one indexed stream (include/huffman_gpu.h,
   kernels/ranges.hpp, kernels/range_tiles.hpp), and the DecRangeArgs fields it shares with hufgpu_update_ranges.
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

/* How the last hufgpu_decode_ranges routed its blocks (include/huffman_gpu.h): host values, no GPU is touched. */
extern "C" int hufgpu_ranges_counters(hufgpu_ctx_t *ctx, uint64_t counters[8])
{
    if (!ctx || !counters) return HUFE_ARGUMENT;
    memcpy(counters, ctx->rcounters, sizeof(ctx->rcounters));
    return HUFE_OK;
}

/* What hufgpu_decode_ranges and hufgpu_update_ranges fill alike in a zeroed DecRangeArgs: the ranges' tables at the
 * front of the staging area (range_lo, range_hi, out_offsets), the blocks as decode_prepare_kernel left them, and the
 * plan's workspace.  Returns the y extent of drange_mark_kernel's grid - a few long ranges: several workgroups a range
 * walk its blocks; many ranges are parallel enough as they are. */
static unsigned fill_range_args(hufgpu_ctx *ctx, DecRangeArgs &ra, uint64_t nranges, uint64_t nb, const TwoLevel &lens)
{
    ra.range_lo = ctx->d_bstage;
    ra.range_hi = ctx->d_bstage + nranges;
    ra.out_offsets = ctx->d_bstage + 2 * nranges;
    ra.nranges = nranges;
    ra.nblocks = nb;
    ra.dmeta = ctx->d_dmeta;
    ra.status = ctx->d_status;
    ra.lens = lens;
    ra.first_bad = (unsigned long long *)ctx->d_result + 2;
    ra.bprefix = ctx->d_bprefix;
    ra.obase = ctx->d_bobase;
    ra.cover = ctx->d_rcover;
    ra.rel = ctx->d_rrel;
    ra.kind = ctx->d_blk_item;
    ra.rplan = ctx->d_rplan;
    ra.rflag = ctx->d_rflag;
    ra.counters = ctx->d_rcounters;
    return nranges >= 64 ? 1u : (unsigned)(nb / 2048 < 1 ? 1 : (nb / 2048 > 16 ? 16 : nb / 2048));
}

extern "C" int hufgpu_decode_ranges(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                    const uint64_t *d_block_offsets, uint64_t nblocks, uint64_t nranges,
                                    const uint64_t *range_lo, const uint64_t *range_hi, const uint64_t *out_offsets,
                                    const void *d_sub_index, uint64_t raw_size, uint64_t blocksize, void *d_out,
                                    uint32_t flags, int32_t *range_errs, uint64_t *range_raw_lens, void *stream)
{
    if (nranges == 0) return HUFE_OK;
    if (!range_lo || !range_hi || !out_offsets || !range_errs || !range_raw_lens || nranges > 0x7fffffffull) {
        set_err(ctx, "decode_ranges: range_lo, range_hi, out_offsets, range_errs and range_raw_lens are required (at most 2^31 - 1 ranges)");
        return HUFE_ARGUMENT;
    }
    for (uint64_t i = 0; i < nranges; i++) {
        if (range_lo[i] > range_hi[i]) {
            set_err(ctx, "decode_ranges: range %llu ends in front of its start", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
        if (out_offsets[i + 1] < out_offsets[i]) {
            set_err(ctx, "decode_ranges: out_offsets must not decrease (range %llu)", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
    }
    if (d_sub_index) {
        if (blocksize == 0) blocksize = raw_size;
        const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
        if (((uintptr_t)d_sub_index & 7u) || raw_size == 0 || hufgpu_block_count(raw_size, blocksize) != nblocks ||
            nblocks * cpb > 0x7fffffffull) {
            set_err(ctx, "decode_ranges: a sub-index needs an 8-byte aligned buffer and the (raw_size, blocksize) of the encode that wrote these %llu blocks",
                    (unsigned long long)nblocks);
            return HUFE_ARGUMENT;
        }
    }
    if (!ctx) {
        set_err(NULL, "decode_ranges: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    const uint64_t nb = nblocks;
    const uint64_t out_end = out_offsets[nranges];
    if (nb > 0x7fffffffull || (nb && stream_len && (!d_stream || !d_block_offsets)) || (!d_out && out_end > out_offsets[0])) {
        set_err(ctx, "decode_ranges: the stream, its block index or the output is missing, or more than 2^31 - 1 blocks");
        return HUFE_ARGUMENT;
    }
    for (uint64_t i = 0; i < nranges; i++) { range_errs[i] = HUFE_OK; range_raw_lens[i] = 0; }
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    memset(ctx->rcounters, 0, sizeof(ctx->rcounters));
    if (nb == 0 || stream_len == 0) return HUFE_OK;     /* no data (src/decoder.c:218): every range lies behind its end */
    /* the tile route (kernels/range_tiles.hpp): the caller vouches for the sub-index */
    const bool tiles = (flags & HUFGPU_RANGES_TILES) != 0u && d_sub_index != NULL;

    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    ctx->last_stream = s;
    int rc = ensure_decode_ws(ctx, nb);
    if (rc) return rc;
    rc = ensure_batch_ws(ctx, nb, nranges);
    if (rc) return rc;
    rc = ensure_range_ws(ctx, nb, nranges);
    if (rc) return rc;
    uint64_t *h = NULL;
    rc = batch_stage(ctx, 3 * nranges + 1, &h);
    if (rc) return rc;
    memcpy(h, range_lo, nranges * sizeof(uint64_t));
    memcpy(h + nranges, range_hi, nranges * sizeof(uint64_t));
    memcpy(h + 2 * nranges, out_offsets, (nranges + 1) * sizeof(uint64_t));
    rc = batch_upload(ctx, 3 * nranges + 1, s);
    if (rc) return rc;

    const int max_tree = max_tree_of(flags);
    const uint8_t *st = (const uint8_t *)d_stream;
    const TwoLevel lens = decode_lens(ctx, nb);
    launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nb, max_tree, lens, s);

    DecRangeArgs ra;
    memset(&ra, 0, sizeof(ra));
    const unsigned mark_y = fill_range_args(ctx, ra, nranges, nb, lens);
    ra.range_fail = ctx->d_item_fail;
    ra.range_res = ctx->d_item_res;
    ra.dout = (uint8_t *)d_out;
    if (tiles) {
        ra.tpairs = ctx->d_rtpairs;
        ra.raw_size = raw_size;
        ra.blocksize = blocksize;
    }
    drange_plan_kernel<<<dim3(grid256((nb + 1 > nranges ? nb + 1 : nranges))), dim3(256), 0, s>>>(ra);
    drange_mark_kernel<<<dim3((unsigned)nranges, mark_y), dim3(256), 0, s>>>(ra);
    drange_class_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ra);
    HIP_OK(ctx, hipGetLastError());
    /* how many blocks are staged and how long the longest of them is decides the scratch area: the one wait in front of the decoders */
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_rcounters, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const uint64_t nstaged = ctx->h_result[8], longest = ctx->h_result[9];
    const uint64_t ndirect = ctx->h_result[11], ntiled = ctx->h_result[12], nitems = ctx->h_result[13];
    ctx->rcounters[0] = ndirect;
    ctx->rcounters[1] = nstaged;
    ctx->rcounters[2] = ntiled;
    ctx->rcounters[3] = nitems;
    const uint64_t stride = (longest + 15u) & ~15ull;
    uint64_t scratch_bytes = 0;
    if (nstaged) {
        if (__builtin_mul_overflow(nstaged, stride, &scratch_bytes) || scratch_bytes > ((uint64_t)1 << 46)) scratch_bytes = ~0ull;
        const int rcs = grow_range_scratch(ctx, scratch_bytes);
        if (rcs == HUFE_MEMORY) {
            set_err(ctx, "decode_ranges: no room for %llu staged blocks of up to %llu bytes", (unsigned long long)nstaged,
                    (unsigned long long)longest);
            for (uint64_t i = 0; i < nranges; i++) range_errs[i] = HUFE_MEMORY;
        }
        if (rcs) return rcs;
    }
    /* The decoders write at one base + a 64-bit offset and check offset + block_len against out_cap.  Two destinations
     * without touching them: the base is the lower of d_out and the scratch area, the offsets count from it, out_cap is
     * the span of both; the slot checks were made by drange_plan_kernel, and a staged block has `stride` bytes. */
    uint8_t *base = (uint8_t *)d_out;
    uint64_t span = out_end;
    if (nstaged) {
        uint8_t *scr = ctx->d_rscratch;
        if (!base || (uintptr_t)scr < (uintptr_t)base) base = scr;
        ra.dout_off = d_out ? (uint64_t)((uintptr_t)d_out - (uintptr_t)base) : 0;
        ra.scratch_off = (uint64_t)((uintptr_t)scr - (uintptr_t)base);
        ra.stride = stride;
        ra.scratch = scr;
        const uint64_t e0 = ra.dout_off + out_end, e1 = ra.scratch_off + scratch_bytes;
        span = e0 > e1 ? e0 : e1;
    }
    drange_place_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ra);

    /* the decoders read a block's output base as gprefix[blk / SCAN_GROUP] + local[blk]: zeros + the planned offsets */
    TwoLevel blens = lens;
    blens.gprefix = ctx->d_bzero;
    blens.local = ctx->d_bobase;
    const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
    if (ntiled) {
        /* one wave an item; a workgroup's eight waves take about four items each of a long range, so that the table build
         * it starts with is paid once per 32 tiles - the longest range, known here, bounds the tiles a range has in a block */
        uint64_t longest_range = 0;
        for (uint64_t i = 0; i < nranges; i++)
            if (range_hi[i] - range_lo[i] > longest_range) longest_range = range_hi[i] - range_lo[i];
        uint64_t tile_y = (longest_range / HUF_SUB_TILE + 2 + 31) / 32;
        if (tile_y > 1024) tile_y = 1024;
        const SubStream ta = sub_stream_args(st, stream_len, d_block_offsets, nb, d_sub_index, raw_size, blocksize, flags);
        drange_tiles_kernel<<<dim3((unsigned)nranges, (unsigned)tile_y), dim3(RTILE_THREADS), 0, s>>>(ra, ta);
    }
    /* (every touched block served by tiles: nothing for the block decoders to do) */
    if (!(ntiled && nstaged == 0 && ndirect == 0)) {
        const IndexedDecode job = {st, stream_len, d_block_offsets, nb, blens, base, span, &sub, blocksize};
        rc = launch_indexed_decoders(ctx, job, s);
        if (rc) return rc;
    }
    drange_result_kernel<<<dim3((unsigned)nranges), dim3(256), 0, s>>>(ra);
    if (nstaged) {
        const unsigned gather_y = nranges >= 1024 ? 2u : (nranges >= 64 ? 4u : 16u);
        drange_gather_kernel<<<dim3((unsigned)nranges, gather_y), dim3(256), 0, s>>>(ra);
    }
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_item_res, ctx->d_item_res, 3 * nranges * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (ntiled) HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 14, ctx->d_rcounters + 6, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    if (ntiled && ctx->h_result[14] != 0) {
        /* A tile-routed block failed a check (a sub-index that is not the stream's, damage in a touched tile or in the
         * tree): the call once more by the staged route, which verifies everything and produces the reference's errors
         * and partial deliveries - the slots are simply written again.  Of the counters, the blocks are then those of
         * that call (none is served by tiles); the items and the failed blocks are this one's. */
        const uint64_t nfailed = ctx->h_result[14];
        const int rc2 = hufgpu_decode_ranges(ctx, d_stream, stream_len, d_block_offsets, nblocks, nranges, range_lo, range_hi, out_offsets,
                                             d_sub_index, raw_size, blocksize, d_out, flags & ~HUFGPU_RANGES_TILES, range_errs,
                                             range_raw_lens, stream);
        ctx->rcounters[3] = nitems;
        ctx->rcounters[4] = nfailed;
        return rc2;
    }

    int first_err = HUFE_OK;
    uint64_t first_range = 0;
    for (uint64_t i = 0; i < nranges; i++) {
        const uint64_t *r = ctx->h_item_res + 3 * i;
        const int err = (int)(int32_t)r[0];
        uint64_t raw = r[1];
        const uint64_t f = r[2];
        if ((err == HUFE_RW || err == HUFE_CORRUPTED) && f < nb) {
            /* what hufgpu_decode_result() does: the failing block once more, in order, its record as the whole input
             * (src/decoder.c:69-91), into the place the block was decoded to - its own part of the slot when it is direct,
             * its scratch entry when it is staged; of a staged block the delivered bytes inside the range are copied on */
            uint64_t o[2] = {0, 0}, rel = 0, p0 = 0, plan[2] = {0, 0};
            uint32_t kind = DRANGE_UNTOUCHED;
            HufDecodeMeta m;
            memset(&m, 0, sizeof(m));
            HIP_OK(ctx, hipMemcpyAsync(o, d_block_offsets + f, sizeof(o), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(&rel, ctx->d_rrel + f, sizeof(rel), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(&p0, ctx->d_bprefix + f, sizeof(p0), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(&kind, ctx->d_blk_item + f, sizeof(kind), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(&m, ctx->d_dmeta + f, sizeof(m), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(plan, ctx->d_rplan + 4 * i, sizeof(plan), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            if (o[1] > stream_len) o[1] = stream_len;
            uint8_t *dst = kind == DRANGE_DIRECT ? (uint8_t *)d_out + rel : (kind == DRANGE_STAGED ? ctx->d_rscratch + rel * stride : NULL);
            if (o[0] < o[1] && dst) {
                uint64_t got = 0, used = 0, gu = 0, gr = 0;
                const int rc2 = decode_chain(ctx, st + o[0], o[1] - o[0], 1, dst, m.block_len, max_tree, s, &got, &used, &gu, &gr);
                if (rc2 == err) {
                    const uint64_t c0 = plan[0] > p0 ? plan[0] : p0;
                    const uint64_t c1 = plan[1] < p0 + got ? plan[1] : p0 + got;
                    if (c1 > c0) {
                        if (kind == DRANGE_STAGED) {
                            HIP_OK(ctx, hipMemcpyAsync((uint8_t *)d_out + out_offsets[i] + (c0 - plan[0]), dst + (c0 - p0), c1 - c0, hipMemcpyDeviceToDevice, s));
                            HIP_OK(ctx, hipStreamSynchronize(s));
                        }
                        raw = c1 - plan[0];
                    }
                }
            }
        }
        range_errs[i] = err;
        range_raw_lens[i] = raw;
        if (err != HUFE_OK && first_err == HUFE_OK) {
            first_err = err;
            first_range = i;
        }
    }
    if (first_err != HUFE_OK)
        set_err(ctx, "decode_ranges: range %llu failed with error %d (%llu ranges in all)", (unsigned long long)first_range, first_err,
                (unsigned long long)nranges);
    return first_err;
}

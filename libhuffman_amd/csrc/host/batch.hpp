/* batch.hpp - hufgpu_encode_batch / hufgpu_decode_batch: many independent inputs in one launch sequence
   (include/huffman_gpu.h, kernels/batch.hpp), the row layout of a batch's sub-index, and the pinned staging area that
   the host tables of these and of the range calls go up through.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

static_assert(HUFGPU_BATCH_CHUNKED_FROM == HUF_CHUNKED_FROM, "include/huffman_gpu.h states the chunked threshold");

static uint64_t sub_rows_bytes(uint64_t nb, uint64_t row_blocksize)
{
    if (nb == 0) return 0;
    const uint64_t gpb = ((row_blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;
    const uint64_t tpb = (row_blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    return nb * tpb * sizeof(uint64_t) + nb * gpb * sizeof(uint16_t) + nb * HUF_NSYM;
}

/* the sub-index of a batch: hufgpu_encode_sub's three arrays, one row per block of row_blocksize symbols */
static HufSubIndex sub_index_rows(void *d_sub, uint64_t nb, uint64_t row_blocksize)
{
    HufSubIndex v;
    memset(&v, 0, sizeof(v));
    if (!d_sub || nb == 0) return v;
    v.gpb = ((row_blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;
    v.tpb = (row_blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    v.tile_bits = (uint64_t *)d_sub;
    v.group_bits = (uint16_t *)((uint64_t *)d_sub + nb * v.tpb);
    v.lens = (uint8_t *)(v.group_bits + nb * v.gpb);
    return v;
}

extern "C" int hufgpu_batch_geometry(uint64_t nitems, const uint64_t *item_lens, uint64_t blocksize, uint64_t *nblocks,
                                     uint64_t *row_blocksize, uint64_t *out_bound, uint64_t *sub_index_bytes)
{
    if (nitems && !item_lens) return HUFE_ARGUMENT;
    uint64_t nb = 0, longest = 0, bound = 0;
    for (uint64_t i = 0; i < nitems; i++) {
        nb += hufgpu_block_count(item_lens[i], blocksize);
        bound += hufgpu_encode_bound(item_lens[i], blocksize);
        if (item_lens[i] > longest) longest = item_lens[i];
    }
    const uint64_t rbs = (blocksize && blocksize < longest) ? blocksize : longest;
    if (nblocks) *nblocks = nb;
    if (row_blocksize) *row_blocksize = rbs;
    if (out_bound) *out_bound = bound;
    if (sub_index_bytes) *sub_index_bytes = sub_rows_bytes(nb, rbs);
    return HUFE_OK;
}

/* `words` words of the pinned staging area, once the copy of the previous call has left it */
static int batch_stage(hufgpu_ctx *c, uint64_t words, uint64_t **h)
{
    if (!c->bstage_ev) HIP_OK(c, hipEventCreateWithFlags(&c->bstage_ev, hipEventDisableTiming));
    if (c->bstage_pending) HIP_OK(c, hipEventSynchronize(c->bstage_ev));
    c->bstage_pending = 0;
    const int rc = grow_ws(c, G_BSTAGE, words);
    *h = c->h_bstage;
    return rc;
}

static int batch_upload(hufgpu_ctx *c, uint64_t words, hipStream_t s)
{
    HIP_OK(c, hipMemcpyAsync(c->d_bstage, c->h_bstage, words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_OK(c, hipEventRecord(c->bstage_ev, s));
    c->bstage_pending = 1;
    return HUFE_OK;
}

extern "C" int hufgpu_encode_batch(hufgpu_ctx_t *ctx, const void *d_in, uint64_t nitems, const uint64_t *item_lens,
                                   uint64_t blocksize, void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                                   uint64_t *d_item_offsets, void *d_sub_index, uint64_t *item_offsets, void *stream)
{
    if (!ctx || (nitems && !item_lens)) return HUFE_ARGUMENT;
    uint64_t nb = 0, rbs = 0, bound = 0, total_in = 0;
    (void)hufgpu_batch_geometry(nitems, item_lens, blocksize, &nb, &rbs, &bound, NULL);
    for (uint64_t i = 0; i < nitems; i++) total_in += item_lens[i];
    if ((total_in && !d_in) || !d_out || out_cap < bound) {
        set_err(ctx, "encode_batch: input / output missing or output capacity %llu below the batch bound %llu",
                (unsigned long long)out_cap, (unsigned long long)bound);
        return HUFE_ARGUMENT;
    }
    if (blocksize > HUFGPU_MAX_BLOCK || rbs > HUFGPU_MAX_BLOCK || nb > 0x7fffffffull || nitems > 0xffffffffull) {
        set_err(ctx, "encode_batch: blocks of %llu bytes or %llu blocks exceed the kernel limits", (unsigned long long)rbs,
                (unsigned long long)nb);
        return HUFE_ARGUMENT;
    }
    if (d_sub_index && (rbs >= HUF_CHUNKED_FROM || ((uintptr_t)d_sub_index & 7u))) {
        set_err(ctx, "encode_batch: a sub-index needs an 8-byte aligned buffer and blocks below %llu bytes",
                (unsigned long long)HUF_CHUNKED_FROM);
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    int rc = ensure_encode_ws(ctx, nb > 0 ? nb : 1);
    if (rc) return rc;
    rc = ensure_batch_ws(ctx, nb, nitems);
    if (rc) return rc;
    uint64_t *offs = d_block_offsets ? d_block_offsets : ctx->d_offsets;
    const uint8_t *in = (const uint8_t *)d_in;

    /* the table of block starts, then item_blocks */
    uint64_t *h = NULL;
    rc = batch_stage(ctx, nb + 1 + nitems + 1, &h);
    if (rc) return rc;
    uint64_t *h_starts = h, *h_ib = h + nb + 1;
    {
        uint64_t b = 0, pos = 0;
        for (uint64_t i = 0; i < nitems; i++) {
            h_ib[i] = b;
            const uint64_t len = item_lens[i], bs = blocksize ? blocksize : len;
            for (uint64_t o = 0; o < len; o += bs) h_starts[b++] = pos + o;
            pos += len;
        }
        h_ib[nitems] = b;
        h_starts[nb] = pos;
    }
    rc = batch_upload(ctx, nb + 1 + nitems + 1, s);
    if (rc) return rc;
    const uint64_t *d_starts = ctx->d_bstage, *d_ib = ctx->d_bstage + nb + 1;

    if (nb == 0) {
        HIP_OK(ctx, hipMemsetAsync(offs, 0, sizeof(uint64_t), s));
    } else if (rbs >= HUF_CHUNKED_FROM) {
        /* blocks of 2 MiB and more: item by item through the chunked path, each behind the one before */
        uint64_t pos = 0;
        for (uint64_t i = 0; i < nitems; i++) {
            const uint64_t len = item_lens[i];
            if (len == 0) continue;
            const uint64_t fb = h_ib[i], nbi = h_ib[i + 1] - fb;
            uint64_t got = 0;
            rc = encode_impl(ctx, in + h_starts[fb], len, blocksize, (uint8_t *)d_out + pos, out_cap - pos, offs + fb, NULL, &got, s);
            if (rc) return rc;
            if (pos) ebatch_shift_kernel<<<dim3(grid256(nbi + 1)), dim3(256), 0, s>>>(offs + fb, nbi + 1, pos);
            HIP_OK(ctx, hipGetLastError());
            pos += got;
        }
    } else {
        static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;
        const HufSubIndex sub = sub_index_rows(d_sub_index, nb, rbs);
        TwoLevel sizes = ctx->enc_sizes;
        sizes.total = offs + nb;
        /* the kernels encode_impl picks for blocks of rbs bytes: every one is bit-exact, the route only decides speed */
        if (rbs >= HL_MIN_BLOCK && !fused_only) {
            hist_lanes_batch_kernel<HL_THREADS><<<dim3((unsigned)nb), dim3(HL_THREADS), 0, s>>>(in, d_starts, ctx->d_hist);
            tree_wave_kernel<<<dim3((unsigned)nb), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        } else if (rbs <= HT_PACKED_MAX_BLOCK) {
            hist_tree_batch_kernel<HIST_THREADS, true><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, d_starts, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        } else {
            hist_tree_batch_kernel<HIST_THREADS, false><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, d_starts, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        }
        if (rbs <= 121392ull)
            pack_batch_kernel<PACK_THREADS, true><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, d_starts, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
        else
            pack_batch_kernel<PACK_THREADS, false><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, d_starts, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
        HIP_OK(ctx, hipGetLastError());
    }
    if (d_item_offsets || item_offsets) {
        uint64_t *dst = d_item_offsets ? d_item_offsets : ctx->d_bitem_offs;
        ebatch_item_offsets_kernel<<<dim3(grid256(nitems + 1)), dim3(256), 0, s>>>(offs, d_ib, nitems, dst);
        HIP_OK(ctx, hipGetLastError());
        if (item_offsets) {
            HIP_OK(ctx, hipMemcpyAsync(item_offsets, dst, (nitems + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
        }
    }
    return HUFE_OK;
}

extern "C" int hufgpu_decode_batch(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                   uint64_t nitems, const uint64_t *item_blocks, const uint64_t *out_offsets,
                                   const void *d_sub_index, uint64_t row_blocksize, void *d_out, uint32_t flags,
                                   int32_t *item_errs, uint64_t *item_raw_lens, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (nitems == 0) return HUFE_OK;
    if (!item_blocks || !out_offsets || !item_errs || !item_raw_lens || nitems > 0xffffffffull) return HUFE_ARGUMENT;
    if (item_blocks[0] != 0) {
        set_err(ctx, "decode_batch: item_blocks[0] must be 0");
        return HUFE_ARGUMENT;
    }
    for (uint64_t i = 0; i < nitems; i++) {
        if (item_blocks[i + 1] < item_blocks[i] || out_offsets[i + 1] < out_offsets[i]) {
            set_err(ctx, "decode_batch: item_blocks and out_offsets must not decrease (item %llu)", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
    }
    const uint64_t nb = item_blocks[nitems];
    const uint64_t out_end = out_offsets[nitems];
    if (nb > 0x7fffffffull || (nb && (!d_stream || !d_block_offsets)) || (!d_out && out_end > out_offsets[0])) return HUFE_ARGUMENT;
    const uint64_t cpb = d_sub_index ? (row_blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS : 0;
    if (d_sub_index && (row_blocksize == 0 || row_blocksize >= HUF_CHUNKED_FROM || ((uintptr_t)d_sub_index & 7u) ||
                        nb * cpb > 0x7fffffffull)) {
        set_err(ctx, "decode_batch: a sub-index needs an 8-byte aligned buffer and a row blocksize in 1 .. %llu",
                (unsigned long long)HUF_CHUNKED_FROM - 1);
        return HUFE_ARGUMENT;
    }
    for (uint64_t i = 0; i < nitems; i++) { item_errs[i] = HUFE_OK; item_raw_lens[i] = 0; }
    ctx->decode_pending = 0;
    if (nb == 0 || stream_len == 0) return HUFE_OK;     /* what hufgpu_decode() says to every item (src/decoder.c:218) */

    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    int rc = ensure_decode_ws(ctx, nb);
    if (rc) return rc;
    rc = ensure_batch_ws(ctx, nb, nitems);
    if (rc) return rc;
    uint64_t *h = NULL;
    rc = batch_stage(ctx, 2 * (nitems + 1), &h);
    if (rc) return rc;
    memcpy(h, item_blocks, (nitems + 1) * sizeof(uint64_t));
    memcpy(h + nitems + 1, out_offsets, (nitems + 1) * sizeof(uint64_t));
    rc = batch_upload(ctx, 2 * (nitems + 1), s);
    if (rc) return rc;

    const int max_tree = max_tree_of(flags);
    const uint8_t *st = (const uint8_t *)d_stream;
    const TwoLevel lens = decode_lens(ctx, nb);
    launch_decode_prepare(ctx, st, stream_len, d_block_offsets, nb, max_tree, lens, s);

    DecBatchArgs ba;
    ba.item_blocks = ctx->d_bstage;
    ba.out_offsets = ctx->d_bstage + nitems + 1;
    ba.nitems = nitems;
    ba.nblocks = nb;
    ba.dmeta = ctx->d_dmeta;
    ba.status = ctx->d_status;
    ba.lens = lens;
    ba.bprefix = ctx->d_bprefix;
    ba.obase = ctx->d_bobase;
    ba.blk_item = ctx->d_blk_item;
    ba.item_fail = ctx->d_item_fail;
    ba.item_res = ctx->d_item_res;
    dbatch_rebase_kernel<<<dim3(grid256((nb + 1 > nitems ? nb + 1 : nitems))), dim3(256), 0, s>>>(ba);

    /* the decoders read a block's output base as gprefix[blk / SCAN_GROUP] + local[blk]: zeros + the rebased offsets */
    TwoLevel blens = lens;
    blens.gprefix = ctx->d_bzero;
    blens.local = ctx->d_bobase;
    const HufSubIndex sub = sub_index_rows((void *)d_sub_index, nb, row_blocksize);
    const IndexedDecode job = {st, stream_len, d_block_offsets, nb, blens, (uint8_t *)d_out, out_end, &sub, row_blocksize};
    rc = launch_indexed_decoders(ctx, job, s);
    if (rc) return rc;
    dbatch_fail_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ba);
    dbatch_result_kernel<<<dim3(grid256(nitems)), dim3(256), 0, s>>>(ba);
    HIP_OK(ctx, hipGetLastError());
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_item_res, ctx->d_item_res, 3 * nitems * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));

    int first_err = HUFE_OK;
    uint64_t first_item = 0;
    for (uint64_t i = 0; i < nitems; i++) {
        const uint64_t *r = ctx->h_item_res + 3 * i;
        int err = (int)(int32_t)r[0];
        uint64_t raw = r[1];
        const uint64_t f = r[2];
        const uint64_t slot = out_offsets[i + 1] - out_offsets[i];
        if ((err == HUFE_RW || err == HUFE_CORRUPTED) && f < nb && raw <= slot) {
            /* what hufgpu_decode_result() does for the item alone: the failing block once more, in order, its record as the
             * whole input, into the item's slot behind the bytes in front of it (src/decoder.c:69-91) */
            uint64_t o[2] = {0, 0};
            HIP_OK(ctx, hipMemcpyAsync(o, d_block_offsets + f, sizeof(o), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            if (o[1] > stream_len) o[1] = stream_len;
            if (o[0] < o[1]) {
                uint64_t got = 0, used = 0, gu = 0, gr = 0;
                const int rc2 = decode_chain(ctx, st + o[0], o[1] - o[0], 1, (uint8_t *)d_out + out_offsets[i] + raw, slot - raw,
                                             max_tree, s, &got, &used, &gu, &gr);
                if (rc2 == err) raw += got;
            }
        }
        item_errs[i] = err;
        item_raw_lens[i] = raw;
        if (err != HUFE_OK && first_err == HUFE_OK) {
            first_err = err;
            first_item = i;
        }
    }
    if (first_err != HUFE_OK)
        set_err(ctx, "decode_batch: item %llu failed with error %d (%llu items in all)", (unsigned long long)first_item, first_err,
                (unsigned long long)nitems);
    return first_err;
}

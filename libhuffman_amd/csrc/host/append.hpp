/* append.hpp - hufgpu_append / hufgpu_truncate: an indexed stream made longer or shorter in place
   (include/huffman_gpu.h, kernels/append.hpp).  Part of hufgpu_api.hip (one translation unit). */
#pragma once

static HufSubIndex sub_view_from(HufSubIndex v, uint64_t b)     /* the view whose block 0 is block b */
{
    if (v.tile_bits) {
        v.tile_bits += b * v.tpb;
        v.group_bits += b * v.gpb;
        v.lens += b * HUF_NSYM;
    }
    return v;
}

/* What hufgpu_append and hufgpu_truncate share, behind their argument checks.  Blocks [0, nb_keep) stay.  With
 * view_len > 0, block `view` is opened again: its header must show view_len bytes, and with head > 0 it is decoded
 * and its first `head` bytes start row 0.  The src_len bytes at d_src follow.  new_raw is what the stream decodes to
 * afterwards: the layout of d_out_sub_index. */
static int append_impl(hufgpu_ctx *ctx, const char *who, void *d_stream, uint64_t stream_len, uint64_t stream_cap,
                       uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize, uint64_t nb_keep, uint64_t view,
                       uint64_t view_len, uint64_t head, const void *d_src, uint64_t src_len, uint64_t new_raw,
                       const void *d_sub_index, void *d_out_sub_index, uint32_t flags, uint64_t *out_len, void *stream)
{
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    ctx->last_stream = s;
    const uint8_t *st = (const uint8_t *)d_stream;
    const uint64_t new_bytes = head + src_len;
    const uint64_t rows = (new_bytes + blocksize - 1) / blocksize;
    const uint64_t block_bytes = (blocksize + 15u) & ~15ull;
    const bool big = blocksize >= HUF_CHUNKED_FROM;
    const int max_tree = max_tree_of(flags);
    const uint64_t *view_offsets = d_block_offsets + view;
    const HufSubIndex old_sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
    const HufSubIndex view_sub = sub_view_from(old_sub, view);

    int rc = ensure_decode_ws(ctx, 1);
    if (rc) return rc;
    const TwoLevel lens = decode_lens(ctx, 1);

    if (big) {
        /* blocks of 2 MiB and more: the rows go through encode_impl into the scratch area behind the decoded block and
         * are copied to their places once the new length is known to fit; a wait per step */
        const uint64_t len0 = head ? (new_bytes < blocksize ? new_bytes : blocksize) : 0;
        const uint64_t rest = new_bytes - len0;
        const uint64_t cap0 = len0 ? ((hufgpu_encode_bound(len0, blocksize) + 15u) & ~15ull) : 0;
        const uint64_t cap1 = rest ? ((hufgpu_encode_bound(rest, blocksize) + 15u) & ~15ull) : 0;
        rc = grow_range_scratch(ctx, block_bytes + cap0 + cap1);
        if (rc == HUFE_MEMORY) set_err(ctx, "%s: no room for the scratch area", who);
        if (rc) return rc;
        uint8_t *scr = ctx->d_rscratch, *enc0 = scr + block_bytes, *enc1 = enc0 + cap0;
        uint64_t base = 0;
        if (view_len) {
            launch_decode_prepare(ctx, st, stream_len, view_offsets, 1, max_tree, lens, s);
            HIP_OK(ctx, hipGetLastError());
            HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_dmeta, sizeof(HufDecodeMeta), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 10, d_block_offsets + nb_keep, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            HufDecodeMeta m;
            memcpy(&m, ctx->h_result + 8, sizeof(m));
            base = ctx->h_result[10];
            if (m.status != HUFE_OK) {
                set_err(ctx, "%s: the header of block %llu does not parse (error %d)", who, (unsigned long long)view, (int)m.status);
                return m.status;
            }
            if (m.block_len != view_len || base > stream_len) {
                set_err(ctx, "%s: block %llu holds %llu bytes where (raw_size, blocksize) give %llu: not a stream of hufgpu_encode() with these",
                        who, (unsigned long long)view, (unsigned long long)m.block_len, (unsigned long long)view_len);
                return HUFE_ARGUMENT;
            }
        }
        if (head) {
            uint64_t raw = 0;
            rc = decode_impl(ctx, st, stream_len, view_offsets, 1, view_sub.tile_bits ? &view_sub : NULL, blocksize, scr, view_len, flags, &raw, (void *)s);
            ctx->decode_pending = 0;
            ctx->last_st = NULL;
            if (rc) {
                set_err(ctx, "%s: block %llu does not decode (error %d)", who, (unsigned long long)view, rc);
                return rc;
            }
            if (len0 > head) HIP_OK(ctx, hipMemcpyAsync(scr + head, d_src, len0 - head, hipMemcpyDeviceToDevice, s));
        }
        uint64_t got0 = 0, got1 = 0;
        if (len0) {
            rc = encode_impl(ctx, scr, len0, blocksize, enc0, cap0, NULL, NULL, &got0, (void *)s);
            if (rc) return rc;
        }
        const uint64_t nb_rest = hufgpu_block_count(rest, blocksize);
        uint64_t *h_new = (uint64_t *)malloc((rows + 1) * sizeof(uint64_t));
        if (!h_new) return HUFE_MEMORY;
        h_new[0] = base;
        if (len0) h_new[1] = base + got0;
        if (rest) {
            rc = encode_impl(ctx, (const uint8_t *)d_src + (len0 - head), rest, blocksize, enc1, cap1, NULL, NULL, &got1, (void *)s);
            uint64_t *h_rest = h_new + (len0 ? 1 : 0);            /* the index of the rest, from 0: moved behind what is in front */
            const uint64_t front = h_rest[0];
            hipError_t he = hipSuccess;
            if (!rc) he = hipMemcpyAsync(h_rest, ctx->d_offsets, (nb_rest + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
            if (!rc && he == hipSuccess) he = hipStreamSynchronize(s);
            if (rc || he != hipSuccess) {
                free(h_new);
                HIP_OK(ctx, he);
                return rc;
            }
            for (uint64_t i = 0; i <= nb_rest; i++) h_rest[i] += front;
        }
        const uint64_t total = base + got0 + got1;
        if (total > stream_cap) {
            free(h_new);
            set_err(ctx, "%s: the new stream of %llu bytes does not fit the buffer of %llu", who, (unsigned long long)total, (unsigned long long)stream_cap);
            return HUFE_MEMORY;
        }
        hipError_t he = hipSuccess;
        if (got0) he = hipMemcpyAsync((uint8_t *)d_stream + base, enc0, got0, hipMemcpyDeviceToDevice, s);
        if (he == hipSuccess && got1) he = hipMemcpyAsync((uint8_t *)d_stream + base + got0, enc1, got1, hipMemcpyDeviceToDevice, s);
        if (he == hipSuccess) {
            if (view_len) he = hipMemcpyAsync(d_block_offsets + nb_keep + 1, h_new + 1, rows * sizeof(uint64_t), hipMemcpyHostToDevice, s);
            else he = hipMemcpyAsync(d_block_offsets + nb_keep, h_new, (rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s);
        }
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        free(h_new);
        HIP_OK(ctx, he);
        if (out_len) *out_len = total;
        return HUFE_OK;
    }

    rc = ensure_update_ws(ctx, rows + 1, 0);
    if (rc) return rc;
    rc = ensure_encode_ws(ctx, rows);
    if (rc) return rc;
    if (head) {
        rc = grow_range_scratch(ctx, block_bytes);
        if (rc == HUFE_MEMORY) set_err(ctx, "%s: no room for one block of %llu bytes in the scratch area", who, (unsigned long long)blocksize);
        if (rc) return rc;
    }
    uint8_t *scr = ctx->d_rscratch;
    const uint8_t *base = (const uint8_t *)d_src;
    if (head && (!base || (uintptr_t)scr < (uintptr_t)base)) base = scr;

    AppendArgs aa;
    memset(&aa, 0, sizeof(aa));
    aa.old_offsets = d_block_offsets;
    aa.index_w = d_block_offsets;
    aa.nb_keep = nb_keep;
    aa.rows = rows;
    aa.empty = view_len == 0;
    aa.stream_len = stream_len;
    aa.stream_cap = stream_cap;
    aa.blocksize = blocksize;
    aa.head = head;
    aa.expect_len = view_len;
    aa.new_bytes = new_bytes;
    aa.src_off = d_src ? (uint64_t)((uintptr_t)d_src - (uintptr_t)base) : 0;
    aa.scratch_off = head ? (uint64_t)((uintptr_t)scr - (uintptr_t)base) : 0;
    aa.src = (const uint8_t *)d_src;
    aa.scratch_w = scr;
    aa.dmeta = ctx->d_dmeta;
    aa.status = ctx->d_status;
    aa.meta = ctx->d_meta;
    aa.pairs = ctx->d_upairs;
    aa.row_blk = ctx->d_urow_blk;
    aa.sums = ctx->d_unew;
    aa.acount = ctx->d_ucount;

    if (view_len)
        launch_decode_prepare(ctx, st, stream_len, view_offsets, 1, max_tree, lens, s);
    app_plan_kernel<<<dim3(grid256(rows)), dim3(256), 0, s>>>(aa);
    if (head) {
        /* the block that is opened again through the indexed decoders as they are, to the front of the scratch area */
        const IndexedDecode job = {st, stream_len, view_offsets, 1, lens, scr, view_len, &view_sub, blocksize};
        rc = launch_indexed_decoders(ctx, job, s);
        if (rc) return rc;
        const uint64_t joined = (new_bytes < blocksize ? new_bytes : blocksize) - head;
        if (joined) {
            const uint64_t lead = (16u - (uint32_t)((uintptr_t)(scr + head) & 15u)) & 15u;
            const uint64_t chunks = (joined - (joined < lead ? joined : lead)) >> 4;
            const uint64_t npieces = chunks == 0 ? 1 : (chunks + DRANGE_PIECE_CHUNKS - 1) / DRANGE_PIECE_CHUNKS;
            app_join_kernel<<<dim3((unsigned)npieces), dim3(256), 0, s>>>(aa, joined);
        }
    }
    {
        TwoLevel sizes = ctx->enc_sizes;
        sizes.total = (uint64_t *)ctx->d_ucount + APP_WORDS;      /* (the rows' sum: not used, app_index_kernel sums them from the base) */
        launch_pairs_trees(ctx, base, rows, blocksize, sizes, s);
        app_index_kernel<256><<<dim3(1), dim3(256), 0, s>>>(aa);      /* few rows: four waves sweep them without the spill of sixteen */
        const HufSubIndex sub = sub_view_from(sub_index_view(d_out_sub_index, new_raw, blocksize), nb_keep);
        launch_pairs_pack(ctx, base, rows, blocksize, ctx->d_unew + 1, rows, stream_cap, (uint8_t *)d_stream, sub, s);
        app_commit_kernel<<<dim3(grid256(rows)), dim3(256), 0, s>>>(aa);
        if (d_sub_index && d_out_sub_index && nb_keep)
            app_sub_rows_kernel<<<dim3((unsigned)nb_keep), dim3(256), 0, s>>>(old_sub, sub_index_view(d_out_sub_index, new_raw, blocksize), blocksize, ctx->d_ucount);
    }
    HIP_OK(ctx, hipGetLastError());
    /* the one wait: (error, length) */
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_ucount, APP_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const int err = (int)ctx->h_result[8 + APP_ERR];
    if (err) {
        if (ctx->h_result[8 + APP_PLAN_ERR] == HUFE_ARGUMENT)
            set_err(ctx, "%s: block %llu does not hold the %llu bytes that (raw_size, blocksize) give it, or its index entry lies behind the stream: not a stream of hufgpu_encode() with these",
                    who, (unsigned long long)view, (unsigned long long)view_len);
        else if (ctx->h_result[8 + APP_PLAN_ERR])
            set_err(ctx, "%s: the header of block %llu does not parse (error %d)", who, (unsigned long long)view, err);
        else if (err == HUFE_MEMORY)
            set_err(ctx, "%s: the new stream does not fit the buffer of %llu bytes", who, (unsigned long long)stream_cap);
        else
            set_err(ctx, "%s: block %llu does not decode (error %d)", who, (unsigned long long)view, err);
        return err;
    }
    if (out_len) *out_len = ctx->h_result[8 + APP_TOTAL];
    return HUFE_OK;
}

/* the checks hufgpu_append and hufgpu_truncate share; new_raw gives the layout of d_out_sub_index */
static int append_check(const char *who, const void *d_stream, uint64_t stream_len, uint64_t stream_cap, const uint64_t *d_block_offsets,
                        uint64_t raw_size, uint64_t blocksize, uint64_t new_raw, const void *d_src, uint64_t src_len,
                        const void *d_sub_index, const void *d_out_sub_index)
{
    if (blocksize == 0 || blocksize > HUFGPU_MAX_BLOCK) {
        set_err(NULL, "%s: needs the blocksize the stream was written with (not 0, at most %llu)", who, (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUFE_ARGUMENT;
    }
    if (stream_len > stream_cap) {
        set_err(NULL, "%s: the stream of %llu bytes is longer than its buffer of %llu", who, (unsigned long long)stream_len, (unsigned long long)stream_cap);
        return HUFE_ARGUMENT;
    }
    if (new_raw < src_len || hufgpu_block_count(new_raw > raw_size ? new_raw : raw_size, blocksize) > 0x7fffffffull) {
        set_err(NULL, "%s: more than 2^31 - 1 blocks", who);
        return HUFE_ARGUMENT;
    }
    if ((raw_size || src_len) && (!d_stream || !d_block_offsets)) {
        set_err(NULL, "%s: the stream or its block index is missing", who);
        return HUFE_ARGUMENT;
    }
    if (src_len && !d_src) {
        set_err(NULL, "%s: the new bytes are missing", who);
        return HUFE_ARGUMENT;
    }
    if ((uintptr_t)d_stream & 3u) {                   /* pack writes whole words of the destination, as in hufgpu_encode */
        set_err(NULL, "%s: the stream must be 4-byte aligned", who);
        return HUFE_ARGUMENT;
    }
    if (((uintptr_t)d_sub_index | (uintptr_t)d_out_sub_index) & 7u) {
        set_err(NULL, "%s: a sub-index needs an 8-byte aligned buffer", who);
        return HUFE_ARGUMENT;
    }
    if (d_out_sub_index && blocksize >= HUF_CHUNKED_FROM) {
        set_err(NULL, "%s: a new sub-index needs blocks below %llu bytes", who, (unsigned long long)HUF_CHUNKED_FROM);
        return HUFE_ARGUMENT;
    }
    const uint64_t nb_old = hufgpu_block_count(raw_size, blocksize), nb_new = hufgpu_block_count(new_raw, blocksize);
    const uint64_t index_bytes = ((nb_old > nb_new ? nb_old : nb_new) + 1) * sizeof(uint64_t);
    const uint64_t old_sub = d_sub_index ? hufgpu_sub_index_bytes(raw_size, blocksize) : 0;
    const uint64_t new_sub = d_out_sub_index ? hufgpu_sub_index_bytes(new_raw, blocksize) : 0;
    if (spans_overlap(d_stream, stream_cap, d_block_offsets, index_bytes) || spans_overlap(d_src, src_len, d_stream, stream_cap) ||
        spans_overlap(d_src, src_len, d_block_offsets, index_bytes) || spans_overlap(d_sub_index, old_sub, d_stream, stream_cap) ||
        spans_overlap(d_sub_index, old_sub, d_block_offsets, index_bytes) || spans_overlap(d_out_sub_index, new_sub, d_stream, stream_cap) ||
        spans_overlap(d_out_sub_index, new_sub, d_block_offsets, index_bytes) || spans_overlap(d_out_sub_index, new_sub, d_sub_index, old_sub) ||
        spans_overlap(d_out_sub_index, new_sub, d_src, src_len) || spans_overlap(d_sub_index, old_sub, d_src, src_len)) {
        set_err(NULL, "%s: the new bytes and the sub-indexes must not overlap the stream's buffer, its index or one another", who);
        return HUFE_ARGUMENT;
    }
    return HUFE_OK;
}

extern "C" int hufgpu_append(hufgpu_ctx_t *ctx, void *d_stream, uint64_t stream_len, uint64_t stream_cap,
                             uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize, const void *d_src, uint64_t src_len,
                             const void *d_sub_index, void *d_out_sub_index, uint32_t flags, uint64_t *out_len, void *stream)
{
    if (out_len) *out_len = 0;
    const uint64_t new_raw = raw_size + src_len;
    int rc = append_check("append", d_stream, stream_len, stream_cap, d_block_offsets, raw_size, blocksize, new_raw, d_src, src_len,
                          d_sub_index, d_out_sub_index);
    if (rc) return rc;
    if (src_len == 0) {                               /* nothing to append: no context is needed for that */
        if (out_len) *out_len = stream_len;
        return HUFE_OK;
    }
    if (!ctx) {
        set_err(NULL, "append: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    const uint64_t nb_old = hufgpu_block_count(raw_size, blocksize), t = raw_size % blocksize;
    const uint64_t nb_keep = nb_old - (t > 0);
    const uint64_t view_len = raw_size == 0 ? 0 : (t ? t : blocksize);
    return append_impl(ctx, "append", d_stream, stream_len, stream_cap, d_block_offsets, raw_size, blocksize, nb_keep,
                       nb_old ? nb_old - 1 : 0, view_len, t, d_src, src_len, new_raw, d_sub_index, d_out_sub_index, flags, out_len, stream);
}

extern "C" int hufgpu_truncate(hufgpu_ctx_t *ctx, void *d_stream, uint64_t stream_len, uint64_t *d_block_offsets, uint64_t raw_size,
                               uint64_t blocksize, uint64_t new_raw_size, const void *d_sub_index, void *d_out_sub_index,
                               uint32_t flags, uint64_t *out_len, void *stream)
{
    if (out_len) *out_len = 0;
    if (new_raw_size > raw_size) {
        set_err(NULL, "truncate: the new size of %llu bytes is above the old one of %llu", (unsigned long long)new_raw_size, (unsigned long long)raw_size);
        return HUFE_ARGUMENT;
    }
    int rc = append_check("truncate", d_stream, stream_len, stream_len, d_block_offsets, raw_size, blocksize, new_raw_size, NULL, 0,
                          d_sub_index, d_out_sub_index);
    if (rc) return rc;
    if (new_raw_size == raw_size) {                   /* nothing to cut: no context is needed for that */
        if (out_len) *out_len = stream_len;
        return HUFE_OK;
    }
    if (!ctx) {
        set_err(NULL, "truncate: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    const uint64_t k = new_raw_size / blocksize, cut = new_raw_size % blocksize;
    if (cut == 0) {
        /* a cut on a block border: the records in front of it are the new stream, its length is the index entry there */
        ctx->decode_pending = 0;
        ctx->last_st = NULL;
        HIP_OK(ctx, hipSetDevice(ctx->device));
        hipStream_t s = pick_stream(ctx, stream);
        ctx->last_stream = s;
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, d_block_offsets + k, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        const uint64_t total = ctx->h_result[8];
        if (total > stream_len) {
            set_err(ctx, "truncate: index entry %llu lies behind the stream: not a stream of hufgpu_encode() with this (raw_size, blocksize)", (unsigned long long)k);
            return HUFE_ARGUMENT;
        }
        if (d_sub_index && d_out_sub_index && k) {
            rc = ensure_update_ws(ctx, 1, 0);
            if (rc) return rc;
            HIP_OK(ctx, hipMemsetAsync(ctx->d_ucount, 0, APP_WORDS * sizeof(unsigned long long), s));
            app_sub_rows_kernel<<<dim3((unsigned)k), dim3(256), 0, s>>>(sub_index_view((void *)d_sub_index, raw_size, blocksize),
                                                                         sub_index_view(d_out_sub_index, new_raw_size, blocksize), blocksize, ctx->d_ucount);
            HIP_OK(ctx, hipGetLastError());
            HIP_OK(ctx, hipStreamSynchronize(s));
        }
        if (out_len) *out_len = total;
        return HUFE_OK;
    }
    const uint64_t nb_old = hufgpu_block_count(raw_size, blocksize), t = raw_size % blocksize;
    const uint64_t view_len = (k == nb_old - 1 && t) ? t : blocksize;
    return append_impl(ctx, "truncate", d_stream, stream_len, stream_len, d_block_offsets, raw_size, blocksize, k, k, view_len, cut,
                       NULL, 0, new_raw_size, d_sub_index, d_out_sub_index, flags, out_len, stream);
}

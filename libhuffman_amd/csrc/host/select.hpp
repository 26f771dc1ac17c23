/* select.hpp - hufgpu_select_spans: the non-overlapping leftmost-longest selection over the spans of
   hufgpu_find_any_spans (include/huffman_gpu.h, kernels/select.hpp), enqueue-only.  Part of hufgpu_api.hip (one
   translation unit). */
#pragma once

static_assert(SEL_WINDOW == HUFGPU_FIND_PATTERN_MAX, "kernels/select.hpp and include/huffman_gpu.h");
static_assert(HUFGPU_SELECT_MAX / SEL_TILE <= (uint64_t)SEL_FAN * SEL_FAN * SEL_FAN * SEL_FAN, "SEL_LEVELS_MAX levels reach every tile");

extern "C" void hufgpu_select_geometry(uint32_t out[2])
{
    if (!out) return;
    out[0] = SEL_TILE;
    out[1] = SEL_FAN;
}

extern "C" int hufgpu_select_spans(hufgpu_ctx_t *ctx, const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_n, uint64_t n_cap,
                                   uint64_t *d_sel_pos, uint32_t *d_sel_len, uint64_t *d_sel_rank, uint64_t sel_cap, uint64_t pad_pos,
                                   uint64_t *d_sel_totals, uint32_t flags, void *stream)
{
    if (!d_pos || !d_len || !d_sel_totals) return find_bad(ctx, "select_spans: d_pos, d_len and d_sel_totals are required");
    if (sel_cap > 0 && (!d_sel_pos || !d_sel_len))
        return find_bad(ctx, "select_spans: sel_cap %llu needs d_sel_pos and d_sel_len", (unsigned long long)sel_cap);
    if (n_cap > HUFGPU_SELECT_MAX)
        return find_bad(ctx, "select_spans: n_cap %llu is above HUFGPU_SELECT_MAX, %llu", (unsigned long long)n_cap,
                        (unsigned long long)HUFGPU_SELECT_MAX);
    if (flags & ~HUFGPU_SELECT_PAD) return find_bad(ctx, "select_spans: flags 0x%x has a bit other than HUFGPU_SELECT_PAD", flags);
    const struct { const void *p; const char *name; } ins[] = {{d_pos, "d_pos"}, {d_len, "d_len"}, {d_n, "d_n"}},
                                                      outs[] = {{d_sel_pos, "d_sel_pos"}, {d_sel_len, "d_sel_len"},
                                                                {d_sel_rank, "d_sel_rank"}, {d_sel_totals, "d_sel_totals"}};
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (o.p && o.p == i.p) return find_bad(ctx, "select_spans: %s starts at the address of %s", o.name, i.name);
    if (!ctx) return find_bad(NULL, "select_spans: needs a context (there is no CPU path)");
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);

    SelectArgs a;
    memset(&a, 0, sizeof(a));
    a.pos = d_pos;
    a.len = d_len;
    a.n_word = d_n;
    a.n_cap = n_cap;
    a.ntiles = (n_cap + SEL_TILE - 1) / SEL_TILE;
    a.sel_pos = d_sel_pos;
    a.sel_len = d_sel_len;
    a.sel_rank = d_sel_rank;
    a.sel_cap = sel_cap;
    a.pad_pos = pad_pos;
    a.totals = d_sel_totals;
    a.flags = flags;
    if (a.ntiles > 0) {
        const int rc = grow_ws(ctx, G_SELECT, a.ntiles);
        if (rc) return rc;
        /* three levels whatever n_cap is, up to 2^28 ranks: the number of launches does not depend on it */
        a.levels = a.ntiles <= (uint64_t)SEL_FAN * SEL_FAN * SEL_FAN ? 3 : SEL_LEVELS_MAX;
        uint64_t at = 0, count = a.ntiles;
        for (uint32_t k = 0; k <= a.levels; k++) {
            a.maps[k] = ctx->d_smaps + at * SEL_WINDOW;
            a.count[k] = count;
            at += count;
            count = (count + SEL_FAN - 1) / SEL_FAN;
        }
        a.marks = ctx->d_smarks;
        a.bad = ctx->d_swords;
        a.scan = ctx->sel_scan;
        a.scan.total = (uint64_t *)ctx->d_swords + 1;
        HIP_OK(ctx, hipMemsetAsync(ctx->d_swords, 0xff, sizeof(unsigned long long), s));
        select_tile_kernel<<<dim3((unsigned)a.ntiles), dim3(SEL_THREADS), 0, s>>>(a);
        for (uint32_t k = 0; k < a.levels; k++) {
            const uint64_t groups = (a.count[k] + SEL_FAN - 1) / SEL_FAN, waves = SEL_THREADS / 64;
            select_compose_kernel<<<dim3((unsigned)((groups + waves - 1) / waves)), dim3(SEL_THREADS), 0, s>>>(a, k);
        }
        select_mark_kernel<<<dim3((unsigned)a.ntiles), dim3(SEL_THREADS), 0, s>>>(a);
        if (sel_cap > 0) select_emit_kernel<<<dim3((unsigned)a.ntiles), dim3(SEL_THREADS), 0, s>>>(a);
    }
    uint64_t pads = flags & HUFGPU_SELECT_PAD ? (sel_cap + 255) / 256 : 1;
    if (pads < 1) pads = 1;
    if (pads > 8ull * (uint64_t)ctx->cus) pads = 8ull * (uint64_t)ctx->cus;
    select_finish_kernel<<<dim3((unsigned)pads), dim3(256), 0, s>>>(a);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

/* profile.hpp - per-kernel timing of the encode and decode calls: STAGE_BEGIN / STAGE_MARK record HIP events into the
   context's slots, hufgpu_set_profiling / hufgpu_get_profile switch them on and sum them.
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

#define STAGE_BEGIN(c, s, kind)                                                         \
    do {                                                                                \
        (c)->n_stages = 0;                                                              \
        (c)->cur_slot = -1;                                                             \
        if ((c)->profiling && (c)->prof_used < PROF_SLOTS) {                            \
            (c)->cur_slot = (c)->prof_used++;                                           \
            (c)->slot_kind[(c)->cur_slot] = (kind);                                     \
            (c)->slot_stages[(c)->cur_slot] = 0;                                        \
            HIP_OK((c), hipEventRecord((c)->ev[(c)->cur_slot][0], (s)));                \
        }                                                                               \
    } while (0)
#define STAGE_MARK(c, s)                                                                \
    do {                                                                                \
        if ((c)->cur_slot >= 0 && (c)->n_stages < MAX_STAGES) {                         \
            (c)->n_stages++;                                                            \
            (c)->slot_stages[(c)->cur_slot] = (c)->n_stages;                            \
            HIP_OK((c), hipEventRecord((c)->ev[(c)->cur_slot][(c)->n_stages], (s)));    \
        }                                                                               \
    } while (0)

extern "C" int hufgpu_set_profiling(hufgpu_ctx_t *ctx, int enabled)
{
    if (!ctx) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    if (enabled && !ctx->ev) {
        ctx->ev = (hipEvent_t(*)[MAX_STAGES + 1])calloc(PROF_SLOTS, sizeof(*ctx->ev));
        if (!ctx->ev) return HUFE_MEMORY;
        for (int k = 0; k < PROF_SLOTS; k++)
            for (int i = 0; i <= MAX_STAGES; i++) HIP_OK(ctx, hipEventCreate(&ctx->ev[k][i]));
    }
    ctx->profiling = enabled ? 1 : 0;
    if (enabled == 1) ctx->prof_used = 0;        /* 1 = start a new record, 2 = resume, 0 = pause (record kept) */
    ctx->cur_slot = -1;
    return HUFE_OK;
}

extern "C" int hufgpu_get_profile(hufgpu_ctx_t *ctx, int kind, float *ms_sum, int max_stages,
                                  int *n_stages, int *n_calls)
{
    if (!ctx || !ms_sum || !n_stages || !n_calls) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    *n_stages = 0;
    *n_calls = 0;
    for (int i = 0; i < max_stages; i++) ms_sum[i] = 0.f;
    for (int k = 0; k < ctx->prof_used; k++) {
        if (ctx->slot_kind[k] != kind) continue;
        const int ns = ctx->slot_stages[k] < max_stages ? ctx->slot_stages[k] : max_stages;
        if (ns <= 0) continue;
        HIP_OK(ctx, hipEventSynchronize(ctx->ev[k][ctx->slot_stages[k]]));
        for (int i = 0; i < ns; i++) {
            float ms = 0.f;
            HIP_OK(ctx, hipEventElapsedTime(&ms, ctx->ev[k][i], ctx->ev[k][i + 1]));
            ms_sum[i] += ms;
        }
        if (ns > *n_stages) *n_stages = ns;
        (*n_calls)++;
    }
    return HUFE_OK;
}

/* ctx.hpp - the per-device context of the device C ABI (include/huffman_gpu.h): the struct, the error text, create and
   destroy, and every workspace of it - each feature's free_* / ensure_* pair lives here, next to the members it owns.
   Part of hufgpu_api.hip (one translation unit). */
#pragma once

struct hufgpu_ctx {
    int device;
    hipStream_t stream;
    char err[512];

    /* encode workspace, sized for ws_blocks blocks */
    uint64_t ws_blocks;
    uint32_t *d_hist;
    hufcode_t *d_codetab;
    int16_t *d_treebuf;
    HufBlockMeta *d_meta;
    uint64_t *d_offsets;          /* used when the caller passes no index buffer */
    TwoLevel enc_sizes;           /* two-level prefix sums of the encoded block sizes */
    uint64_t ws_chunks;           /* blocks >= HUF_BIG_BLOCK: per-chunk counts, payload bits and first bits */
    uint32_t *d_chunk_hist;
    uint64_t *d_chunk_tot, *d_chunk_bits;

    /* decode workspace */
    uint64_t dws_blocks;
    HufDecodeMeta *d_dmeta;
    uint64_t *d_out_offsets;
    int32_t *d_status;
    TwoLevel dec_lens;            /* two-level prefix sums of the block lengths */
    uint32_t *d_fix_count;        /* decode_sub_kernel: blocks its sub-index could not verify */
    uint32_t *d_fix_blocks;
    uint32_t *d_fix_flag;

    /* raw-stream discovery workspace */
    uint64_t disc_wgs, disc_cands;
    uint32_t *d_wg_counts;
    void *d_disc_slots;           /* DISC_SLOTS candidates a discovery workgroup (kernels/discover.hpp, DiscSlot) */
    uint64_t *d_disc_masks;       /* 64 header-test verdicts per discovery thread */
    uint64_t *d_wg_base;
    uint64_t *d_cand, *d_cand_end, *d_chain;
    int32_t *d_cand_status;
    uint32_t *d_nxt;
    uint64_t *d_walk;             /* 5 result words of walk_kernel */
    uint64_t *d_spec_off;         /* speculative output offsets of the candidates (disc_cands + 1) */

    /* blocks of many MiB in a raw stream: the sub-index built for them (kernels/spec_index.hpp) */
    uint64_t big_lanes, big_sub_bytes;
    uint64_t *d_big_entry, *d_big_exit, *d_big_pre, *d_big_wgpre, *d_big_wgscratch, *d_big_first_pos, *d_big_first_g, *d_big_last_pos;
    uint32_t *d_big_cnt;
    void *d_big_sub;
    uint64_t *d_big_offs;         /* SPEC_WORDS status words, then the two-entry block index */

    uint64_t *d_result;           /* 8 words: err, raw_len, failing block / consumed, blocks, complete consumed, complete raw */
    uint64_t complete_used, complete_raw;   /* of the last hufgpu_decode_stream(): see hufgpu_decode_stream_complete() */
    uint64_t *h_result;           /* pinned mirror */
    uint64_t *d_zipf;             /* 255 cumulative weights */

    /* per-kernel timing: every profiled call records HIP events around its kernels into the
     * next slot; hufgpu_get_profile() sums the slots, so a timed loop needs no host sync */
    int profiling;
    int prof_used;
    int cur_slot;
    int n_stages;
    hipEvent_t (*ev)[MAX_STAGES + 1];
    int slot_stages[PROF_SLOTS];
    int slot_kind[PROF_SLOTS];
    int decode_pending;
    hipStream_t last_stream;
    /* the last enqueued indexed decode: hufgpu_decode_result() decodes a failing block once more, in order */
    const uint8_t *last_st;
    const uint64_t *last_offsets;
    uint8_t *last_out;
    uint64_t last_stream_len, last_out_cap, last_nblocks;
    uint64_t last_failing;        /* hufgpu_decode_result: the first failing block of the last indexed decode (~0: none) */
    int last_max_tree;

    /* batch calls (hufgpu_encode_batch / hufgpu_decode_batch): their host tables go up through a pinned staging
     * area; an encode only enqueues, so the next call waits for the event behind the last copy before it writes there */
    uint64_t *h_bstage, *d_bstage;
    uint64_t bstage_words;
    hipEvent_t bstage_ev;
    int bstage_pending;
    uint64_t bws_blocks, bws_items;
    uint64_t *d_bprefix, *d_bobase, *d_bzero;
    uint32_t *d_blk_item;
    unsigned long long *d_item_fail;
    uint64_t *d_item_res, *h_item_res;
    uint64_t *d_bitem_offs;

    /* hufgpu_decode_ranges (kernels/ranges.hpp): its plan per block and per range, next to the batch workspace it shares,
     * and the scratch area the staged blocks are decoded into */
    uint64_t rws_blocks, rws_ranges;
    unsigned long long *d_rcover;
    uint64_t *d_rrel, *d_rplan;
    uint32_t *d_rflag;
    unsigned long long *d_rcounters;
    unsigned long long *d_rtpairs;            /* the tile route's (range, tile) pairs per block (kernels/range_tiles.hpp) */
    uint64_t rcounters[8];                    /* hufgpu_ranges_counters(): of the last hufgpu_decode_ranges */
    uint8_t *d_rscratch;
    uint64_t rscratch_bytes;

    /* hufgpu_gather (kernels/gather.hpp): part counts and cursors per block, the list of touched blocks, the scan of the
     * counts and its grand total, the parts */
    uint64_t gws_blocks, gws_parts;
    uint32_t *d_gcnt, *d_glist;
    TwoLevel gat_scan;
    uint64_t *d_gtotal;
    void *d_gparts;
    int cus;                                  /* compute units of the device */

    /* hufgpu_find_bytes (kernels/find.hpp): a match mask per group of 32 symbols, a count per tile, the scan of the counts */
    uint64_t fws_words, fws_tiles;
    uint32_t *d_fbitmap, *d_ftcnt;
    TwoLevel find_scan;

    /* the sub-index builders (kernels/sub_build.hpp): what their kernels hand to one another, per block and per chunk */
    uint64_t sbws_blocks, sbws_chunks;
    uint32_t *d_sb_state;
    uint64_t *d_sb_pay, *d_sb_chunk_tot, *d_sb_chunk_bits;
    unsigned long long *d_sb_unbuilt;

    /* hufgpu_update_ranges (kernels/update.hpp): the touched blocks' rows, the new index when the caller wants none,
     * the copy pieces' first blocks */
    uint64_t uws_blocks, uws_pieces;
    uint32_t *d_urow_of, *d_urow_blk, *d_upiece;
    uint64_t *d_upairs, *d_unew;
    unsigned long long *d_ucount;
};

static char g_err[512] = "";

static void set_err(hufgpu_ctx *ctx, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof(g_err), "%s", buf);
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s", buf);
    fprintf(stderr, "libhuffman(gpu): %s\n", buf);
}

#define HIP_OK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_err((ctx), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                    __LINE__);                                                              \
            return HUFE_FATAL;                                                              \
        }                                                                                   \
    } while (0)

extern "C" int hufgpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int usable = 0;
    for (int d = 0; d < n; d++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) usable++;
    }
    return usable;
}

extern "C" const char *hufgpu_last_error(const hufgpu_ctx_t *ctx) { return ctx ? ctx->err : g_err; }

extern "C" int hufgpu_ctx_create(hufgpu_ctx_t **out, int device)
{
    if (!out) return HUFE_ARGUMENT;
    *out = NULL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_err(NULL, "no HIP device available (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "0 devices");
        return HUFE_FATAL;
    }
    if (device < 0 || device >= n) {
        set_err(NULL, "device %d out of range (have %d)", device, n);
        return HUFE_ARGUMENT;
    }
    hipDeviceProp_t prop;
    HIP_OK(NULL, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(NULL, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
        return HUFE_FATAL;
    }
    hufgpu_ctx *ctx = (hufgpu_ctx *)calloc(1, sizeof(hufgpu_ctx));
    if (!ctx) return HUFE_MEMORY;
    ctx->device = device;
    ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_OK(NULL, hipSetDevice(device));
    ctx->stream = NULL;   /* the device's default stream: ordered with every blocking stream (torch's default included) */
    HIP_OK(ctx, hipMalloc((void **)&ctx->d_result, 8 * sizeof(uint64_t)));
    HIP_OK(ctx, hipMalloc((void **)&ctx->d_walk, DISC_WORDS * sizeof(uint64_t)));
    HIP_OK(ctx, hipHostMalloc((void **)&ctx->h_result, 16 * sizeof(uint64_t), hipHostMallocDefault));

    /* zipf255 cumulative weights: w_r = floor(2^32 / r), r = 1..255 */
    uint64_t cum[255], acc = 0;
    for (int r = 1; r <= 255; r++) {
        acc += (1ull << 32) / (uint64_t)r;
        cum[r - 1] = acc;
    }
    HIP_OK(ctx, hipMalloc((void **)&ctx->d_zipf, sizeof(cum)));
    HIP_OK(ctx, hipMemcpy(ctx->d_zipf, cum, sizeof(cum), hipMemcpyHostToDevice));
    *out = ctx;
    return HUFE_OK;
}

extern "C" int hufgpu_ctx_device(const hufgpu_ctx_t *ctx) { return ctx ? ctx->device : -1; }

/* workspace of a two-level prefix sum over `cap` blocks; counters start (and are left) at zero */
static int alloc_two_level(hufgpu_ctx *c, TwoLevel *t, uint64_t cap, bool with_min)
{
    const uint64_t groups = cap / SCAN_GROUP + 2;
    memset(t, 0, sizeof(*t));
    HIP_OK(c, hipMalloc((void **)&t->vals, cap * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&t->local, cap * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&t->gsum, groups * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&t->gprefix, groups * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&t->gcount, groups * SCAN_TICKET_STRIDE * sizeof(uint32_t)));
    HIP_OK(c, hipMalloc((void **)&t->done, sizeof(uint32_t)));
    if (with_min) HIP_OK(c, hipMalloc((void **)&t->gmin, groups * sizeof(uint64_t)));
    HIP_OK(c, hipMemset(t->gcount, 0, groups * SCAN_TICKET_STRIDE * sizeof(uint32_t)));
    HIP_OK(c, hipMemset(t->done, 0, sizeof(uint32_t)));
    HIP_OK(c, hipDeviceSynchronize());   /* the kernels may run on a non-blocking stream: the zeros must be there first */
    return HUFE_OK;
}

static void free_two_level(TwoLevel *t)
{
    (void)hipFree(t->vals); (void)hipFree(t->local); (void)hipFree(t->gsum); (void)hipFree(t->gprefix);
    (void)hipFree(t->gcount); (void)hipFree(t->done); (void)hipFree(t->gmin);
    memset(t, 0, sizeof(*t));
}

static void free_encode_ws(hufgpu_ctx *c)
{
    free_two_level(&c->enc_sizes);
    (void)hipFree(c->d_hist);
    (void)hipFree(c->d_codetab);
    (void)hipFree(c->d_treebuf);
    (void)hipFree(c->d_meta);
    (void)hipFree(c->d_offsets);
    (void)hipFree(c->d_chunk_hist); (void)hipFree(c->d_chunk_tot); (void)hipFree(c->d_chunk_bits);
    c->d_chunk_hist = NULL; c->d_chunk_tot = NULL; c->d_chunk_bits = NULL; c->ws_chunks = 0;
    c->d_hist = NULL; c->d_codetab = NULL; c->d_treebuf = NULL; c->d_meta = NULL; c->d_offsets = NULL;
    c->ws_blocks = 0;
}

static void free_disc_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) { (void)hipFree(c->d_wg_counts); (void)hipFree(c->d_wg_base); (void)hipFree(c->d_disc_masks); (void)hipFree(c->d_disc_slots); c->d_disc_slots = NULL; c->d_wg_counts = NULL; c->d_wg_base = NULL; c->d_disc_masks = NULL; c->disc_wgs = 0; }
    if (which & 2) {
        (void)hipFree(c->d_cand); (void)hipFree(c->d_cand_end); (void)hipFree(c->d_chain); (void)hipFree(c->d_cand_status); (void)hipFree(c->d_nxt); (void)hipFree(c->d_spec_off);
        c->d_cand = c->d_cand_end = c->d_chain = NULL; c->d_cand_status = NULL; c->d_nxt = NULL; c->d_spec_off = NULL; c->disc_cands = 0;
    }
}

static void free_big_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) {
        (void)hipFree(c->d_big_entry); (void)hipFree(c->d_big_exit); (void)hipFree(c->d_big_pre); (void)hipFree(c->d_big_cnt);
        (void)hipFree(c->d_big_wgpre); (void)hipFree(c->d_big_wgscratch);
        (void)hipFree(c->d_big_first_pos); (void)hipFree(c->d_big_first_g); (void)hipFree(c->d_big_last_pos);
        c->d_big_entry = c->d_big_exit = c->d_big_pre = c->d_big_wgpre = c->d_big_wgscratch = NULL; c->d_big_cnt = NULL; c->big_lanes = 0;
        c->d_big_first_pos = c->d_big_first_g = c->d_big_last_pos = NULL;
    }
    if (which & 4) { (void)hipFree(c->d_big_sub); c->d_big_sub = NULL; c->big_sub_bytes = 0; }
    if (which & 8) { (void)hipFree(c->d_big_offs); c->d_big_offs = NULL; }
}

static void free_decode_ws(hufgpu_ctx *c)
{
    free_two_level(&c->dec_lens);
    (void)hipFree(c->d_dmeta);
    (void)hipFree(c->d_out_offsets);
    (void)hipFree(c->d_status);
    (void)hipFree(c->d_fix_count); (void)hipFree(c->d_fix_blocks); (void)hipFree(c->d_fix_flag);
    c->d_fix_count = NULL; c->d_fix_blocks = NULL; c->d_fix_flag = NULL;
    c->d_dmeta = NULL; c->d_out_offsets = NULL; c->d_status = NULL;
    c->dws_blocks = 0;
}

static void free_batch_ws(hufgpu_ctx *c)
{
    (void)hipFree(c->d_bprefix); (void)hipFree(c->d_bobase); (void)hipFree(c->d_bzero); (void)hipFree(c->d_blk_item);
    (void)hipFree(c->d_item_fail); (void)hipFree(c->d_item_res); (void)hipFree(c->d_bitem_offs); (void)hipHostFree(c->h_item_res);
    c->d_bprefix = c->d_bobase = c->d_bzero = NULL; c->d_blk_item = NULL; c->d_item_fail = NULL;
    c->d_item_res = c->h_item_res = c->d_bitem_offs = NULL;
    c->bws_blocks = c->bws_items = 0;
}

static void free_range_ws(hufgpu_ctx *c)
{
    (void)hipFree(c->d_rcover); (void)hipFree(c->d_rrel); (void)hipFree(c->d_rplan); (void)hipFree(c->d_rflag); (void)hipFree(c->d_rtpairs);
    c->d_rcover = NULL; c->d_rrel = c->d_rplan = NULL; c->d_rflag = NULL; c->d_rtpairs = NULL;
    c->rws_blocks = c->rws_ranges = 0;
}

static void free_gather_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) {
        if (c->gws_blocks) free_two_level(&c->gat_scan);
        (void)hipFree(c->d_gcnt); (void)hipFree(c->d_glist);
        c->d_gcnt = c->d_glist = NULL; c->gws_blocks = 0;
    }
    if (which & 2) { (void)hipFree(c->d_gparts); c->d_gparts = NULL; c->gws_parts = 0; }
}

static void free_find_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) { (void)hipFree(c->d_fbitmap); c->d_fbitmap = NULL; c->fws_words = 0; }
    if (which & 2) {
        if (c->fws_tiles) free_two_level(&c->find_scan);
        (void)hipFree(c->d_ftcnt);
        c->d_ftcnt = NULL; c->fws_tiles = 0;
    }
}

static void free_range_scratch(hufgpu_ctx *c)
{
    (void)hipFree(c->d_rscratch);
    c->d_rscratch = NULL;
    c->rscratch_bytes = 0;
}

/* The scratch area that hufgpu_decode_ranges, hufgpu_build_sub_index and hufgpu_update_ranges share: at least `bytes`
 * bytes, with an eighth of room to grow into when that can be had.  HUFE_MEMORY (the area is then gone) when it cannot. */
static int grow_range_scratch(hufgpu_ctx *ctx, uint64_t bytes)
{
    if (bytes <= ctx->rscratch_bytes) return HUFE_OK;
    HIP_OK(ctx, hipDeviceSynchronize());
    free_range_scratch(ctx);
    if (bytes > ((uint64_t)1 << 46)) return HUFE_MEMORY;
    uint64_t got = bytes + bytes / 8;
    if (hipMalloc((void **)&ctx->d_rscratch, got) != hipSuccess) {
        (void)hipGetLastError();
        ctx->d_rscratch = NULL;
        got = bytes;
        if (hipMalloc((void **)&ctx->d_rscratch, got) != hipSuccess) {
            (void)hipGetLastError();
            ctx->d_rscratch = NULL;
            return HUFE_MEMORY;
        }
    }
    ctx->rscratch_bytes = got;
    return HUFE_OK;
}

static void free_sub_build_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) { (void)hipFree(c->d_sb_state); (void)hipFree(c->d_sb_pay); c->d_sb_state = NULL; c->d_sb_pay = NULL; c->sbws_blocks = 0; }
    if (which & 2) { (void)hipFree(c->d_sb_chunk_tot); (void)hipFree(c->d_sb_chunk_bits); c->d_sb_chunk_tot = c->d_sb_chunk_bits = NULL; c->sbws_chunks = 0; }
}

static void free_update_ws(hufgpu_ctx *c, int which)
{
    if (which & 1) {
        (void)hipFree(c->d_urow_of); (void)hipFree(c->d_urow_blk); (void)hipFree(c->d_upairs); (void)hipFree(c->d_unew);
        c->d_urow_of = c->d_urow_blk = NULL; c->d_upairs = c->d_unew = NULL; c->uws_blocks = 0;
    }
    if (which & 2) { (void)hipFree(c->d_upiece); c->d_upiece = NULL; c->uws_pieces = 0; }
}

static void free_batch_stage(hufgpu_ctx *c)
{
    if (c->bstage_pending) (void)hipEventSynchronize(c->bstage_ev);
    (void)hipHostFree(c->h_bstage); (void)hipFree(c->d_bstage);
    c->h_bstage = c->d_bstage = NULL;
    c->bstage_words = 0;
    c->bstage_pending = 0;
}

extern "C" int hufgpu_ctx_destroy(hufgpu_ctx_t *ctx)
{
    if (!ctx) return HUFE_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    free_batch_stage(ctx);
    if (ctx->bstage_ev) (void)hipEventDestroy(ctx->bstage_ev);
    free_batch_ws(ctx);
    free_range_ws(ctx);
    free_range_scratch(ctx);
    free_gather_ws(ctx, 3);
    (void)hipFree(ctx->d_gtotal);
    free_find_ws(ctx, 3);
    (void)hipFree(ctx->d_rcounters);
    free_sub_build_ws(ctx, 3);
    (void)hipFree(ctx->d_sb_unbuilt);
    free_update_ws(ctx, 3);
    (void)hipFree(ctx->d_ucount);
    free_encode_ws(ctx);
    free_decode_ws(ctx);
    free_disc_ws(ctx, 3);
    free_big_ws(ctx, 15);
    (void)hipFree(ctx->d_walk);
    (void)hipFree(ctx->d_result);
    (void)hipFree(ctx->d_zipf);
    (void)hipHostFree(ctx->h_result);
    if (ctx->ev) {
        for (int k = 0; k < PROF_SLOTS; k++)
            for (int i = 0; i <= MAX_STAGES; i++) (void)hipEventDestroy(ctx->ev[k][i]);
        free(ctx->ev);
    }
    free(ctx);
    return HUFE_OK;
}

static int ensure_encode_ws(hufgpu_ctx *c, uint64_t nblocks)
{
    if (nblocks <= c->ws_blocks) return HUFE_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    free_encode_ws(c);
    const uint64_t cap = nblocks + nblocks / 8 + 16;
    HIP_OK(c, hipMalloc((void **)&c->d_hist, cap * HUF_NSYM * sizeof(uint64_t)));   /* (64-bit counts for chunked blocks) */
    HIP_OK(c, hipMalloc((void **)&c->d_codetab, cap * HUF_NSYM * sizeof(hufcode_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_treebuf, cap * HUF_TREE_STRIDE * sizeof(int16_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_meta, cap * sizeof(HufBlockMeta)));
    HIP_OK(c, hipMalloc((void **)&c->d_offsets, (cap + 1) * sizeof(uint64_t)));
    int rc2 = alloc_two_level(c, &c->enc_sizes, cap, false);
    if (rc2) return rc2;
    c->ws_blocks = cap;
    return HUFE_OK;
}

static int ensure_chunk_ws(hufgpu_ctx *c, uint64_t nchunks)
{
    if (nchunks <= c->ws_chunks) return HUFE_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_chunk_hist); (void)hipFree(c->d_chunk_tot); (void)hipFree(c->d_chunk_bits);
    c->d_chunk_hist = NULL; c->d_chunk_tot = NULL; c->d_chunk_bits = NULL; c->ws_chunks = 0;
    const uint64_t cap = nchunks + nchunks / 8 + 16;
    HIP_OK(c, hipMalloc((void **)&c->d_chunk_hist, cap * HUF_NSYM * sizeof(uint32_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_chunk_tot, cap * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_chunk_bits, cap * sizeof(uint64_t)));
    c->ws_chunks = cap;
    return HUFE_OK;
}

static int ensure_decode_ws(hufgpu_ctx *c, uint64_t nblocks)
{
    if (nblocks <= c->dws_blocks) return HUFE_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    free_decode_ws(c);
    const uint64_t cap = nblocks + nblocks / 8 + 16;
    HIP_OK(c, hipMalloc((void **)&c->d_dmeta, cap * sizeof(HufDecodeMeta)));
    HIP_OK(c, hipMalloc((void **)&c->d_out_offsets, (cap + 1) * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_status, cap * sizeof(int32_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_fix_count, 2 * sizeof(uint32_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_fix_blocks, cap * sizeof(uint32_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_fix_flag, cap * sizeof(uint32_t)));
    HIP_OK(c, hipMemset(c->d_fix_count, 0, 2 * sizeof(uint32_t)));
    HIP_OK(c, hipMemset(c->d_fix_flag, 0, cap * sizeof(uint32_t)));
    int rc2 = alloc_two_level(c, &c->dec_lens, cap, true);
    if (rc2) return rc2;
    c->dws_blocks = cap;
    return HUFE_OK;
}

static int ensure_batch_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nitems)
{
    if (nblocks <= c->bws_blocks && nitems <= c->bws_items) return HUFE_OK;
    HIP_OK(c, hipDeviceSynchronize());
    const uint64_t nbc = (nblocks > c->bws_blocks ? nblocks + nblocks / 8 : c->bws_blocks) + 16;
    const uint64_t nic = (nitems > c->bws_items ? nitems + nitems / 8 : c->bws_items) + 16;
    free_batch_ws(c);
    HIP_OK(c, hipMalloc((void **)&c->d_bprefix, (nbc + 1) * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_bobase, nbc * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_bzero, (nbc / SCAN_GROUP + 2) * sizeof(uint64_t)));
    HIP_OK(c, hipMemset(c->d_bzero, 0, (nbc / SCAN_GROUP + 2) * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_blk_item, nbc * sizeof(uint32_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_item_fail, nic * sizeof(unsigned long long)));
    HIP_OK(c, hipMalloc((void **)&c->d_item_res, 3 * nic * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_bitem_offs, (nic + 1) * sizeof(uint64_t)));
    HIP_OK(c, hipHostMalloc((void **)&c->h_item_res, 3 * nic * sizeof(uint64_t), hipHostMallocDefault));
    HIP_OK(c, hipDeviceSynchronize());
    c->bws_blocks = nbc;
    c->bws_items = nic;
    return HUFE_OK;
}

static int ensure_range_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nranges)
{
    if (!c->d_rcounters) HIP_OK(c, hipMalloc((void **)&c->d_rcounters, 8 * sizeof(unsigned long long)));
    if (nblocks <= c->rws_blocks && nranges <= c->rws_ranges) return HUFE_OK;
    HIP_OK(c, hipDeviceSynchronize());
    const uint64_t nbc = (nblocks > c->rws_blocks ? nblocks + nblocks / 8 : c->rws_blocks) + 16;
    const uint64_t nrc = (nranges > c->rws_ranges ? nranges + nranges / 8 : c->rws_ranges) + 16;
    free_range_ws(c);
    HIP_OK(c, hipMalloc((void **)&c->d_rcover, nbc * sizeof(unsigned long long)));
    HIP_OK(c, hipMalloc((void **)&c->d_rrel, nbc * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_rtpairs, nbc * sizeof(unsigned long long)));
    HIP_OK(c, hipMalloc((void **)&c->d_rplan, 4 * nrc * sizeof(uint64_t)));
    HIP_OK(c, hipMalloc((void **)&c->d_rflag, nrc * sizeof(uint32_t)));
    c->rws_blocks = nbc;
    c->rws_ranges = nrc;
    return HUFE_OK;
}

/* sized by bounds the host knows - the blocks, records x the parts a record can have - and doubled when they grow */
static int ensure_gather_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nparts)
{
    if (!c->d_gtotal) HIP_OK(c, hipMalloc((void **)&c->d_gtotal, sizeof(uint64_t)));
    if (nblocks > c->gws_blocks) {
        HIP_OK(c, hipDeviceSynchronize());
        const uint64_t cap = (nblocks > 2 * c->gws_blocks ? nblocks : 2 * c->gws_blocks) + 16;
        free_gather_ws(c, 1);
        HIP_OK(c, hipMalloc((void **)&c->d_gcnt, 2 * cap * sizeof(uint32_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_glist, cap * sizeof(uint32_t)));
        const int rc = alloc_two_level(c, &c->gat_scan, cap, false);
        if (rc) return rc;
        c->gws_blocks = cap;
    }
    if (nparts > c->gws_parts) {
        HIP_OK(c, hipDeviceSynchronize());
        const uint64_t cap = (nparts > 2 * c->gws_parts ? nparts : 2 * c->gws_parts) + 16;
        free_gather_ws(c, 2);
        HIP_OK(c, hipMalloc(&c->d_gparts, cap * sizeof(GatherPart)));
        c->gws_parts = cap;
    }
    return HUFE_OK;
}

/* sized by the layout - mask words and tiles of all blocks - and doubled when they grow */
static int ensure_find_ws(hufgpu_ctx *c, uint64_t nwords, uint64_t ntiles)
{
    if (nwords > c->fws_words) {
        HIP_OK(c, hipDeviceSynchronize());
        const uint64_t cap = (nwords > 2 * c->fws_words ? nwords : 2 * c->fws_words) + 16;
        free_find_ws(c, 1);
        HIP_OK(c, hipMalloc((void **)&c->d_fbitmap, cap * sizeof(uint32_t)));
        c->fws_words = cap;
    }
    if (ntiles > c->fws_tiles) {
        HIP_OK(c, hipDeviceSynchronize());
        const uint64_t cap = (ntiles > 2 * c->fws_tiles ? ntiles : 2 * c->fws_tiles) + 16;
        free_find_ws(c, 2);
        HIP_OK(c, hipMalloc((void **)&c->d_ftcnt, cap * sizeof(uint32_t)));
        const int rc = alloc_two_level(c, &c->find_scan, cap, false);
        if (rc) return rc;
        c->fws_tiles = cap;
    }
    return HUFE_OK;
}

static int ensure_update_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t npieces)
{
    if (!c->d_ucount) HIP_OK(c, hipMalloc((void **)&c->d_ucount, UPD_WORDS * sizeof(unsigned long long)));
    if (nblocks > c->uws_blocks) {
        HIP_OK(c, hipDeviceSynchronize());
        free_update_ws(c, 1);
        const uint64_t cap = nblocks + nblocks / 8 + 16;
        HIP_OK(c, hipMalloc((void **)&c->d_urow_of, cap * sizeof(uint32_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_urow_blk, cap * sizeof(uint32_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_upairs, 2 * cap * sizeof(uint64_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_unew, (cap + 1) * sizeof(uint64_t)));
        c->uws_blocks = cap;
    }
    if (npieces > c->uws_pieces) {
        HIP_OK(c, hipDeviceSynchronize());
        free_update_ws(c, 2);
        const uint64_t cap = npieces + npieces / 8 + 16;
        HIP_OK(c, hipMalloc((void **)&c->d_upiece, cap * sizeof(uint32_t)));
        c->uws_pieces = cap;
    }
    return HUFE_OK;
}

static int ensure_sub_build_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nchunks)
{
    if (!c->d_sb_unbuilt) HIP_OK(c, hipMalloc((void **)&c->d_sb_unbuilt, sizeof(unsigned long long)));
    if (nblocks > c->sbws_blocks) {
        HIP_OK(c, hipDeviceSynchronize());
        free_sub_build_ws(c, 1);
        const uint64_t cap = nblocks + nblocks / 8 + 16;
        HIP_OK(c, hipMalloc((void **)&c->d_sb_state, cap * sizeof(uint32_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_sb_pay, cap * sizeof(uint64_t)));
        c->sbws_blocks = cap;
    }
    if (nchunks > c->sbws_chunks) {
        HIP_OK(c, hipDeviceSynchronize());
        free_sub_build_ws(c, 2);
        const uint64_t cap = nchunks + nchunks / 8 + 16;
        HIP_OK(c, hipMalloc((void **)&c->d_sb_chunk_tot, cap * sizeof(uint64_t)));
        HIP_OK(c, hipMalloc((void **)&c->d_sb_chunk_bits, cap * sizeof(uint64_t)));
        c->sbws_chunks = cap;
    }
    return HUFE_OK;
}

static inline hipStream_t pick_stream(hufgpu_ctx *c, void *stream) { (void)c; return (hipStream_t)stream; }
static inline unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

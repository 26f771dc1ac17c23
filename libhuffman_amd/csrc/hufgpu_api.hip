/*
 * hufgpu_api.hip - host side of the device-resident C ABI (include/huffman_gpu.h).
 *
 * Owns the per-device context (stream, workspace in HBM, pinned result words) and launches the
 * kernels of hufgpu_kernels.hip.  No CPU implementation of the codec lives here: if HIP or a
 * gfx950 device is unavailable every entry point fails with HUF_ERROR_FATAL and says why.
 */
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/huffman_gpu.h"
#include "hufgpu_common.h"
#include "hufgpu_kernels.hip"

using namespace hufgpu;

#ifndef HIST_THREADS
#define HIST_THREADS 256
#endif
#define PACK_THREADS 256
#ifndef DSUB_THREADS
#define DSUB_THREADS 256      /* decode_sub_kernel: four waves a workgroup, eight wave tiles a wave - a workgroup's table build is paid once per 64 KiB */
#endif
#ifndef DEC_THREADS
#define DEC_THREADS 512
#endif
#define SCAN_THREADS 1024
#define MAX_STAGES 8
#define PROF_SLOTS 256
#define PROF_ENCODE 0
#define PROF_DECODE 1

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

extern "C" uint64_t hufgpu_block_count(uint64_t n, uint64_t blocksize)
{
    if (n == 0) return 0;
    if (blocksize == 0) blocksize = n;            /* src/encoder.c:163-165 */
    return (n + blocksize - 1) / blocksize;
}

extern "C" uint64_t hufgpu_encode_bound(uint64_t n, uint64_t blocksize)
{
    /* per block: 10 + 2*1025 header; payload <= 9 bits per byte (an optimal prefix code never
     * costs more than the 8-bit fixed code, plus the wrap-root bit), +1 byte of padding */
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    return nb * (HUF_HEADER_FIXED + 2ull * HUF_TREE_MAX + 1) + (n * 9 + 7) / 8 + 16;
}

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

static void free_two_level(TwoLevel *t);

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

static inline hipStream_t pick_stream(hufgpu_ctx *c, void *stream) { (void)c; return (hipStream_t)stream; }

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

static int check_block_args(hufgpu_ctx *c, uint64_t n, uint64_t *blocksize)
{
    if (*blocksize == 0) *blocksize = n;
    if (*blocksize > HUFGPU_MAX_BLOCK) {
        set_err(c, "blocksize %llu exceeds the kernel limit of %llu bytes", (unsigned long long)*blocksize,
                (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUFE_ARGUMENT;
    }
    return HUFE_OK;
}

extern "C" int hufgpu_histogram(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                                uint32_t *d_hist, void *stream)
{
    if (!ctx || (!d_in && n) || !d_hist) return HUFE_ARGUMENT;
    if (n == 0) return HUFE_OK;
    int rc = check_block_args(ctx, n, &blocksize);
    if (rc) return rc;
    if (blocksize > 0xffffffffull) {
        set_err(ctx, "hufgpu_histogram returns 32-bit counts: blocks of 2^32 bytes and more are not taken");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    hist256_kernel<HIST_THREADS><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>((const uint8_t *)d_in, n, blocksize, d_hist);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

/* where the two arrays of a sub-index live inside the caller's buffer */
static HufSubIndex sub_index_view(void *d_sub, uint64_t n, uint64_t blocksize)
{
    HufSubIndex v;
    memset(&v, 0, sizeof(v));
    if (!d_sub || n == 0) return v;
    if (blocksize == 0) blocksize = n;
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    v.gpb = ((blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;   /* rows of 16-byte multiples */
    v.tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    v.tile_bits = (uint64_t *)d_sub;
    v.group_bits = (uint16_t *)((uint64_t *)d_sub + nb * v.tpb);
    v.lens = (uint8_t *)(v.group_bits + nb * v.gpb);        /* gpb is a multiple of 8: 16-byte aligned */
    return v;
}

extern "C" uint64_t hufgpu_sub_index_bytes(uint64_t n, uint64_t blocksize)
{
    if (n == 0) return 0;
    if (blocksize == 0) blocksize = n;
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    const uint64_t gpb = ((blocksize + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP + 7) & ~7ull;
    const uint64_t tpb = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    return nb * tpb * sizeof(uint64_t) + nb * gpb * sizeof(uint16_t) + nb * HUF_NSYM;
}

static int encode_impl(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                       void *d_out, uint64_t out_cap, uint64_t *d_block_offsets, void *d_sub_index,
                       uint64_t *out_len, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (n == 0) {                                  /* src/encoder.c:288: nothing to do */
        if (out_len) *out_len = 0;
        if (d_block_offsets) {                     /* the index of an empty stream: its length, 0 */
            HIP_OK(ctx, hipSetDevice(ctx->device));
            HIP_OK(ctx, hipMemsetAsync(d_block_offsets, 0, sizeof(uint64_t), pick_stream(ctx, stream)));
        }
        return HUFE_OK;
    }
    if (!d_in || !d_out) return HUFE_ARGUMENT;
    int rc = check_block_args(ctx, n, &blocksize);
    if (rc) return rc;
    if (out_cap < hufgpu_encode_bound(n, blocksize)) {
        set_err(ctx, "output capacity %llu below hufgpu_encode_bound() = %llu", (unsigned long long)out_cap,
                (unsigned long long)hufgpu_encode_bound(n, blocksize));
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    const uint64_t nb = hufgpu_block_count(n, blocksize);
    if (nb > 0x7fffffffull) {
        set_err(ctx, "too many blocks (%llu)", (unsigned long long)nb);
        return HUFE_ARGUMENT;
    }
    rc = ensure_encode_ws(ctx, nb);
    if (rc) return rc;
    hipStream_t s = pick_stream(ctx, stream);
    uint64_t *offs = d_block_offsets ? d_block_offsets : ctx->d_offsets;
    const uint8_t *in = (const uint8_t *)d_in;
    if (d_sub_index && ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "the sub-index buffer must be 8-byte aligned");
        return HUFE_ARGUMENT;
    }
    const HufSubIndex sub = sub_index_view(d_sub_index, n, blocksize);

    STAGE_BEGIN(ctx, s, PROF_ENCODE);
    TwoLevel sizes = ctx->enc_sizes;
    static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;   /* (measurements: the one-launch form) */
    if (blocksize < HUF_CHUNKED_FROM) {
        /* counts, tree and the sums of the encoded sizes in one launch (the profile's "tree" and
         * "scan_sizes" stages are then empty) */
        sizes.total = offs + nb;
        if (blocksize >= HL_MIN_BLOCK && !fused_only) {
            /* counts with lane-private counters at the rate HBM delivers, then the trees as a launch of their
             * own (kernels/hist_lanes.hpp): 0.19 + 0.13 ms per GiB on zipf255 where the fused kernel takes 0.44 */
            hist_lanes_kernel<HL_THREADS><<<dim3((unsigned)nb), dim3(HL_THREADS), 0, s>>>(in, n, blocksize, ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_wave_kernel<<<dim3((unsigned)nb), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
        } else
        if (blocksize <= HT_PACKED_MAX_BLOCK)
            hist_tree_kernel<HIST_THREADS, true><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        else
            hist_tree_kernel<HIST_THREADS, false><<<dim3((unsigned)nb), dim3(HIST_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        if (!(blocksize >= HL_MIN_BLOCK && !fused_only)) {
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
            STAGE_MARK(ctx, s);
        }
    } else {
        /* blocks of HUF_BIG_BLOCK bytes and more are cut into chunks, one workgroup each (blocksize = 0:
         * the whole input is ONE block, src/encoder.c:163-165 - the reference's default) */
        const uint64_t cpb = (blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS;
        const uint64_t nchunks = nb * cpb;
        if (nchunks > 0x7fffffffull) return HUFE_ARGUMENT;
        rc = ensure_chunk_ws(ctx, nchunks);
        if (rc) return rc;
        ChunkGeom geo;
        geo.n = n;
        geo.blocksize = blocksize;
        geo.cpb = (uint32_t)cpb;
        chunk_hist_kernel<HL_THREADS><<<dim3((unsigned)nchunks), dim3(HL_THREADS), 0, s>>>(in, geo, ctx->d_chunk_hist);
        if (blocksize < HUF_BIG_BLOCK) {
            /* rates below 2^23: the wave-per-block tree with 32-bit keys (its sums of the encoded sizes are not used
             * here: scan_sizes_kernel writes the index below) */
            sizes.total = offs + nb;
            block_hist32_kernel<<<dim3((unsigned)nb), dim3(HUF_NSYM), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_wave_kernel<<<dim3((unsigned)nb), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
        } else {
            block_hist_kernel<<<dim3((unsigned)nb), dim3(HUF_NSYM), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, (uint64_t *)ctx->d_hist);
            STAGE_MARK(ctx, s);
            tree_kernel<uint64_t, uint64_t><<<dim3((unsigned)nb), dim3(64), 0, s>>>((const uint64_t *)ctx->d_hist, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta);
        }
        STAGE_MARK(ctx, s);
        scan_sizes_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ctx->d_meta, nb, offs);
        chunk_total_kernel<<<dim3((unsigned)nchunks), dim3(64), 0, s>>>(ctx->d_chunk_hist, (uint32_t)cpb, ctx->d_codetab, ctx->d_meta, ctx->d_chunk_tot);
        chunk_scan_kernel<SCAN_THREADS><<<dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s>>>(ctx->d_chunk_tot, (uint32_t)cpb, ctx->d_chunk_bits);
        STAGE_MARK(ctx, s);
        sizes.local = NULL;              /* pack reads the finished index */
        PackChunk ck;
        ck.chunk_bits = ctx->d_chunk_bits;
        ck.chunk_syms = HUF_CHUNK_SYMS;
        ck.cpb = (uint32_t)cpb;
        pack_chunk_kernel<PACK_THREADS, false><<<dim3((unsigned)nchunks), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub, ck);
    }
    if (blocksize >= HUF_CHUNKED_FROM) {
        /* (packed above) */
    } else if (blocksize <= 121392ull)   /* deepest possible code <= 24 bits: 32-bit code path only */
        pack_kernel<PACK_THREADS, true><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
    else
        pack_kernel<PACK_THREADS, false><<<dim3((unsigned)nb), dim3(PACK_THREADS), 0, s>>>(in, n, blocksize, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offs, sizes, (uint8_t *)d_out, sub);
    STAGE_MARK(ctx, s);
    HIP_OK(ctx, hipGetLastError());

    if (out_len) {
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, offs + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        *out_len = ctx->h_result[0];
    }
    return HUFE_OK;
}

extern "C" int hufgpu_encode(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                             void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                             uint64_t *out_len, void *stream)
{
    return encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, d_block_offsets, NULL, out_len, stream);
}

extern "C" int hufgpu_encode_sub(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                                 void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                                 void *d_sub_index, uint64_t *out_len, void *stream)
{
    return encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, d_block_offsets, d_sub_index, out_len, stream);
}

static int decode_chain(hufgpu_ctx *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint8_t *out,
                        uint64_t out_cap, int max_tree, hipStream_t s, uint64_t *raw, uint64_t *used,
                        uint64_t *good_used, uint64_t *good_raw);

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

/* One small encode with ONE synchronisation (include/huffman_gpu.h): input from pinned host memory, the stream and its
 * length back into pinned host memory.  A call through the general entry points waits three times (input up, the length,
 * the stream back); for inputs of a few KiB those waits are most of the call. */
extern "C" int hufgpu_encode_small(hufgpu_ctx_t *ctx, const void *h_in_pinned, uint64_t n, uint64_t blocksize, void *d_in,
                                   void *d_out, uint64_t out_cap, void *h_out_pinned, uint64_t h_out_cap, uint64_t *out_len)
{
    if (!ctx || !h_in_pinned || !d_in || !d_out || !h_out_pinned || !out_len || n == 0) return HUFE_ARGUMENT;
    const uint64_t bound = hufgpu_encode_bound(n, blocksize);
    const uint64_t len_at = (bound + 7u) & ~7ull;
    if (h_out_cap < len_at + 8u || out_cap < bound) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIP_OK(ctx, hipMemcpyAsync(d_in, h_in_pinned, n, hipMemcpyHostToDevice, s));
    const int rc = encode_impl(ctx, d_in, n, blocksize, d_out, out_cap, NULL, NULL, NULL, (void *)s);
    if (rc != HUFE_OK) return rc;
    const uint64_t nb = hufgpu_block_count(n, blocksize ? blocksize : n);
    HIP_OK(ctx, hipMemcpyAsync(h_out_pinned, d_out, bound, hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipMemcpyAsync((char *)h_out_pinned + len_at, ctx->d_offsets + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    *out_len = *(const uint64_t *)((const char *)h_out_pinned + len_at);
    return (*out_len <= bound) ? HUFE_OK : HUFE_FATAL;
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

/* How the last hufgpu_decode_ranges routed its blocks (include/huffman_gpu.h): host values, no GPU is touched. */
extern "C" int hufgpu_ranges_counters(hufgpu_ctx_t *ctx, uint64_t counters[8])
{
    if (!ctx || !counters) return HUFE_ARGUMENT;
    memcpy(counters, ctx->rcounters, sizeof(ctx->rcounters));
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
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    const uint8_t *st = (const uint8_t *)d_stream;

    STAGE_BEGIN(ctx, s, PROF_DECODE);
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    /* header parse + two-level sums of the block lengths; also (re)initialises result[1] and [2] */
    TwoLevel lens = ctx->dec_lens;
    lens.total = (uint64_t *)res + 1;
    lens.total2 = ctx->d_out_offsets + nblocks;
    lens.min_out = (uint64_t *)res + 2;
    decode_prepare_kernel<<<dim3((unsigned)((nblocks + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, d_block_offsets, nblocks, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);
    STAGE_MARK(ctx, s);
    if (sub && sub->tile_bits) {
        /* the encoder's sub-index: one table pass per symbol, verified; what cannot be verified is
         * decoded again by the self-synchronising decoder (decode_fix_kernel) */
        const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
        if (nblocks * cpb > 0x7fffffffull) return HUFE_ARGUMENT;
        DecFixList fix;
        fix.count = ctx->d_fix_count;
        fix.blocks = ctx->d_fix_blocks;
        fix.flag = ctx->d_fix_flag;
        decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)(nblocks * cpb)), dim3(DSUB_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, lens, (uint8_t *)d_out, out_cap, ctx->d_status, res, *sub, blocksize, (uint32_t)cpb, fix);
        const unsigned fix_grid = (unsigned)(nblocks < 1024 ? nblocks : 1024);
        decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, lens, (uint8_t *)d_out, out_cap, ctx->d_status, res, fix);
    } else {
        static const bool exact_only = getenv("HUF_GPU_EXACT_DECODE") && atoi(getenv("HUF_GPU_EXACT_DECODE")) != 0;   /* (measurements: the exact decoder for every block) */
        if (exact_only) {
            decode_kernel<DEC_THREADS><<<dim3((unsigned)nblocks), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, lens, (uint8_t *)d_out, out_cap, ctx->d_status, res);
        } else {
            /* the lean self-synchronising decoder (kernels/decode_fast.hpp); what it cannot vouch for - a damaged
             * stream, an unusual tree - is decoded again by the exact one, which also reports the reference's error */
            DecFixList fix;
            fix.count = ctx->d_fix_count;
            fix.blocks = ctx->d_fix_blocks;
            fix.flag = ctx->d_fix_flag;
            const unsigned fix_grid = (unsigned)(nblocks < 1024 ? nblocks : 1024);
            DecodeFastArgs fa;
            fa.stream = st; fa.stream_len = stream_len; fa.offsets = d_block_offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
            fa.lens = lens; fa.out = (uint8_t *)d_out; fa.out_cap = out_cap; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
            decode_fast_kernel<DEC_THREADS><<<dim3((unsigned)nblocks), dim3(DEC_THREADS), 0, s>>>(fa);
            decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, lens, (uint8_t *)d_out, out_cap, ctx->d_status, res, fix);
        }
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
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
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

/* Leading blocks of HUF_BIG_BLOCK symbols and more (blocksize = 0 makes the whole input ONE block,
 * src/encoder.c:163-165): one workgroup per block would leave the device idle, so a sub-index is
 * built for each such block (kernels/spec_index.hpp) and decode_sub_kernel decodes - and verifies -
 * it chunk by chunk.  Stops at the first block this does not apply to or does not work for; the
 * caller's general path takes over at *pos / *rawpos and reports whatever is wrong there. */
static int decode_big_blocks(hufgpu_ctx *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint8_t *out,
                             uint64_t out_cap, uint32_t flags, hipStream_t s, void *stream, uint64_t *pos_io,
                             uint64_t *rawpos_io)
{
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    uint64_t pos = *pos_io, rawpos = *rawpos_io;
    if (!ctx->d_big_offs) HIP_OK(ctx, hipMalloc((void **)&ctx->d_big_offs, (SPEC_WORDS + 2) * sizeof(uint64_t)));
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
        if (sub_bytes > ctx->big_sub_bytes) {
            free_big_ws(ctx, 4);
            if (hipMalloc(&ctx->d_big_sub, sub_bytes) != hipSuccess) { (void)hipGetLastError(); ctx->d_big_sub = NULL; break; }
            ctx->big_sub_bytes = sub_bytes;
        }
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
            if (nlanes > ctx->big_lanes) {
                free_big_ws(ctx, 1);
                const uint64_t cap = nlanes + nlanes / 8 + 16;
                if (hipMalloc((void **)&ctx->d_big_entry, cap * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_exit, cap * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_pre, (cap + 1) * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_wgpre, (cap / DEC_THREADS + 4) * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_wgscratch, (cap / DEC_THREADS + 4) * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_first_pos, cap * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_first_g, cap * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_last_pos, cap * sizeof(uint64_t)) != hipSuccess ||
                    hipMalloc((void **)&ctx->d_big_cnt, cap * sizeof(uint32_t)) != hipSuccess) {
                    (void)hipGetLastError();
                    free_big_ws(ctx, 1);
                    break;
                }
                ctx->big_lanes = cap;
            }
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

static int decode_stream_general(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                                 void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                                 uint64_t *consumed, void *stream);

static int discover_chain(hufgpu_ctx_t *ctx, const uint8_t *st, uint64_t avail, uint64_t length, uint64_t scan_len, int max_tree,
                          uint8_t *out, uint64_t out_cap, hipStream_t s, uint64_t *m_out, uint64_t *resume_out,
                          bool *complete_out, uint64_t *in_place_out);

/* The block index of a raw stream without decoding it into anything: see include/huffman_gpu.h. */
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

extern "C" int hufgpu_block_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length, uint32_t flags,
                                  const uint64_t **d_index, uint64_t *nblocks, uint64_t *consumed, void *stream)
{
    if (!ctx || !d_index || !nblocks || !consumed) return HUFE_ARGUMENT;
    *d_index = NULL; *nblocks = 0; *consumed = 0;
    if (length == 0) return HUFE_OK;
    if (!d_stream || ((uintptr_t)d_stream & 15u)) return HUFE_ARGUMENT;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
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

extern "C" int hufgpu_decode_stream(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                                    void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                                    uint64_t *consumed, void *stream)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (raw_len) *raw_len = 0;
    if (consumed) *consumed = 0;
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
    const uint64_t nwg = (scan_len + DISC_CHUNK - 1) / DISC_CHUNK;
    const uint64_t ngroups = (nwg + DISC_SCAN_GROUP - 1) / DISC_SCAN_GROUP;
    if (nwg > ctx->disc_wgs) {
        HIP_OK(ctx, hipStreamSynchronize(s));
        free_disc_ws(ctx, 1);
        const uint64_t cap = nwg + nwg / 8 + 16;
        const uint64_t gcap = (cap + DISC_SCAN_GROUP - 1) / DISC_SCAN_GROUP + 1;
        HIP_OK(ctx, hipMalloc((void **)&ctx->d_wg_counts, cap * sizeof(uint32_t)));
        HIP_OK(ctx, hipMalloc((void **)&ctx->d_wg_base, (cap + 1 + 2 * gcap) * sizeof(uint64_t)));     /* local sums, then the groups' bases and totals */
        HIP_OK(ctx, hipMalloc((void **)&ctx->d_disc_masks, cap * DISC_THREADS * sizeof(uint64_t)));
        HIP_OK(ctx, hipMalloc((void **)&ctx->d_disc_slots, cap * DISC_SLOTS * sizeof(DiscSlot)));
        ctx->disc_wgs = cap;
    }
    uint64_t *const group_base = ctx->d_wg_base + ctx->disc_wgs + 1;
    uint64_t *const group_total = group_base + (ctx->disc_wgs + DISC_SCAN_GROUP - 1) / DISC_SCAN_GROUP + 1;
    /* Round 6: ONE wait per call.  Everything that needs the number of candidates - the probes' launch, the sums, the links,
     * the walk - reads it on the device (ctx->d_walk, DISC_NCAND) and is launched as wide as the candidate arrays are:
     * surplus workgroups leave at once.  Only when there are no arrays yet (the context's first raw stream), or when the
     * stream turns out to hold more candidates than they take (the walk's result says so), does the host wait for the
     * count, make room and go again - what every call did until round 5. */
    for (int attempt = 0; attempt < 2; attempt++) {
        HIP_OK(ctx, hipMemsetAsync(ctx->d_walk, 0, DISC_WORDS * sizeof(uint64_t), s));
        discover_kernel<<<dim3((unsigned)nwg), dim3(DISC_THREADS), 0, s>>>(st, avail, scan_len, max_tree, ctx->d_wg_counts, (DiscSlot *)ctx->d_disc_slots, ctx->d_disc_masks);
        scan_counts_kernel<SCAN_THREADS><<<dim3((unsigned)ngroups), dim3(SCAN_THREADS), 0, s>>>(ctx->d_wg_counts, nwg, ctx->d_wg_base, group_base, group_total, ctx->d_walk, ctx->disc_cands);
        HIP_OK(ctx, hipGetLastError());
        if (ctx->disc_cands == 0 || attempt == 1) {
            HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_walk + DISC_FOUND, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_OK(ctx, hipStreamSynchronize(s));
            const uint64_t found = ctx->h_result[0];
            if (found == 0 || found >= 0x7fffffffull) return HUFE_OK;
            if (found > ctx->disc_cands) {
                free_disc_ws(ctx, 2);
                const uint64_t cap = found + found / 8 + 16;
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_cand, cap * sizeof(uint64_t)));
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_cand_end, cap * sizeof(uint64_t)));
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_chain, (cap + 1) * sizeof(uint64_t)));
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_cand_status, cap * sizeof(int32_t)));
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_nxt, cap * sizeof(uint32_t)));
                HIP_OK(ctx, hipMalloc((void **)&ctx->d_spec_off, (cap + 1) * sizeof(uint64_t)));
                ctx->disc_cands = cap;
            }
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
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result, ctx->d_walk, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        if (ctx->h_result[DISC_FOUND] > width) continue;                 /* more candidates than the arrays took: once more, with room */
        *m_out = ctx->h_result[0];
        *in_place_out = ctx->h_result[4];   /* bytes the probe already decoded into `out` for these m blocks */
        *complete_out = ctx->h_result[2] != 0;
        *resume_out = *complete_out ? ctx->h_result[3] : ctx->h_result[1];
        return HUFE_OK;
    }
    return HUFE_OK;
}

static int decode_stream_general(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                                 void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                                 uint64_t *consumed, void *stream)
{
    hipStream_t s = pick_stream(ctx, stream);
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
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

extern "C" int hufgpu_decode_stream_complete(hufgpu_ctx_t *ctx, uint64_t *raw_len, uint64_t *consumed)
{
    if (!ctx) return HUFE_ARGUMENT;
    if (raw_len) *raw_len = ctx->complete_raw;
    if (consumed) *consumed = ctx->complete_used;
    return HUFE_OK;
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

extern "C" int hufgpu_ctx_device(const hufgpu_ctx_t *ctx) { return ctx ? ctx->device : -1; }

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

/* ======================================================================================
 * Batches: many independent inputs in one launch sequence (include/huffman_gpu.h, kernels/batch.hpp)
 * ==================================================================================== */

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
    if (words > c->bstage_words) {
        HIP_OK(c, hipDeviceSynchronize());          /* (kernels of an earlier batch may still read the device copy) */
        free_batch_stage(c);
        const uint64_t cap = words + words / 4 + 64;
        HIP_OK(c, hipHostMalloc((void **)&c->h_bstage, cap * sizeof(uint64_t), hipHostMallocDefault));
        HIP_OK(c, hipMalloc((void **)&c->d_bstage, cap * sizeof(uint64_t)));
        c->bstage_words = cap;
    }
    *h = c->h_bstage;
    return HUFE_OK;
}

static int batch_upload(hufgpu_ctx *c, uint64_t words, hipStream_t s)
{
    HIP_OK(c, hipMemcpyAsync(c->d_bstage, c->h_bstage, words * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_OK(c, hipEventRecord(c->bstage_ev, s));
    c->bstage_pending = 1;
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

static inline unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

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

    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    const uint8_t *st = (const uint8_t *)d_stream;
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    TwoLevel lens = ctx->dec_lens;
    lens.total = (uint64_t *)res + 1;
    lens.total2 = ctx->d_out_offsets + nb;
    lens.min_out = (uint64_t *)res + 2;
    decode_prepare_kernel<<<dim3((unsigned)((nb + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, d_block_offsets, nb, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);

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
    DecFixList fix;
    fix.count = ctx->d_fix_count;
    fix.blocks = ctx->d_fix_blocks;
    fix.flag = ctx->d_fix_flag;
    const unsigned fix_grid = (unsigned)(nb < 1024 ? nb : 1024);
    if (d_sub_index) {
        const HufSubIndex sub = sub_index_rows((void *)d_sub_index, nb, row_blocksize);
        decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)(nb * cpb)), dim3(DSUB_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, blens, (uint8_t *)d_out, out_end, ctx->d_status, res, sub, row_blocksize, (uint32_t)cpb, fix);
    } else {
        DecodeFastArgs fa;
        fa.stream = st; fa.stream_len = stream_len; fa.offsets = d_block_offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
        fa.lens = blens; fa.out = (uint8_t *)d_out; fa.out_cap = out_end; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
        decode_fast_kernel<DEC_THREADS><<<dim3((unsigned)nb), dim3(DEC_THREADS), 0, s>>>(fa);
    }
    decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, blens, (uint8_t *)d_out, out_end, ctx->d_status, res, fix);
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

/* ======================================================================================
 * Byte ranges of the original data out of one indexed stream (include/huffman_gpu.h, kernels/ranges.hpp)
 * ==================================================================================== */

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
    uint64_t cpb = 0;
    if (d_sub_index) {
        if (blocksize == 0) blocksize = raw_size;
        cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
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

    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    const uint8_t *st = (const uint8_t *)d_stream;
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    TwoLevel lens = ctx->dec_lens;
    lens.total = (uint64_t *)res + 1;
    lens.total2 = ctx->d_out_offsets + nb;
    lens.min_out = (uint64_t *)res + 2;
    decode_prepare_kernel<<<dim3((unsigned)((nb + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, d_block_offsets, nb, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);

    DecRangeArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.range_lo = ctx->d_bstage;
    ra.range_hi = ctx->d_bstage + nranges;
    ra.out_offsets = ctx->d_bstage + 2 * nranges;
    ra.nranges = nranges;
    ra.nblocks = nb;
    ra.dmeta = ctx->d_dmeta;
    ra.status = ctx->d_status;
    ra.lens = lens;
    ra.first_bad = res + 2;
    ra.bprefix = ctx->d_bprefix;
    ra.obase = ctx->d_bobase;
    ra.cover = ctx->d_rcover;
    ra.rel = ctx->d_rrel;
    ra.kind = ctx->d_blk_item;
    ra.rplan = ctx->d_rplan;
    ra.rflag = ctx->d_rflag;
    ra.counters = ctx->d_rcounters;
    ra.range_fail = ctx->d_item_fail;
    ra.range_res = ctx->d_item_res;
    ra.dout = (uint8_t *)d_out;
    if (tiles) {
        ra.tpairs = ctx->d_rtpairs;
        ra.raw_size = raw_size;
        ra.blocksize = blocksize;
    }
    drange_plan_kernel<<<dim3(grid256((nb + 1 > nranges ? nb + 1 : nranges))), dim3(256), 0, s>>>(ra);
    /* a few long ranges: several workgroups a range walk its blocks; many ranges are parallel enough as they are */
    const unsigned mark_y = nranges >= 64 ? 1u : (unsigned)(nb / 2048 < 1 ? 1 : (nb / 2048 > 16 ? 16 : nb / 2048));
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
    DecFixList fix;
    fix.count = ctx->d_fix_count;
    fix.blocks = ctx->d_fix_blocks;
    fix.flag = ctx->d_fix_flag;
    const unsigned fix_grid = (unsigned)(nb < 1024 ? nb : 1024);
    if (ntiled) {
        /* one wave an item; a workgroup's eight waves take about four items each of a long range, so that the table build
         * it starts with is paid once per 32 tiles - the longest range, known here, bounds the tiles a range has in a block */
        uint64_t longest_range = 0;
        for (uint64_t i = 0; i < nranges; i++)
            if (range_hi[i] - range_lo[i] > longest_range) longest_range = range_hi[i] - range_lo[i];
        uint64_t tile_y = (longest_range / HUF_SUB_TILE + 2 + 31) / 32;
        if (tile_y > 1024) tile_y = 1024;
        RangeTileArgs ta;
        ta.stream = st;
        ta.stream_len = stream_len;
        ta.offsets = d_block_offsets;
        ta.sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
        drange_tiles_kernel<<<dim3((unsigned)nranges, (unsigned)tile_y), dim3(RTILE_THREADS), 0, s>>>(ra, ta);
    }
    /* (every touched block served by tiles: nothing for the block decoders to do) */
    const bool block_decoders = !(ntiled && nstaged == 0 && ndirect == 0);
    if (!block_decoders) {
    } else if (d_sub_index) {
        const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
        decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)(nb * cpb)), dim3(DSUB_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, blens, base, span, ctx->d_status, res, sub, blocksize, (uint32_t)cpb, fix);
    } else {
        DecodeFastArgs fa;
        fa.stream = st; fa.stream_len = stream_len; fa.offsets = d_block_offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
        fa.lens = blens; fa.out = base; fa.out_cap = span; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
        decode_fast_kernel<DEC_THREADS><<<dim3((unsigned)nb), dim3(DEC_THREADS), 0, s>>>(fa);
    }
    if (block_decoders)
        decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, blens, base, span, ctx->d_status, res, fix);
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

/* ======================================================================================
 * Records at device-resident positions (include/huffman_gpu.h, kernels/gather.hpp): enqueue-only
 * ==================================================================================== */

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

extern "C" int hufgpu_gather(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                             uint64_t nblocks, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                             uint64_t nrecords, const uint64_t *d_pos, const uint32_t *d_len, uint32_t max_len, void *d_out,
                             uint64_t out_stride, int32_t *d_errs, uint32_t *d_raw_lens, uint32_t flags, void *stream)
{
    if (nrecords == 0 || max_len == 0) return HUFE_OK;
    if (!d_stream || !d_block_offsets || !d_pos || !d_out || !d_errs) {
        set_err(ctx, "gather: the stream, its block index, d_pos, d_out and d_errs are required");
        return HUFE_ARGUMENT;
    }
    if (out_stride < max_len) {
        set_err(ctx, "gather: out_stride %llu is less than max_len %u", (unsigned long long)out_stride, max_len);
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(ctx, "gather: needs the stream's sub-index in an 8-byte aligned buffer");
        return HUFE_ARGUMENT;
    }
    if (blocksize == 0) blocksize = raw_size;
    if (raw_size == 0 || blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, blocksize) != nblocks || nblocks > 0x7fffffffull) {
        set_err(ctx, "gather: (raw_size, blocksize) must be those of the encode that wrote these %llu blocks", (unsigned long long)nblocks);
        return HUFE_ARGUMENT;
    }
    /* what the host knows of the records: how many, and how long at most - the parts a record can have, the tiles a part */
    uint64_t per_record = ((uint64_t)max_len + blocksize - 2) / blocksize + 1;
    if (per_record > nblocks) per_record = nblocks;
    const uint64_t nparts = nrecords > 0x7fffffffull ? ~0ull : nrecords * per_record;
    if (nparts > 0xffffffffull) {
        set_err(ctx, "gather: %llu records of up to %u bytes are more than 2^32 - 1 (record, block) parts", (unsigned long long)nrecords, max_len);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "gather: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const int rc = ensure_gather_ws(ctx, nblocks, nparts);
    if (rc) return rc;

    const uint64_t tiles_per_block = (blocksize + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
    uint64_t tmax = ((uint64_t)max_len + HUF_SUB_TILE - 2) / HUF_SUB_TILE + 1;
    if (tmax > tiles_per_block) tmax = tiles_per_block;
    /* The serving grid: no wider than the touched blocks can be, and a few workgroups a compute unit (three fit its LDS).
     * Where the stream has fewer blocks than that, a block's items are dealt to several workgroups - one item a wave,
     * as far as the grid goes: with blocksize = 0 every record lies in the one block. */
    const uint64_t width = 4ull * (uint64_t)ctx->cus;
    uint64_t shares = 1;
    if (nblocks < width) {
        shares = (nparts * tmax + GATHER_WAVES - 1) / GATHER_WAVES;
        if (shares > width / nblocks) shares = width / nblocks;
        if (shares < 1) shares = 1;
    }
    uint64_t grid = (nblocks < nparts ? nblocks : nparts) * shares;
    if (grid > width) grid = width;

    GatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.stream = (const uint8_t *)d_stream;
    ga.stream_len = stream_len;
    ga.offsets = d_block_offsets;
    ga.nblocks = nblocks;
    ga.sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
    ga.raw_size = raw_size;
    ga.bsize = blocksize;
    ga.max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    ga.max_len = max_len;
    ga.nrecords = nrecords;
    ga.pos = d_pos;
    ga.len = d_len;
    ga.out = (uint8_t *)d_out;
    ga.stride = out_stride;
    ga.errs = d_errs;
    ga.raw_lens = d_raw_lens;
    ga.cnt = ctx->d_gcnt;
    ga.cur = ctx->d_gcnt + nblocks;
    ga.scan = ctx->gat_scan;
    ga.scan.total = ctx->d_gtotal;
    ga.list = ctx->d_glist;
    ga.parts = (GatherPart *)ctx->d_gparts;
    ga.shares = (uint32_t)shares;
    ga.tmax = (uint32_t)tmax;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_gcnt, 0, 2 * nblocks * sizeof(uint32_t), s));
    gather_mark_kernel<<<dim3(grid256(nrecords)), dim3(256), 0, s>>>(ga);
    gather_scan_kernel<<<dim3((unsigned)((nblocks + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(ga);
    gather_place_kernel<<<dim3(grid256(nblocks > nrecords ? nblocks : nrecords)), dim3(256), 0, s>>>(ga);
    gather_serve_kernel<<<dim3((unsigned)grid), dim3(GATHER_THREADS), 0, s>>>(ga);
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

/* ======================================================================================
 * Byte ranges of the original data overwritten in one indexed stream (include/huffman_gpu.h, kernels/update.hpp)
 * ==================================================================================== */

/* Counts + trees, and pack, of a compact list of rows (kernels/update.hpp) by the kernels encode_impl picks for blocks
 * of `longest` bytes: every one is bit-exact, the route only decides speed.  hufgpu_update_ranges and hufgpu_append /
 * hufgpu_truncate share them, so the thresholds stand in one place. */
static void launch_pairs_trees(hufgpu_ctx *ctx, const uint8_t *base, uint64_t rows, uint64_t longest, const TwoLevel &sizes, hipStream_t s)
{
    static const bool fused_only = getenv("HUF_GPU_FUSED_HIST") && atoi(getenv("HUF_GPU_FUSED_HIST")) != 0;
    if (longest >= HL_MIN_BLOCK && !fused_only) {
        hist_lanes_pairs_kernel<HL_THREADS><<<dim3((unsigned)rows), dim3(HL_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_hist);
        tree_wave_kernel<<<dim3((unsigned)rows), dim3(64), 0, s>>>(ctx->d_hist, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    } else if (longest <= HT_PACKED_MAX_BLOCK) {
        hist_tree_pairs_kernel<HIST_THREADS, true><<<dim3((unsigned)rows), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    } else {
        hist_tree_pairs_kernel<HIST_THREADS, false><<<dim3((unsigned)rows), dim3(HIST_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, sizes);
    }
}

static void launch_pairs_pack(hufgpu_ctx *ctx, const uint8_t *base, uint64_t rows, uint64_t longest, uint64_t *offsets, uint64_t nblocks,
                              uint64_t out_cap, uint8_t *out, const HufSubIndex &sub, hipStream_t s)
{
    if (longest <= 121392ull)            /* deepest possible code <= 24 bits: 32-bit code path only, as in encode_impl */
        pack_pairs_kernel<PACK_THREADS, true><<<dim3((unsigned)rows), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub);
    else
        pack_pairs_kernel<PACK_THREADS, false><<<dim3((unsigned)rows), dim3(PACK_THREADS), 0, s>>>(base, ctx->d_upairs, ctx->d_urow_blk, ctx->d_codetab, ctx->d_treebuf, ctx->d_meta, offsets, nblocks, out_cap, out, sub);
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

static bool spans_overlap(const void *a, uint64_t an, const void *b, uint64_t bn)
{
    if (!a || !b || !an || !bn) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

struct UpdRangeOrder {
    uint64_t lo, hi, i;
};
static int upd_range_cmp(const void *a, const void *b)
{
    const UpdRangeOrder *x = (const UpdRangeOrder *)a, *y = (const UpdRangeOrder *)b;
    return x->lo < y->lo ? -1 : (x->lo > y->lo ? 1 : (x->i < y->i ? -1 : 1));
}

extern "C" int hufgpu_update_ranges(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                    const uint64_t *d_block_offsets, uint64_t nblocks, uint64_t nranges,
                                    const uint64_t *range_lo, const uint64_t *range_hi, const uint64_t *src_offsets,
                                    const void *d_src, const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                    void *d_out, uint64_t out_cap, uint64_t *d_out_block_offsets, void *d_out_sub_index,
                                    uint32_t flags, uint64_t *out_len, uint64_t *blocks_reencoded, void *stream)
{
    if (out_len) *out_len = 0;
    if (blocks_reencoded) *blocks_reencoded = 0;
    if (nranges > 0x7fffffffull || (nranges && (!range_lo || !range_hi))) {
        set_err(ctx, "update_ranges: range_lo and range_hi are required (at most 2^31 - 1 ranges)");
        return HUFE_ARGUMENT;
    }
    uint64_t nfull = 0, src_extent = 0, src_total = 0;
    for (uint64_t i = 0; i < nranges; i++) {
        if (range_lo[i] > range_hi[i]) {
            set_err(ctx, "update_ranges: range %llu ends in front of its start", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
        const uint64_t len = range_hi[i] - range_lo[i];
        if (len == 0) continue;
        nfull++;
        const uint64_t at = src_offsets ? src_offsets[i] : src_total;
        if (at + len < at) {
            set_err(ctx, "update_ranges: the new bytes of range %llu wrap around the address space", (unsigned long long)i);
            return HUFE_ARGUMENT;
        }
        if (at + len > src_extent) src_extent = at + len;
        src_total += len;
    }
    if (nfull > 1) {                                  /* an overwrite has one value per byte: the ranges must not overlap */
        UpdRangeOrder *ord = (UpdRangeOrder *)malloc(nfull * sizeof(UpdRangeOrder));
        if (!ord) return HUFE_MEMORY;
        uint64_t k = 0;
        for (uint64_t i = 0; i < nranges; i++)
            if (range_lo[i] < range_hi[i]) { ord[k].lo = range_lo[i]; ord[k].hi = range_hi[i]; ord[k].i = i; k++; }
        qsort(ord, nfull, sizeof(UpdRangeOrder), upd_range_cmp);
        for (k = 1; k < nfull; k++) {
            if (ord[k - 1].hi > ord[k].lo) {
                set_err(ctx, "update_ranges: ranges %llu and %llu overlap", (unsigned long long)ord[k - 1].i, (unsigned long long)ord[k].i);
                free(ord);
                return HUFE_ARGUMENT;
            }
        }
        free(ord);
    }
    uint64_t cpb = 0, sub_bytes = 0;
    if (d_sub_index || d_out_sub_index) {
        if (blocksize == 0) blocksize = raw_size;
        cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
        if ((((uintptr_t)d_sub_index | (uintptr_t)d_out_sub_index) & 7u) || raw_size == 0 ||
            hufgpu_block_count(raw_size, blocksize) != nblocks || nblocks * cpb > 0x7fffffffull) {
            set_err(ctx, "update_ranges: a sub-index needs an 8-byte aligned buffer and the (raw_size, blocksize) that give the layout of these %llu blocks",
                    (unsigned long long)nblocks);
            return HUFE_ARGUMENT;
        }
        if (d_out_sub_index && blocksize >= HUF_CHUNKED_FROM) {
            set_err(ctx, "update_ranges: a new sub-index needs blocks below %llu bytes", (unsigned long long)HUF_CHUNKED_FROM);
            return HUFE_ARGUMENT;
        }
        sub_bytes = hufgpu_sub_index_bytes(raw_size, blocksize);
    }
    if ((uintptr_t)d_out & 3u) {                      /* pack writes whole words of the destination, as in hufgpu_encode */
        set_err(ctx, "update_ranges: the output must be 4-byte aligned");
        return HUFE_ARGUMENT;
    }
    const uint64_t index_bytes = (nblocks + 1) * sizeof(uint64_t);
    if (spans_overlap(d_out, out_cap, d_stream, stream_len) || spans_overlap(d_out, out_cap, d_block_offsets, index_bytes) ||
        spans_overlap(d_out, out_cap, d_src, src_extent) || spans_overlap(d_out, out_cap, d_sub_index, sub_bytes) ||
        spans_overlap(d_out, out_cap, d_out_block_offsets, index_bytes) || spans_overlap(d_out, out_cap, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_block_offsets, index_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_src, src_extent) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_sub_index, sub_bytes) ||
        spans_overlap(d_out_block_offsets, index_bytes, d_out_sub_index, sub_bytes) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_sub_index, sub_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_stream, stream_len) ||
        spans_overlap(d_out_sub_index, sub_bytes, d_block_offsets, index_bytes) || spans_overlap(d_out_sub_index, sub_bytes, d_src, src_extent)) {
        set_err(ctx, "update_ranges: the output buffers overlap the input (the call works out of place) or one another");
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "update_ranges: needs a context (there is no CPU path)");
        return HUFE_ARGUMENT;
    }
    const uint64_t nb = nblocks;
    if (nb > 0x7fffffffull || (nb && stream_len && (!d_stream || !d_block_offsets)) || (stream_len && !d_out) || (src_total && !d_src)) {
        set_err(ctx, "update_ranges: the stream, its block index, the new bytes or the output is missing, or more than 2^31 - 1 blocks");
        return HUFE_ARGUMENT;
    }
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    ctx->last_stream = s;
    const uint8_t *st = (const uint8_t *)d_stream;

    if (nfull == 0) {                                 /* nothing to write: the stream, its index and its sub-index as they are */
        if (stream_len > out_cap) {
            set_err(ctx, "update_ranges: the stream of %llu bytes does not fit the output of %llu", (unsigned long long)stream_len, (unsigned long long)out_cap);
            return HUFE_MEMORY;
        }
        if (stream_len) HIP_OK(ctx, hipMemcpyAsync(d_out, d_stream, stream_len, hipMemcpyDeviceToDevice, s));
        if (d_out_block_offsets && d_block_offsets) HIP_OK(ctx, hipMemcpyAsync(d_out_block_offsets, d_block_offsets, index_bytes, hipMemcpyDeviceToDevice, s));
        if (d_out_sub_index && d_sub_index && nblocks && stream_len && d_block_offsets) {
            /* the rows as the general path copies them - the entries the encoder writes, nothing else: every block is a copy block */
            int rc0 = ensure_decode_ws(ctx, nblocks);
            if (!rc0) rc0 = ensure_batch_ws(ctx, nblocks, 1);
            if (rc0) return rc0;
            const int max_tree0 = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
            unsigned long long *res0 = (unsigned long long *)ctx->d_result;
            TwoLevel lens0 = ctx->dec_lens;
            lens0.total = (uint64_t *)res0 + 1;
            lens0.total2 = ctx->d_out_offsets + nblocks;
            lens0.min_out = (uint64_t *)res0 + 2;
            decode_prepare_kernel<<<dim3((unsigned)((nblocks + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, d_block_offsets, nblocks, max_tree0, ctx->d_dmeta, ctx->d_status, lens0, ctx->d_fix_count);
            upd_positions_kernel<<<dim3(grid256(nblocks + 1)), dim3(256), 0, s>>>(lens0, nblocks, ctx->d_bprefix, ctx->d_blk_item);
            const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize), to = sub_index_view(d_out_sub_index, raw_size, blocksize);
            upd_sub_rows_kernel<<<dim3((unsigned)nblocks), dim3(256), 0, s>>>(from, to, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
            HIP_OK(ctx, hipGetLastError());
        }
        HIP_OK(ctx, hipStreamSynchronize(s));
        if (out_len) *out_len = stream_len;
        return HUFE_OK;
    }
    if (nb == 0 || stream_len == 0) {
        set_err(ctx, "update_ranges: the stream holds no data, every range lies behind its end");
        return HUFE_ARGUMENT;
    }

    int rc = ensure_decode_ws(ctx, nb);
    if (rc) return rc;
    rc = ensure_batch_ws(ctx, nb, nranges);
    if (rc) return rc;
    rc = ensure_range_ws(ctx, nb, nranges);
    if (rc) return rc;
    rc = ensure_update_ws(ctx, nb, 0);
    if (rc) return rc;
    uint64_t *h = NULL;
    rc = batch_stage(ctx, 4 * nranges + 1, &h);
    if (rc) return rc;
    memcpy(h, range_lo, nranges * sizeof(uint64_t));
    memcpy(h + nranges, range_hi, nranges * sizeof(uint64_t));
    {
        uint64_t acc = 0;
        for (uint64_t i = 0; i < nranges; i++) {
            h[2 * nranges + i] = acc;                 /* the plan's slot check: every range has room for itself */
            h[3 * nranges + 1 + i] = src_offsets ? src_offsets[i] : acc;
            acc += range_hi[i] - range_lo[i];
        }
        h[3 * nranges] = acc;
    }
    rc = batch_upload(ctx, 4 * nranges + 1, s);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_ucount, 0, UPD_WORDS * sizeof(unsigned long long), s));

    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    TwoLevel lens = ctx->dec_lens;
    lens.total = (uint64_t *)res + 1;
    lens.total2 = ctx->d_out_offsets + nb;
    lens.min_out = (uint64_t *)res + 2;
    decode_prepare_kernel<<<dim3((unsigned)((nb + SCAN_GROUP - 1) / SCAN_GROUP)), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, d_block_offsets, nb, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);

    uint64_t *offs_new = d_out_block_offsets ? d_out_block_offsets : ctx->d_unew;
    UpdateArgs ua;
    memset(&ua, 0, sizeof(ua));
    DecRangeArgs &ra = ua.r;
    ra.range_lo = ctx->d_bstage;
    ra.range_hi = ctx->d_bstage + nranges;
    ra.out_offsets = ctx->d_bstage + 2 * nranges;
    ra.nranges = nranges;
    ra.nblocks = nb;
    ra.dmeta = ctx->d_dmeta;
    ra.status = ctx->d_status;
    ra.lens = lens;
    ra.first_bad = res + 2;
    ra.bprefix = ctx->d_bprefix;
    ra.obase = ctx->d_bobase;
    ra.cover = ctx->d_rcover;
    ra.rel = ctx->d_rrel;
    ra.kind = ctx->d_blk_item;
    ra.rplan = ctx->d_rplan;
    ra.rflag = ctx->d_rflag;
    ra.counters = ctx->d_rcounters;
    ua.src_offsets = ctx->d_bstage + 3 * nranges + 1;
    ua.old_offsets = d_block_offsets;
    ua.new_offsets = offs_new;
    ua.stream_len = stream_len;
    ua.row_of = ctx->d_urow_of;
    ua.row_blk = ctx->d_urow_blk;
    ua.pairs = ctx->d_upairs;
    ua.ucount = ctx->d_ucount;
    const unsigned plan_grid = grid256((nb + 1 > nranges ? nb + 1 : nranges));
    drange_plan_kernel<<<dim3(plan_grid), dim3(256), 0, s>>>(ra);
    const unsigned mark_y = nranges >= 64 ? 1u : (unsigned)(nb / 2048 < 1 ? 1 : (nb / 2048 > 16 ? 16 : nb / 2048));
    drange_mark_kernel<<<dim3((unsigned)nranges, mark_y), dim3(256), 0, s>>>(ra);
    upd_class_kernel<<<dim3(plan_grid), dim3(256), 0, s>>>(ua);
    HIP_OK(ctx, hipGetLastError());
    /* the one wait in front of the work: how many blocks are touched and staged and how long they are decides the rows,
     * the scratch area and the kernels; a range that cannot be served ends the call here */
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_rcounters, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 10, ctx->d_ucount, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    const uint64_t nstaged = ctx->h_result[8], longest_staged = ctx->h_result[9];
    const uint64_t ntouched = ctx->h_result[10], longest = ctx->h_result[11];
    if (ctx->h_result[12]) {
        const uint64_t key = ~ctx->h_result[12];
        const int err = (int)(key & 0xffu);
        set_err(ctx, err == HUFE_ARGUMENT ? "update_ranges: range %llu reaches past the end of the data"
                                          : "update_ranges: range %llu reaches a block whose header does not parse", (unsigned long long)(key >> 8));
        return err;
    }
    if (d_out_sub_index && longest > blocksize) {
        set_err(ctx, "update_ranges: a touched block of %llu bytes is longer than the sub-index rows of %llu", (unsigned long long)longest,
                (unsigned long long)blocksize);
        return HUFE_ARGUMENT;
    }
    const bool big = longest >= HUF_CHUNKED_FROM;      /* blocks of 2 MiB and more: one at a time through the chunked path */
    const uint64_t stride = (longest_staged + 15u) & ~15ull;
    const uint64_t enc_cap = big ? ((hufgpu_encode_bound(longest, longest) + 15u) & ~15ull) : 0;
    uint64_t staged_bytes = 0, scratch_bytes = 0;
    if (__builtin_mul_overflow(nstaged, stride, &staged_bytes) || __builtin_add_overflow(staged_bytes, enc_cap, &scratch_bytes)) scratch_bytes = ~0ull;
    if (scratch_bytes) {
        rc = grow_range_scratch(ctx, scratch_bytes);
        if (rc == HUFE_MEMORY) set_err(ctx, "update_ranges: no room for %llu staged blocks of up to %llu bytes", (unsigned long long)nstaged, (unsigned long long)longest_staged);
        if (rc) return rc;
    }
    rc = ensure_encode_ws(ctx, ntouched ? ntouched : 1);
    if (rc) return rc;
    ua.meta = ctx->d_meta;

    /* the rows' sources: one base, the lower of the new bytes and the scratch area, and 64-bit offsets */
    uint8_t *scr = ctx->d_rscratch;
    const uint8_t *base = (const uint8_t *)d_src;
    if (nstaged && (!base || (uintptr_t)scr < (uintptr_t)base)) base = scr;
    ua.src_off = d_src ? (uint64_t)((uintptr_t)d_src - (uintptr_t)base) : 0;
    ua.scratch_off = nstaged ? (uint64_t)((uintptr_t)scr - (uintptr_t)base) : 0;
    ua.src = (const uint8_t *)d_src;
    ua.scratch_w = scr;
    ra.stride = stride;
    ra.scratch = scr;
    upd_place_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ua);
    if (nstaged) {
        /* the staged blocks through the indexed decoders as they are, into their scratch entries: zeros + the placed offsets */
        TwoLevel blens = lens;
        blens.gprefix = ctx->d_bzero;
        blens.local = ctx->d_bobase;
        DecFixList fix;
        fix.count = ctx->d_fix_count;
        fix.blocks = ctx->d_fix_blocks;
        fix.flag = ctx->d_fix_flag;
        const unsigned fix_grid = (unsigned)(nb < 1024 ? nb : 1024);
        if (d_sub_index) {
            const HufSubIndex sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
            decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)(nb * cpb)), dim3(DSUB_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, ctx->d_out_offsets, blens, scr, staged_bytes, ctx->d_status, res, sub, blocksize, (uint32_t)cpb, fix);
        } else {
            DecodeFastArgs fa;
            fa.stream = st; fa.stream_len = stream_len; fa.offsets = d_block_offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
            fa.lens = blens; fa.out = scr; fa.out_cap = staged_bytes; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
            decode_fast_kernel<DEC_THREADS><<<dim3((unsigned)nb), dim3(DEC_THREADS), 0, s>>>(fa);
        }
        decode_fix_kernel<DEC_THREADS><<<dim3(fix_grid), dim3(DEC_THREADS), 0, s>>>(st, stream_len, d_block_offsets, ctx->d_dmeta, blens, scr, staged_bytes, ctx->d_status, res, fix);
        const unsigned overlay_y = nranges >= 1024 ? 2u : (nranges >= 64 ? 4u : 16u);
        upd_overlay_kernel<<<dim3((unsigned)nranges, overlay_y), dim3(256), 0, s>>>(ua);
        upd_fail_kernel<<<dim3(grid256(nb)), dim3(256), 0, s>>>(ua);
    }
    HIP_OK(ctx, hipGetLastError());

    UpdCopyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.stream = st;
    ca.out = (uint8_t *)d_out;
    ca.old_offsets = d_block_offsets;
    ca.new_offsets = offs_new;
    ca.kind = ctx->d_blk_item;
    ca.nblocks = nb;
    ca.out_cap = out_cap;
    ca.align = (uint64_t)((uintptr_t)d_out & 15u);
    /* pieces for all of the output: the new length is known on the device only, and a piece behind it returns at once */
    ca.npieces = (out_cap + ca.align) / UPD_PIECE + 1;
    rc = ensure_update_ws(ctx, nb, ca.npieces);
    if (rc) return rc;
    ca.piece_first = ctx->d_upiece;

    int err = HUFE_OK;
    if (!big) {
        if (ntouched) {
            TwoLevel sizes = ctx->enc_sizes;
            sizes.total = (uint64_t *)ctx->d_ucount + 5;         /* (the rows' sum: not used, the index is summed over all blocks below) */
            launch_pairs_trees(ctx, base, ntouched, longest, sizes, s);
        }
        upd_index_kernel<SCAN_THREADS><<<dim3(1), dim3(SCAN_THREADS), 0, s>>>(ua);
        if (ntouched) {
            const HufSubIndex sub = sub_index_view(d_out_sub_index, raw_size, blocksize);
            launch_pairs_pack(ctx, base, ntouched, longest, offs_new, nb, out_cap, (uint8_t *)d_out, sub, s);
        }
        upd_piece_kernel<<<dim3(grid256(ca.npieces)), dim3(256), 0, s>>>(ca);
        update_copy_kernel<<<dim3((unsigned)ca.npieces), dim3(256), 0, s>>>(ca);
        if (d_sub_index && d_out_sub_index) {
            const HufSubIndex from = sub_index_view((void *)d_sub_index, raw_size, blocksize), to = sub_index_view(d_out_sub_index, raw_size, blocksize);
            upd_sub_rows_kernel<<<dim3((unsigned)nb), dim3(256), 0, s>>>(from, to, ctx->d_blk_item, ctx->d_dmeta, ctx->d_bprefix, blocksize);
        }
        HIP_OK(ctx, hipGetLastError());
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_ucount, UPD_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
    } else {
        /* every block's place is worked out here, a touched block is encoded by encode_impl as a stream of one block into
         * the end of the scratch area and copied to its place; the untouched records then move as above */
        HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 8, ctx->d_ucount, UPD_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        uint8_t *enc = scr + staged_bytes;
        uint32_t *h_kind = (uint32_t *)malloc(nb * sizeof(uint32_t)), *h_row = (uint32_t *)malloc(nb * sizeof(uint32_t));
        uint64_t *h_pairs = (uint64_t *)malloc(2 * ntouched * sizeof(uint64_t)), *h_old = (uint64_t *)malloc(index_bytes), *h_new = (uint64_t *)malloc(index_bytes);
        hipError_t he = hipSuccess;
        if (!h_kind || !h_row || !h_pairs || !h_old || !h_new) err = HUFE_MEMORY;
        if (!err && !ctx->h_result[8 + UPD_FAILED]) {
            if (he == hipSuccess) he = hipMemcpyAsync(h_kind, ctx->d_blk_item, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_row, ctx->d_urow_of, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_pairs, ctx->d_upairs, 2 * ntouched * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_old, d_block_offsets, index_bytes, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);
            uint64_t pos = 0;
            for (uint64_t b = 0; b < nb && he == hipSuccess && !err; b++) {
                h_new[b] = pos;
                if (h_kind[b] == UPD_COPY) {
                    pos += h_old[b + 1] - h_old[b];
                } else if (h_kind[b] != UPD_VOID) {
                    const uint64_t *pr = h_pairs + 2 * (uint64_t)h_row[b];
                    uint64_t got = 0;
                    err = encode_impl(ctx, base + pr[0], pr[1], 0, enc, enc_cap, NULL, NULL, &got, s);
                    if (!err && (got > out_cap || pos > out_cap - got)) err = HUFE_MEMORY;
                    if (!err) he = hipMemcpyAsync((uint8_t *)d_out + pos, enc, got, hipMemcpyDeviceToDevice, s);
                    pos += got;
                }
                if (!err && pos > out_cap) err = HUFE_MEMORY;
            }
            h_new[nb] = pos;
            ctx->h_result[8 + UPD_TOTAL] = err ? ~0ull : pos;
            if (!err && he == hipSuccess) he = hipMemcpyAsync(offs_new, h_new, index_bytes, hipMemcpyHostToDevice, s);
            if (!err && he == hipSuccess) {
                upd_piece_kernel<<<dim3(grid256(ca.npieces)), dim3(256), 0, s>>>(ca);
                update_copy_kernel<<<dim3((unsigned)ca.npieces), dim3(256), 0, s>>>(ca);
                he = hipGetLastError();
            }
            if (he == hipSuccess) he = hipStreamSynchronize(s);
        }
        free(h_kind); free(h_row); free(h_pairs); free(h_old); free(h_new);
        HIP_OK(ctx, he);
        if (err == HUFE_MEMORY) set_err(ctx, "update_ranges: the new stream does not fit the output of %llu bytes", (unsigned long long)out_cap);
        if (err) return err;
    }
    if (ctx->h_result[8 + UPD_FAILED]) {
        /* a staged block that does not decode: what hufgpu_decode() says of it, the first in stream order */
        const uint64_t f = ~ctx->h_result[8 + UPD_FAILED];
        int32_t serr = HUFE_FATAL;
        HIP_OK(ctx, hipMemcpyAsync(&serr, ctx->d_status + f, sizeof(serr), hipMemcpyDeviceToHost, s));
        HIP_OK(ctx, hipStreamSynchronize(s));
        set_err(ctx, "update_ranges: block %llu, which a range cuts, does not decode (error %d)", (unsigned long long)f, (int)serr);
        return serr ? serr : HUFE_FATAL;
    }
    const uint64_t total = ctx->h_result[8 + UPD_TOTAL];
    if (total > out_cap) {
        set_err(ctx, "update_ranges: the new stream of %llu bytes does not fit the output of %llu", (unsigned long long)total, (unsigned long long)out_cap);
        return HUFE_MEMORY;
    }
    if (out_len) *out_len = total;
    if (blocks_reencoded) *blocks_reencoded = ntouched;
    return HUFE_OK;
}

/* ======================================================================================
 * An indexed stream made longer or shorter in place (include/huffman_gpu.h, kernels/append.hpp)
 * ==================================================================================== */

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
    const int max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    const uint64_t *view_offsets = d_block_offsets + view;
    const HufSubIndex old_sub = sub_index_view((void *)d_sub_index, raw_size, blocksize);
    const HufSubIndex view_sub = sub_view_from(old_sub, view);

    int rc = ensure_decode_ws(ctx, 1);
    if (rc) return rc;
    unsigned long long *res = (unsigned long long *)ctx->d_result;
    TwoLevel lens = ctx->dec_lens;
    lens.total = (uint64_t *)res + 1;
    lens.total2 = ctx->d_out_offsets + 1;
    lens.min_out = (uint64_t *)res + 2;

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
            decode_prepare_kernel<<<dim3(1), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, view_offsets, 1, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);
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
        decode_prepare_kernel<<<dim3(1), dim3(SCAN_GROUP), 0, s>>>(st, stream_len, view_offsets, 1, max_tree, ctx->d_dmeta, ctx->d_status, lens, ctx->d_fix_count);
    app_plan_kernel<<<dim3(grid256(rows)), dim3(256), 0, s>>>(aa);
    if (head) {
        /* the block that is opened again through the indexed decoders as they are, to the front of the scratch area */
        DecFixList fix;
        fix.count = ctx->d_fix_count;
        fix.blocks = ctx->d_fix_blocks;
        fix.flag = ctx->d_fix_flag;
        if (view_sub.tile_bits) {
            const uint64_t cpb = (blocksize + DSUB_CHUNK_SYMS - 1) / DSUB_CHUNK_SYMS;
            decode_sub_kernel<DSUB_THREADS><<<dim3((unsigned)cpb), dim3(DSUB_THREADS), 0, s>>>(st, stream_len, view_offsets, ctx->d_dmeta, ctx->d_out_offsets, lens, scr, view_len, ctx->d_status, res, view_sub, blocksize, (uint32_t)cpb, fix);
        } else {
            DecodeFastArgs fa;
            fa.stream = st; fa.stream_len = stream_len; fa.offsets = view_offsets; fa.dmeta = ctx->d_dmeta; fa.out_offsets = ctx->d_out_offsets;
            fa.lens = lens; fa.out = scr; fa.out_cap = view_len; fa.status = ctx->d_status; fa.result = res; fa.fix = fix;
            decode_fast_kernel<DEC_THREADS><<<dim3(1), dim3(DEC_THREADS), 0, s>>>(fa);
        }
        decode_fix_kernel<DEC_THREADS><<<dim3(1), dim3(DEC_THREADS), 0, s>>>(st, stream_len, view_offsets, ctx->d_dmeta, lens, scr, view_len, ctx->d_status, res, fix);
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

/* ======================================================================================
 * The sub-index of a stream that came without one (include/huffman_gpu.h, kernels/sub_build.hpp)
 * ==================================================================================== */

/* hufgpu_build_sub_index decodes this many bytes of whole blocks at a time into the context's scratch area (one block
 * when a block is longer): half of the 256 MiB Infinity Cache, so the builder reads what the decoder has just written
 * from there, and 2 048 blocks of 64 KiB - eight for each of the 256 CUs - a slab */
#define SUB_SLAB_BYTES (128ull << 20)

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

/* what the three entry points check alike, before the context is looked at; blocksize 0 becomes raw_size */
static int sub_build_check(hufgpu_ctx *ctx, const char *who, const void *d_stream, const uint64_t *d_block_offsets, uint64_t raw_size,
                           uint64_t *blocksize, const void *d_sub_index)
{
    if (!d_stream || !d_block_offsets) {
        set_err(NULL, "%s: the stream or its block index is missing", who);
        return HUFE_ARGUMENT;
    }
    if (!d_sub_index || ((uintptr_t)d_sub_index & 7u)) {
        set_err(NULL, "%s: the sub-index buffer must be there and 8-byte aligned", who);
        return HUFE_ARGUMENT;
    }
    if (*blocksize == 0) *blocksize = raw_size;
    const uint64_t cpb = *blocksize >= HUF_CHUNKED_FROM ? (*blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS : 1;
    if (*blocksize > HUFGPU_MAX_BLOCK || hufgpu_block_count(raw_size, *blocksize) * cpb > 0x7fffffffull) {
        set_err(NULL, "%s: blocks of more than %llu bytes, or more than 2^31 - 1 blocks or chunks", who, (unsigned long long)HUFGPU_MAX_BLOCK);
        return HUFE_ARGUMENT;
    }
    if (!ctx) {
        set_err(NULL, "%s: needs a context (there is no CPU path)", who);
        return HUFE_ARGUMENT;
    }
    return HUFE_OK;
}

/* one launch sequence: the rows of blocks blk0 .. blk0 + nblk - 1, whose decoded bytes start at `raw` */
static int sub_build_enqueue(hufgpu_ctx *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                             const void *raw, uint64_t raw_avail, uint64_t raw_size, uint64_t blocksize, uint64_t blk0, uint64_t nblk,
                             void *d_sub_index, uint32_t flags, const int32_t *dec_status, hipStream_t s)
{
    const uint64_t cpb = blocksize >= HUF_CHUNKED_FROM ? (blocksize + HUF_CHUNK_SYMS - 1) / HUF_CHUNK_SYMS : 1;
    int rc = ensure_sub_build_ws(ctx, nblk, cpb > 1 ? nblk * cpb : 0);
    if (rc) return rc;
    SubBuildArgs a;
    memset(&a, 0, sizeof(a));
    a.stream = (const uint8_t *)d_stream;
    a.stream_len = stream_len;
    a.offsets = d_block_offsets;
    a.raw = (const uint8_t *)raw;
    a.raw_avail = raw_avail;
    a.n = raw_size;
    a.blocksize = blocksize;
    a.blk0 = blk0;
    a.nblk = (uint32_t)nblk;
    a.cpb = (uint32_t)cpb;
    a.max_tree = (flags & HUFGPU_RELAXED_TREE) ? HUF_TREE_MAX : HUF_TREE_STRICT;
    a.dec_status = dec_status;
    a.sub = sub_index_view(d_sub_index, raw_size, blocksize);
    a.state = ctx->d_sb_state;
    a.pay_bytes = ctx->d_sb_pay;
    a.chunk_tot = ctx->d_sb_chunk_tot;
    a.chunk_bits = ctx->d_sb_chunk_bits;
    a.unbuilt = ctx->d_sb_unbuilt;
    static const bool wide_table = getenv("HUF_GPU_SUB_TABLE") && atoi(getenv("HUF_GPU_SUB_TABLE")) == 1;   /* (measurements: the 8-byte table reads) */
    sub_lens_kernel<<<dim3((unsigned)nblk), dim3(SB_THREADS), 0, s>>>(a);
    if (wide_table) sub_groups_kernel<1><<<dim3((unsigned)(nblk * cpb)), dim3(SB_THREADS), 0, s>>>(a);
    else sub_groups_kernel<0><<<dim3((unsigned)(nblk * cpb)), dim3(SB_THREADS), 0, s>>>(a);
    if (cpb > 1) {
        sub_chunk_scan_kernel<SCAN_THREADS><<<dim3((unsigned)nblk), dim3(SCAN_THREADS), 0, s>>>(a);
        sub_tile_add_kernel<<<dim3((unsigned)(nblk * cpb)), dim3(HUF_CHUNK_SYMS / HUF_SUB_TILE), 0, s>>>(a);
    }
    HIP_OK(ctx, hipGetLastError());
    return HUFE_OK;
}

static int sub_build_count(hufgpu_ctx *ctx, uint64_t *unbuilt, hipStream_t s)
{
    HIP_OK(ctx, hipMemcpyAsync(ctx->h_result + 10, ctx->d_sb_unbuilt, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_OK(ctx, hipStreamSynchronize(s));
    *unbuilt = ctx->h_result[10];
    return HUFE_OK;
}

extern "C" int hufgpu_sub_index_from_raw(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                         const void *d_raw, uint64_t raw_size, uint64_t blocksize, void *d_sub_index, uint32_t flags,
                                         uint64_t *unbuilt, void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) return HUFE_OK;
    if (!d_raw) {
        set_err(NULL, "sub_index_from_raw: the decoded data is missing");
        return HUFE_ARGUMENT;
    }
    int rc = sub_build_check(ctx, "sub_index_from_raw", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    rc = ensure_sub_build_ws(ctx, 0, 0);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, d_raw, raw_size, raw_size, blocksize, 0, nb, d_sub_index, flags, NULL, s);
    if (rc) return rc;
    return unbuilt ? sub_build_count(ctx, unbuilt, s) : HUFE_OK;
}

extern "C" int hufgpu_decode_build_sub(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                       uint64_t raw_size, uint64_t blocksize, void *d_out, uint64_t out_cap, void *d_sub_index,
                                       uint32_t flags, uint64_t *raw_len, uint64_t *unbuilt, void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) {
        if (ctx) ctx->decode_pending = 0;
        if (raw_len) *raw_len = 0;
        return HUFE_OK;
    }
    if (!d_out && out_cap) {
        set_err(NULL, "decode_build_sub: the output buffer is missing");
        return HUFE_ARGUMENT;
    }
    int rc = sub_build_check(ctx, "decode_build_sub", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    rc = decode_impl(ctx, d_stream, stream_len, d_block_offsets, nb, NULL, 0, d_out, out_cap, flags, NULL, stream);
    if (rc) return rc;
    if (!ctx->decode_pending) {                    /* an empty stream: nothing was decoded, no row can be built */
        if (raw_len) *raw_len = 0;
        if (unbuilt) *unbuilt = nb;
        return HUFE_OK;
    }
    hipStream_t s = pick_stream(ctx, stream);
    rc = ensure_sub_build_ws(ctx, 0, 0);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    /* the rows come from the output just written: a block that did not decode (d_status) is unbuilt */
    rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, d_out, out_cap < raw_size ? out_cap : raw_size, raw_size, blocksize, 0, nb,
                           d_sub_index, flags, ctx->d_status, s);
    if (rc) return rc;
    if (unbuilt) {                                 /* (read first: hufgpu_decode_result may go on to decode a failing block again) */
        rc = sub_build_count(ctx, unbuilt, s);
        if (rc) return rc;
    }
    return raw_len ? hufgpu_decode_result(ctx, raw_len) : HUFE_OK;
}

extern "C" int hufgpu_build_sub_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                                      uint64_t raw_size, uint64_t blocksize, void *d_sub_index, uint32_t flags, uint64_t *unbuilt,
                                      void *stream)
{
    if (unbuilt) *unbuilt = 0;
    if (raw_size == 0) return HUFE_OK;
    int rc = sub_build_check(ctx, "build_sub_index", d_stream, d_block_offsets, raw_size, &blocksize, d_sub_index);
    if (rc) return rc;
    const uint64_t nb = hufgpu_block_count(raw_size, blocksize);
    if (stream_len == 0) {                         /* an empty stream: no row can be built */
        if (unbuilt) *unbuilt = nb;
        return HUFE_OK;
    }
    HIP_OK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = pick_stream(ctx, stream);
    const uint64_t slab_blocks = blocksize >= SUB_SLAB_BYTES ? 1 : (nb < SUB_SLAB_BYTES / blocksize ? nb : SUB_SLAB_BYTES / blocksize);
    const uint64_t need = slab_blocks * blocksize < raw_size ? slab_blocks * blocksize : raw_size;
    rc = grow_range_scratch(ctx, need);           /* the staging area of hufgpu_decode_ranges */
    if (rc == HUFE_MEMORY)
        set_err(ctx, "build_sub_index: no room for %llu decoded blocks of %llu bytes", (unsigned long long)slab_blocks,
                (unsigned long long)blocksize);
    if (rc) return rc;
    rc = ensure_sub_build_ws(ctx, 0, 0);
    if (rc) return rc;
    HIP_OK(ctx, hipMemsetAsync(ctx->d_sb_unbuilt, 0, sizeof(unsigned long long), s));
    for (uint64_t b0 = 0; b0 < nb; b0 += slab_blocks) {
        const uint64_t k = nb - b0 < slab_blocks ? nb - b0 : slab_blocks;
        const uint64_t bytes = b0 + k == nb ? raw_size - b0 * blocksize : k * blocksize;
        rc = decode_impl(ctx, d_stream, stream_len, d_block_offsets + b0, k, NULL, 0, ctx->d_rscratch, bytes, flags, NULL, stream);
        if (rc == HUFE_OK)
            rc = sub_build_enqueue(ctx, d_stream, stream_len, d_block_offsets, ctx->d_rscratch, bytes, raw_size, blocksize, b0, k, d_sub_index,
                                   flags, ctx->d_status, s);
        if (rc) break;
    }
    /* the slabs' decodes were this call's own: nothing of them is left for hufgpu_decode_result() */
    ctx->decode_pending = 0;
    ctx->last_st = NULL;
    uint64_t cnt = 0;
    const int rc2 = sub_build_count(ctx, &cnt, s);
    if (rc) return rc;
    if (rc2) return rc2;
    if (unbuilt) *unbuilt = cnt;
    return HUFE_OK;
}

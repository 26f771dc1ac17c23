/* ctx.hpp - the per-device context of the device C ABI (include/huffman_gpu.h): the struct, the error text, the one
   table of its workspaces behind the struct (host/workspace.hpp grows and frees what the table describes; DESIGN.md,
   "The context's workspaces"), create and destroy.  Part of hufgpu_api.hip (one translation unit). */
#pragma once

#include "workspace.hpp"

struct hufgpu_ctx {
    int device;
    hipStream_t stream;           /* NULL, the device's default stream: ordered with every blocking stream (torch's default included) */
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
    uint64_t *d_walk;             /* 5 result words of walk_kernel (fixed) */
    uint64_t *d_spec_off;         /* speculative output offsets of the candidates (disc_cands + 1) */
    uint64_t scounters[8];        /* hufgpu_stream_counters(): of the last hufgpu_decode_stream / hufgpu_block_index */

    /* blocks of many MiB in a raw stream: the sub-index built for them (kernels/spec_index.hpp) */
    uint64_t big_lanes, big_sub_bytes;
    uint64_t *d_big_entry, *d_big_exit, *d_big_pre, *d_big_wgpre, *d_big_wgscratch, *d_big_first_pos, *d_big_first_g, *d_big_last_pos;
    uint32_t *d_big_cnt;
    void *d_big_sub;
    uint64_t *d_big_offs;         /* SPEC_WORDS status words, then the two-entry block index (fixed) */

    uint64_t fixed_ws;            /* 1 once the fixed group stands: the buffers marked (fixed), allocated by create */
    uint64_t *d_result;           /* 8 words: err, raw_len, failing block / consumed, blocks, complete consumed, complete raw */
    uint64_t complete_used, complete_raw;   /* of the last hufgpu_decode_stream(): see hufgpu_decode_stream_complete() */
    uint64_t *h_result;           /* pinned mirror (d_result, h_result, d_zipf: fixed) */
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
    unsigned long long *d_rcounters;          /* (fixed) */
    unsigned long long *d_rtpairs;            /* the tile route's (range, tile) pairs per block (kernels/range_tiles.hpp) */
    uint64_t rcounters[8];                    /* hufgpu_ranges_counters(): of the last hufgpu_decode_ranges */
    uint8_t *d_rscratch;
    uint64_t rscratch_bytes;

    /* hufgpu_gather (kernels/gather.hpp): part counts and cursors per block, the list of touched blocks, the scan of the
     * counts and its grand total, the parts */
    uint64_t gws_blocks, gws_parts;
    uint32_t *d_gcnt, *d_glist;
    TwoLevel gat_scan;
    uint64_t *d_gtotal;                       /* (fixed) */
    void *d_gparts;
    int cus;                                  /* compute units of the device */

    /* hufgpu_find_bytes and hufgpu_find_pattern (kernels/find.hpp): a match mask per group of 32 symbols, a count per
     * tile, the scan of the counts; the pattern call's edge bytes per tile, which a find_bytes call never allocates */
    uint64_t fws_words, fws_tiles, fws_edge_tiles;
    uint32_t *d_fbitmap, *d_ftcnt;
    TwoLevel find_scan;
    uint8_t *d_fedges;
    /* hufgpu_find_records: a delimiter mask and a mask of record starts next to the match mask, the delimiters of a
     * tile and the record starts of a tile, the delimiters' scan and its grand total; the two other calls never allocate them */
    uint64_t frws_words, frws_tiles;
    uint32_t *d_frdbits, *d_frrbits, *d_frdcnt, *d_frrcnt;
    TwoLevel frec_scan;
    uint64_t *d_frdtotal;
    /* hufgpu_find_records_select with d_rec_no: the first block that is not served; no other call allocates it */
    uint64_t fsel_ws;
    uint64_t *d_fsel_first;
    /* hufgpu_find_records_context with a distance that is not 0: the mask and the tile counts of the records to report next
     * to those of the selected ones, the scan of the selected records' counts and the four words its kernel takes for
     * totals; no other call allocates them */
    uint64_t fcws_words, fcws_tiles;
    uint32_t *d_fcbits, *d_fccnt;
    TwoLevel fctx_scan;
    uint64_t *d_fctotals;
    /* hufgpu_find_records_anchored with HUFGPU_ANCHOR_WORD: a third mask, the bytes that may stand in front of a match, and
     * the tile counts that find_sub_kernel writes next to it (nobody reads them); no other call allocates them */
    uint64_t faws_words, faws_tiles;
    uint32_t *d_fabits, *d_fatcnt;
    /* hufgpu_find_records_terms with two terms or more: a match mask and a record mask a term with their tile counts,
     * term-major (the capacities count terms x words and terms x tiles), sixteen words for the totals of the terms' scans,
     * and - an ordered call only - a scan of the match counts a term; no other call allocates them */
    uint64_t ftws_words, ftws_tiles, ftsws_tiles[FIND_TERMS_MAX];
    uint32_t *d_ftmbits, *d_ftrbits, *d_ftmcnt, *d_ftrcnt;
    uint64_t *d_fttotals;
    TwoLevel fterm_scan[FIND_TERMS_MAX];

    /* the sub-index builders (kernels/sub_build.hpp): what their kernels hand to one another, per block and per chunk */
    uint64_t sbws_blocks, sbws_chunks;
    uint32_t *d_sb_state;
    uint64_t *d_sb_pay, *d_sb_chunk_tot, *d_sb_chunk_bits;
    unsigned long long *d_sb_unbuilt;         /* (fixed) */

    /* hufgpu_update_ranges (kernels/update.hpp): the touched blocks' rows, the new index when the caller wants none,
     * the copy pieces' first blocks */
    uint64_t uws_blocks, uws_pieces;
    uint32_t *d_urow_of, *d_urow_blk, *d_upiece;
    uint64_t *d_upairs, *d_unew;
    unsigned long long *d_ucount;             /* (fixed) */

    /* hufgpu_scatter (kernels/scatter.hpp): what its kernels hand to its last one; everything else it uses is the
     * workspaces of hufgpu_gather and hufgpu_update_ranges */
    unsigned long long *d_scount;             /* (fixed) */

    /* hufgpu_select_spans (kernels/select.hpp): the maps of the tiles and of every composition level, a mark a rank, the scan
     * of the tiles' counts, and two words: the lowest offending rank, the selected count; no other call allocates them */
    uint64_t sws_tiles;
    uint8_t *d_smaps;
    uint64_t *d_smarks;
    unsigned long long *d_swords;
    TwoLevel sel_scan;
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

/* ---- the workspaces: every buffer above but the profiling events is a row here (host/workspace.hpp) ---- */

static hipError_t g_ws_error = hipSuccess;   /* of the hook that failed last: grow_ws() words its report with it */
static int ws_hip(hipError_t e)
{
    if (e == hipSuccess) return 0;
    g_ws_error = e;
    (void)hipGetLastError();
    return 1;
}
static int ws_hip_alloc_device(void **p, uint64_t bytes) { return ws_hip(hipMalloc(p, bytes)); }
static int ws_hip_alloc_pinned(void **p, uint64_t bytes) { return ws_hip(hipHostMalloc(p, bytes, hipHostMallocDefault)); }
static void ws_hip_free_device(void *p) { (void)hipFree(p); }
static void ws_hip_free_pinned(void *p) { (void)hipHostFree(p); }
static int ws_hip_zero_device(void *p, uint64_t bytes) { return ws_hip(hipMemset(p, 0, bytes)); }
/* The one wait rule: the whole device.  A call may have left work on any stream of the caller's, a non-blocking one
 * included, that still uses the buffers about to go, and the zeros of a new buffer must be there before a kernel on such
 * a stream counts on them.  Only a growth pays for it. */
static int ws_hip_wait(void) { return ws_hip(hipDeviceSynchronize()); }
static const ws_hooks WS_HIP = {ws_hip_alloc_device, ws_hip_alloc_pinned, ws_hip_free_device, ws_hip_free_pinned,
                                ws_hip_zero_device, ws_hip_wait};

/* a buffer of `expr` bytes, n and m being the capacities of its group */
#define WS_ROW(type, member, flags, expr) \
    {offsetof(type, member), [](uint64_t n, uint64_t m) -> uint64_t { (void)n; (void)m; return (expr); }, flags}
#define DEV(member, expr) WS_ROW(hufgpu_ctx, member, 0, expr)
#define DEV0(member, expr) WS_ROW(hufgpu_ctx, member, WS_ZERO, expr)
#define PIN(member, expr) WS_ROW(hufgpu_ctx, member, WS_PINNED, expr)
#define SCAN_GROUPS(n) ((n) / SCAN_GROUP + 2)

/* a two-level prefix sum over n values (kernels/offsets.hpp); the counters start, and are left, at zero.  gmin is a row
 * of the one group that combines a minimum */
static const ws_buf WS_SCAN[] = {
    WS_ROW(TwoLevel, vals, 0, n * sizeof(uint64_t)),
    WS_ROW(TwoLevel, local, 0, n * sizeof(uint64_t)),
    WS_ROW(TwoLevel, gsum, 0, SCAN_GROUPS(n) * sizeof(uint64_t)),
    WS_ROW(TwoLevel, gprefix, 0, SCAN_GROUPS(n) * sizeof(uint64_t)),
    WS_ROW(TwoLevel, gcount, WS_ZERO, SCAN_GROUPS(n) * SCAN_TICKET_STRIDE * sizeof(uint32_t)),
    WS_ROW(TwoLevel, done, WS_ZERO, sizeof(uint32_t)),
};
/* what create allocates once: the result words and their pinned mirror, the zipf weights, the status words of the
 * features (SPEC_WORDS status words, then the two-entry block index, for the blocks of many MiB) */
static const ws_buf WS_FIXED[] = {
    DEV(d_result, 8 * sizeof(uint64_t)), PIN(h_result, 16 * sizeof(uint64_t)), DEV(d_walk, DISC_WORDS * sizeof(uint64_t)),
    DEV(d_zipf, 255 * sizeof(uint64_t)), DEV(d_big_offs, (SPEC_WORDS + 2) * sizeof(uint64_t)),
    DEV(d_rcounters, 8 * sizeof(unsigned long long)), DEV(d_gtotal, sizeof(uint64_t)),
    DEV(d_ucount, UPD_WORDS * sizeof(unsigned long long)), DEV(d_sb_unbuilt, sizeof(unsigned long long)),
    DEV(d_scount, SCAT_WORDS * sizeof(unsigned long long)),
};
static const ws_buf WS_ENCODE[] = {
    DEV(d_hist, n * HUF_NSYM * sizeof(uint64_t)),   /* (64-bit counts for chunked blocks) */
    DEV(d_codetab, n * HUF_NSYM * sizeof(hufcode_t)), DEV(d_treebuf, n * HUF_TREE_STRIDE * sizeof(int16_t)),
    DEV(d_meta, n * sizeof(HufBlockMeta)), DEV(d_offsets, (n + 1) * sizeof(uint64_t)),
};
static const ws_buf WS_CHUNK[] = {
    DEV(d_chunk_hist, n * HUF_NSYM * sizeof(uint32_t)), DEV(d_chunk_tot, n * sizeof(uint64_t)), DEV(d_chunk_bits, n * sizeof(uint64_t)),
};
static const ws_buf WS_DECODE[] = {
    DEV(d_dmeta, n * sizeof(HufDecodeMeta)), DEV(d_out_offsets, (n + 1) * sizeof(uint64_t)), DEV(d_status, n * sizeof(int32_t)),
    DEV0(d_fix_count, 2 * sizeof(uint32_t)), DEV(d_fix_blocks, n * sizeof(uint32_t)), DEV0(d_fix_flag, n * sizeof(uint32_t)),
    DEV(dec_lens.gmin, SCAN_GROUPS(n) * sizeof(uint64_t)),
};
#define DISC_GCAP(n) (((n) + DISC_SCAN_GROUP - 1) / DISC_SCAN_GROUP + 1)
static const ws_buf WS_DISC_WGS[] = {
    DEV(d_wg_counts, n * sizeof(uint32_t)),
    DEV(d_wg_base, (n + 1 + 2 * DISC_GCAP(n)) * sizeof(uint64_t)),     /* local sums, then the groups' bases and totals */
    DEV(d_disc_masks, n * DISC_THREADS * sizeof(uint64_t)), DEV(d_disc_slots, n * DISC_SLOTS * sizeof(DiscSlot)),
};
static const ws_buf WS_DISC_CANDS[] = {
    DEV(d_cand, n * sizeof(uint64_t)), DEV(d_cand_end, n * sizeof(uint64_t)), DEV(d_chain, (n + 1) * sizeof(uint64_t)),
    DEV(d_cand_status, n * sizeof(int32_t)), DEV(d_nxt, n * sizeof(uint32_t)), DEV(d_spec_off, (n + 1) * sizeof(uint64_t)),
};
static const ws_buf WS_BIG_LANES[] = {
    DEV(d_big_entry, n * sizeof(uint64_t)), DEV(d_big_exit, n * sizeof(uint64_t)), DEV(d_big_pre, (n + 1) * sizeof(uint64_t)),
    DEV(d_big_wgpre, (n / DEC_THREADS + 4) * sizeof(uint64_t)), DEV(d_big_wgscratch, (n / DEC_THREADS + 4) * sizeof(uint64_t)),
    DEV(d_big_first_pos, n * sizeof(uint64_t)), DEV(d_big_first_g, n * sizeof(uint64_t)), DEV(d_big_last_pos, n * sizeof(uint64_t)),
    DEV(d_big_cnt, n * sizeof(uint32_t)),
};
static const ws_buf WS_BIG_SUB[] = {DEV(d_big_sub, n)};
static const ws_buf WS_BSTAGE[] = {PIN(h_bstage, n * sizeof(uint64_t)), DEV(d_bstage, n * sizeof(uint64_t))};
static const ws_buf WS_BATCH[] = {     /* n blocks, m items */
    DEV(d_bprefix, (n + 1) * sizeof(uint64_t)), DEV(d_bobase, n * sizeof(uint64_t)), DEV0(d_bzero, SCAN_GROUPS(n) * sizeof(uint64_t)),
    DEV(d_blk_item, n * sizeof(uint32_t)), DEV(d_item_fail, m * sizeof(unsigned long long)), DEV(d_item_res, 3 * m * sizeof(uint64_t)),
    DEV(d_bitem_offs, (m + 1) * sizeof(uint64_t)), PIN(h_item_res, 3 * m * sizeof(uint64_t)),
};
static const ws_buf WS_RANGE[] = {     /* n blocks, m ranges */
    DEV(d_rcover, n * sizeof(unsigned long long)), DEV(d_rrel, n * sizeof(uint64_t)), DEV(d_rtpairs, n * sizeof(unsigned long long)),
    DEV(d_rplan, 4 * m * sizeof(uint64_t)), DEV(d_rflag, m * sizeof(uint32_t)),
};
static const ws_buf WS_RSCRATCH[] = {DEV(d_rscratch, n)};
static const ws_buf WS_GATHER_BLOCKS[] = {DEV(d_gcnt, 2 * n * sizeof(uint32_t)), DEV(d_glist, n * sizeof(uint32_t))};
static const ws_buf WS_GATHER_PARTS[] = {DEV(d_gparts, n * sizeof(GatherPart))};
static const ws_buf WS_FIND_WORDS[] = {DEV(d_fbitmap, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_TILES[] = {DEV(d_ftcnt, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_EDGES[] = {DEV(d_fedges, n * FIND_EDGE_SLOT)};
static const ws_buf WS_FIND_REC_WORDS[] = {DEV(d_frdbits, n * sizeof(uint32_t)), DEV(d_frrbits, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_REC_TILES[] = {DEV(d_frdcnt, n * sizeof(uint32_t)), DEV(d_frrcnt, n * sizeof(uint32_t)), DEV(d_frdtotal, sizeof(uint64_t))};
static const ws_buf WS_FIND_SEL[] = {DEV(d_fsel_first, n * sizeof(uint64_t))};
static const ws_buf WS_FIND_CTX_WORDS[] = {DEV(d_fcbits, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_CTX_TILES[] = {DEV(d_fccnt, n * sizeof(uint32_t)), DEV(d_fctotals, 4 * sizeof(uint64_t))};
static const ws_buf WS_FIND_ANC_WORDS[] = {DEV(d_fabits, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_ANC_TILES[] = {DEV(d_fatcnt, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_TERM_WORDS[] = {DEV(d_ftmbits, n * sizeof(uint32_t)), DEV(d_ftrbits, n * sizeof(uint32_t))};
static const ws_buf WS_FIND_TERM_TILES[] = {DEV(d_ftmcnt, n * sizeof(uint32_t)), DEV(d_ftrcnt, n * sizeof(uint32_t)),
                                            DEV(d_fttotals, 4 * FIND_TERMS_MAX * sizeof(uint64_t))};
static const ws_buf WS_SB_BLOCKS[] = {DEV(d_sb_state, n * sizeof(uint32_t)), DEV(d_sb_pay, n * sizeof(uint64_t))};
static const ws_buf WS_SB_CHUNKS[] = {DEV(d_sb_chunk_tot, n * sizeof(uint64_t)), DEV(d_sb_chunk_bits, n * sizeof(uint64_t))};
static const ws_buf WS_UPD_BLOCKS[] = {
    DEV(d_urow_of, n * sizeof(uint32_t)), DEV(d_urow_blk, n * sizeof(uint32_t)), DEV(d_upairs, 2 * n * sizeof(uint64_t)),
    DEV(d_unew, (n + 1) * sizeof(uint64_t)),
};
static const ws_buf WS_UPD_PIECES[] = {DEV(d_upiece, n * sizeof(uint32_t))};
static const ws_buf WS_SELECT[] = {     /* n tiles: their maps and those of the levels above, a sixty-fourth each of the one below */
    DEV(d_smaps, (n + n / 32 + 16) * SEL_WINDOW), DEV(d_smarks, n * SEL_MARK_WORDS * sizeof(uint64_t)),
    DEV(d_swords, 2 * sizeof(unsigned long long)),
};

/* The groups.  Most grow by an eighth; the staging area by a quarter; gather, find and select double, since their bounds come
 * from the host's arguments (records x parts, the layout of all blocks) and jump from call to call; the sub-index of a
 * block of many MiB and the range scratch take what they are asked for (grow_range_scratch adds its own eighth).
 * Soft groups report nothing: the caller has another way, or words the error itself. */
enum { G_FIXED, G_ENCODE, G_CHUNK, G_DECODE, G_DISC_WGS, G_DISC_CANDS, G_BIG_LANES, G_BIG_SUB, G_BSTAGE, G_BATCH, G_RANGE,
       G_RSCRATCH, G_GATHER_BLOCKS, G_GATHER_PARTS, G_FIND_WORDS, G_FIND_TILES, G_FIND_EDGES, G_FIND_REC_WORDS, G_FIND_REC_TILES, G_FIND_SEL, G_FIND_CTX_WORDS, G_FIND_CTX_TILES, G_FIND_ANC_WORDS, G_FIND_ANC_TILES,
       G_FIND_TERM_WORDS, G_FIND_TERM_TILES, G_FIND_TERM_SCAN0, G_FIND_TERM_SCAN1, G_FIND_TERM_SCAN2, G_FIND_TERM_SCAN3, G_SB_BLOCKS, G_SB_CHUNKS, G_UPD_BLOCKS,
       G_UPD_PIECES, G_SELECT, G_COUNT };
#define ROWS(a) a, (int)(sizeof(a) / sizeof(a[0]))
#define CAP(member) {offsetof(hufgpu_ctx, member), WS_NO_CAP}
#define CAPS(m0, m1) {offsetof(hufgpu_ctx, m0), offsetof(hufgpu_ctx, m1)}
#define NO_SCAN NULL, 0, 0
#define SCAN_AT(member) ROWS(WS_SCAN), offsetof(hufgpu_ctx, member)
static const ws_group WS[G_COUNT] = {
    {"fixed", ROWS(WS_FIXED), CAP(fixed_ws), WS_EXACT, false, NO_SCAN},
    {"encode", ROWS(WS_ENCODE), CAP(ws_blocks), WS_EIGHTH, false, SCAN_AT(enc_sizes)},
    {"encode chunks", ROWS(WS_CHUNK), CAP(ws_chunks), WS_EIGHTH, false, NO_SCAN},
    {"decode", ROWS(WS_DECODE), CAP(dws_blocks), WS_EIGHTH, false, SCAN_AT(dec_lens)},
    {"discovery workgroups", ROWS(WS_DISC_WGS), CAP(disc_wgs), WS_EIGHTH, false, NO_SCAN},
    {"discovery candidates", ROWS(WS_DISC_CANDS), CAP(disc_cands), WS_EIGHTH, false, NO_SCAN},
    {"big-block lanes", ROWS(WS_BIG_LANES), CAP(big_lanes), WS_EIGHTH, true, NO_SCAN},
    {"big-block sub-index", ROWS(WS_BIG_SUB), CAP(big_sub_bytes), WS_EXACT, true, NO_SCAN},
    {"batch staging", ROWS(WS_BSTAGE), CAP(bstage_words), WS_QUARTER, false, NO_SCAN},
    {"batch", ROWS(WS_BATCH), CAPS(bws_blocks, bws_items), WS_EIGHTH, false, NO_SCAN},
    {"ranges", ROWS(WS_RANGE), CAPS(rws_blocks, rws_ranges), WS_EIGHTH, false, NO_SCAN},
    {"range scratch", ROWS(WS_RSCRATCH), CAP(rscratch_bytes), WS_EXACT, true, NO_SCAN},
    {"gather blocks", ROWS(WS_GATHER_BLOCKS), CAP(gws_blocks), WS_DOUBLE, false, SCAN_AT(gat_scan)},
    {"gather parts", ROWS(WS_GATHER_PARTS), CAP(gws_parts), WS_DOUBLE, false, NO_SCAN},
    {"find words", ROWS(WS_FIND_WORDS), CAP(fws_words), WS_DOUBLE, false, NO_SCAN},
    {"find tiles", ROWS(WS_FIND_TILES), CAP(fws_tiles), WS_DOUBLE, false, SCAN_AT(find_scan)},
    {"find edges", ROWS(WS_FIND_EDGES), CAP(fws_edge_tiles), WS_DOUBLE, false, NO_SCAN},
    {"find record words", ROWS(WS_FIND_REC_WORDS), CAP(frws_words), WS_DOUBLE, false, NO_SCAN},
    {"find record tiles", ROWS(WS_FIND_REC_TILES), CAP(frws_tiles), WS_DOUBLE, false, SCAN_AT(frec_scan)},
    {"find select", ROWS(WS_FIND_SEL), CAP(fsel_ws), WS_EXACT, false, NO_SCAN},
    {"find context words", ROWS(WS_FIND_CTX_WORDS), CAP(fcws_words), WS_DOUBLE, false, NO_SCAN},
    {"find context tiles", ROWS(WS_FIND_CTX_TILES), CAP(fcws_tiles), WS_DOUBLE, false, SCAN_AT(fctx_scan)},
    {"find anchor words", ROWS(WS_FIND_ANC_WORDS), CAP(faws_words), WS_DOUBLE, false, NO_SCAN},
    {"find anchor tiles", ROWS(WS_FIND_ANC_TILES), CAP(faws_tiles), WS_DOUBLE, false, NO_SCAN},
    {"find term words", ROWS(WS_FIND_TERM_WORDS), CAP(ftws_words), WS_DOUBLE, false, NO_SCAN},
    {"find term tiles", ROWS(WS_FIND_TERM_TILES), CAP(ftws_tiles), WS_DOUBLE, false, NO_SCAN},
    {"find term scan 0", NULL, 0, CAP(ftsws_tiles[0]), WS_DOUBLE, false, SCAN_AT(fterm_scan[0])},      /* (a scan and nothing else) */
    {"find term scan 1", NULL, 0, CAP(ftsws_tiles[1]), WS_DOUBLE, false, SCAN_AT(fterm_scan[1])},
    {"find term scan 2", NULL, 0, CAP(ftsws_tiles[2]), WS_DOUBLE, false, SCAN_AT(fterm_scan[2])},
    {"find term scan 3", NULL, 0, CAP(ftsws_tiles[3]), WS_DOUBLE, false, SCAN_AT(fterm_scan[3])},
    {"sub-build blocks", ROWS(WS_SB_BLOCKS), CAP(sbws_blocks), WS_EIGHTH, false, NO_SCAN},
    {"sub-build chunks", ROWS(WS_SB_CHUNKS), CAP(sbws_chunks), WS_EIGHTH, false, NO_SCAN},
    {"update blocks", ROWS(WS_UPD_BLOCKS), CAP(uws_blocks), WS_EIGHTH, false, NO_SCAN},
    {"update pieces", ROWS(WS_UPD_PIECES), CAP(uws_pieces), WS_EIGHTH, false, NO_SCAN},
    {"select tiles", ROWS(WS_SELECT), CAP(sws_tiles), WS_DOUBLE, false, SCAN_AT(sel_scan)},
};

/* Room in one group (ws_grow): HUFE_OK; HUFE_FATAL with the error text for a hard group; HUFE_MEMORY, silently, for a
 * soft one.  A failed growth leaves the group without buffers and at capacity 0. */
static int grow_ws(hufgpu_ctx *c, int group, uint64_t need0, uint64_t need1 = 0)
{
    if (ws_grow(&WS_HIP, c, &WS[group], need0, need1) == 0) return HUFE_OK;
    if (WS[group].soft) return HUFE_MEMORY;
    set_err(c, "no workspace for %s (%llu, %llu): %s", WS[group].name, (unsigned long long)need0, (unsigned long long)need1,
            hipGetErrorString(g_ws_error));
    return HUFE_FATAL;
}
static int grow_ws2(hufgpu_ctx *c, int g0, uint64_t need0, int g1, uint64_t need1)
{
    const int rc = grow_ws(c, g0, need0);
    return rc ? rc : grow_ws(c, g1, need1);
}

static int ensure_encode_ws(hufgpu_ctx *c, uint64_t nblocks)
{
    const bool grows = nblocks > c->ws_blocks;
    const int rc = grow_ws(c, G_ENCODE, nblocks);
    if (grows) ws_release(&WS_HIP, c, &WS[G_CHUNK]);   /* the chunk arrays have always gone with it (grow_ws has waited) */
    return rc;
}
static int ensure_chunk_ws(hufgpu_ctx *c, uint64_t nchunks) { return grow_ws(c, G_CHUNK, nchunks); }
static int ensure_decode_ws(hufgpu_ctx *c, uint64_t nblocks) { return grow_ws(c, G_DECODE, nblocks); }
static int ensure_batch_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nitems) { return grow_ws(c, G_BATCH, nblocks, nitems); }
static int ensure_range_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nranges) { return grow_ws(c, G_RANGE, nblocks, nranges); }
static int ensure_gather_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nparts) { return grow_ws2(c, G_GATHER_BLOCKS, nblocks, G_GATHER_PARTS, nparts); }
static int ensure_find_ws(hufgpu_ctx *c, uint64_t nwords, uint64_t ntiles) { return grow_ws2(c, G_FIND_WORDS, nwords, G_FIND_TILES, ntiles); }
static int ensure_update_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t npieces) { return grow_ws2(c, G_UPD_BLOCKS, nblocks, G_UPD_PIECES, npieces); }
static int ensure_sub_build_ws(hufgpu_ctx *c, uint64_t nblocks, uint64_t nchunks) { return grow_ws2(c, G_SB_BLOCKS, nblocks, G_SB_CHUNKS, nchunks); }

/* The scratch area that hufgpu_decode_ranges, hufgpu_build_sub_index, hufgpu_update_ranges and hufgpu_append share: at
 * least `bytes` bytes, with an eighth of room to grow into when that can be had.  HUFE_MEMORY (the area is then gone)
 * when it cannot; the caller words the error. */
static int grow_range_scratch(hufgpu_ctx *ctx, uint64_t bytes)
{
    if (bytes <= ctx->rscratch_bytes) return HUFE_OK;
    if (bytes > ((uint64_t)1 << 46)) {
        (void)ws_hip_wait();
        ws_release(&WS_HIP, ctx, &WS[G_RSCRATCH]);
        return HUFE_MEMORY;
    }
    if (grow_ws(ctx, G_RSCRATCH, bytes + bytes / 8) == HUFE_OK) return HUFE_OK;
    return grow_ws(ctx, G_RSCRATCH, bytes);
}

static void free_batch_stage(hufgpu_ctx *c)
{
    if (c->bstage_pending) (void)hipEventSynchronize(c->bstage_ev);
    ws_release(&WS_HIP, c, &WS[G_BSTAGE]);
    c->bstage_pending = 0;
}

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

/* the device side of a new context: the fixed group and the zipf weights */
static int ctx_init(hufgpu_ctx *ctx)
{
    HIP_OK(NULL, hipSetDevice(ctx->device));
    const int rc = grow_ws(ctx, G_FIXED, 1);
    if (rc) return rc;
    /* zipf255 cumulative weights: w_r = floor(2^32 / r), r = 1..255 */
    uint64_t cum[255], acc = 0;
    for (int r = 1; r <= 255; r++) {
        acc += (1ull << 32) / (uint64_t)r;
        cum[r - 1] = acc;
    }
    HIP_OK(ctx, hipMemcpy(ctx->d_zipf, cum, sizeof(cum), hipMemcpyHostToDevice));
    return HUFE_OK;
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
    const int rc = ctx_init(ctx);
    if (rc) {
        (void)hufgpu_ctx_destroy(ctx);   /* (the text stays in hufgpu_last_error(NULL)) */
        return rc;
    }
    *out = ctx;
    return HUFE_OK;
}

extern "C" int hufgpu_ctx_device(const hufgpu_ctx_t *ctx) { return ctx ? ctx->device : -1; }

extern "C" int hufgpu_ctx_destroy(hufgpu_ctx_t *ctx)
{
    if (!ctx) return HUFE_ARGUMENT;
    (void)hipSetDevice(ctx->device);
    (void)ws_hip_wait();
    free_batch_stage(ctx);
    if (ctx->bstage_ev) (void)hipEventDestroy(ctx->bstage_ev);
    ws_release_all(&WS_HIP, ctx, WS, G_COUNT);
    if (ctx->ev) {
        for (int k = 0; k < PROF_SLOTS; k++)
            for (int i = 0; i <= MAX_STAGES; i++) (void)hipEventDestroy(ctx->ev[k][i]);
        free(ctx->ev);
    }
    free(ctx);
    return HUFE_OK;
}

static inline hipStream_t pick_stream(hufgpu_ctx *c, void *stream) { (void)c; return (hipStream_t)stream; }
static inline unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

/* scatter.hpp - the kernels of hufgpu_scatter (include/huffman_gpu.h): records of the original data overwritten in one
   indexed stream, out of place, their positions, lengths and new bytes all in device memory; the host knows the sizes of
   the caller's arrays and a cap on the touched blocks and nothing else, and only enqueues.  Part of hufgpu_kernels.hip
   (one translation unit, gfx950 only).

   It is hufgpu_update_ranges' pipeline (update.hpp) with the plan the host waits for there replaced by bounds the host
   has before anything runs: the layout is fixed-blocksize, so a record's blocks follow from a division, and the caller's
   touched_cap sizes the scratch area, the rows and the row grids.

     scat_zero_kernel       the call's first launch: the counters of the call and the caller's result words zeroed;
     decode_prepare_kernel  as it is: every header, the block lengths' sums;
     scat_mark_kernel       gather_mark_kernel's twin: one count for every block a record has bytes in (a part), the
                            lowest record with len_i > max_len;
     gather_scan_kernel, gather_place_kernel  as they are: a block's segment of the part list, the list of touched blocks;
     scat_class_kernel      one thread a block: copy / void / staged (update.hpp's kinds; there is no direct kind: whether
                            a block lies wholly inside one record would need the records sorted).  A touched block that
                            can be served takes a row with an atomic add; row r's scratch entry is r * stride, known
                            before the launch.  A row at or above touched_cap is not staged, a touched block whose header
                            failed or whose block_len is not the layout's records its status and is not staged either:
                            both keep their old record, decoders off (block_len = 0 in the context's copy);
     the indexed decoders   as they are, into the scratch entries;
     scat_overlay_kernel    every part over its block's scratch entry, dealt by part and by 16-byte piece;
     scat_fail_kernel       the first staged block that did not decode;
     scat_hist_lanes_kernel / scat_tree_wave_kernel / scat_hist_tree_kernel / scat_pack_rows_kernel
                            update.hpp's row kernels in grids touched_cap wide: a row at or above the device's row count
                            does nothing (its tree wave still takes its ticket of the size scan, with 0 bytes, so the
                            tickets come back to zero);
     upd_index_kernel, upd_piece_kernel, update_copy_kernel, upd_sub_rows_kernel  as they are;
     scat_result_kernel     folds what was recorded into the caller's four result words.

   Whatever the status, nothing outside the caller's output buffers and the context's workspaces is written: a record is
   cut at raw_size and at its blocks' borders by gather_place_kernel, a part is overlaid only where the block's header
   length is the layout's, pack and copy write nothing when the new index does not fit out_cap. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "gather.hpp"
#include "update.hpp"

namespace hufgpu {

/* scount[]: what the kernels of one call hand to scat_result_kernel (zero when the first kernel starts) */
#define SCAT_TOUCHED   0            /* touched blocks, staged or not */
#define SCAT_BAD_LEN   1            /* ~(the lowest record with len_i > max_len) (0: none) */
#define SCAT_BAD_BLOCK 2            /* ~((the first touched block that cannot be served << 8) | its status) (0: none) */
#define SCAT_WORDS     4

struct ScatterArgs {
    GatherArgs g;                           /* the grouping by block: g.out, g.errs and g.raw_lens are not used */
    HufDecodeMeta *dmeta;                   /* decode_prepare_kernel's (the context's copy: only staged blocks keep their block_len) */
    const int32_t *status;
    TwoLevel lens;                          /* decode_prepare_kernel's sums of the block lengths */
    const uint64_t *old_offsets;            /* [nblocks + 1] the old block index */
    uint64_t stream_len;
    uint64_t *bprefix;                      /* [nblocks + 1] out: the sums of the header lengths (upd_sub_rows_kernel reads them) */
    uint64_t *obase;                        /* [nblocks] out: a staged block's scratch entry, from the scratch area */
    uint32_t *kind;                         /* [nblocks] out: UPD_COPY / UPD_VOID / UPD_STAGED */
    uint32_t *row_of, *row_blk;             /* [nblocks], [touched_cap] */
    uint64_t *pairs;                        /* [2 touched_cap] (scratch entry, length) */
    unsigned long long *ucount;             /* [UPD_WORDS] UPD_N_TOUCHED: the rows asked for; UPD_TOTAL: the new length */
    unsigned long long *scount;             /* [SCAT_WORDS] */
    uint64_t touched_cap, stride;           /* rows there is room for; bytes a scratch entry */
    uint8_t *scratch;
    const uint8_t *src;                     /* the records' new bytes (NULL with fill) */
    uint32_t fill_on, fill;
    uint32_t group_log2;                    /* threads that share a part in the overlay: 2^group_log2 pieces of 16 bytes */
    uint32_t smax;                          /* such groups a part can need, at most */
    uint32_t shares;                        /* workgroups a touched block's parts are dealt to */
    uint64_t out_cap;
    uint64_t *result;                       /* the caller's four words */
};

/* The call's first launch, one thread per word: the part counts and cursors of the blocks, the counters of the row
 * kernels and of this file, the caller's result words.  A kernel and not three memsets: the call is made to be captured
 * and replayed, and a graph of kernels alone has one kind of node. */
__global__ __launch_bounds__(256) void scat_zero_kernel(ScatterArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * a.g.s.nblocks) a.g.cnt[i] = 0;                   /* (cur lies behind cnt) */
    if (i < UPD_WORDS) a.ucount[i] = 0;
    if (i < SCAT_WORDS) a.scount[i] = 0;
    if (i < 4) a.result[i] = 0;
}

__global__ __launch_bounds__(256) void scat_mark_kernel(ScatterArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.g.nrecords) return;
    uint64_t pos;
    uint32_t n;
    bool too_long;
    const bool any = gather_record(a.g, i, pos, n, too_long);
    if (too_long) atomicMax(&a.scount[SCAT_BAD_LEN], ~(unsigned long long)i);
    if (!any) return;
    const uint64_t fb = pos / a.g.s.bsize, lb = (pos + n - 1) / a.g.s.bsize;
    for (uint64_t b = fb; b <= lb; b++) atomicAdd(&a.g.cnt[b], 1u);
}

/* One thread per block (and one for P's last entry), behind decode_prepare_kernel and the grouping. */
__global__ __launch_bounds__(256) void scat_class_kernel(ScatterArgs a)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t nb = a.g.s.nblocks;
    if (b > nb) return;
    a.bprefix[b] = b == nb ? *a.lens.total : a.lens.gprefix[b / SCAN_GROUP] + a.lens.local[b];
    if (b == nb) return;
    const HufDecodeMeta m = a.dmeta[b];
    bool staged = false;
    uint64_t o = 0;
    if (a.g.cnt[b] != 0u) {
        atomicAdd(&a.scount[SCAT_TOUCHED], 1ull);
        const uint64_t blen = dmin<uint64_t>(a.g.s.bsize, a.g.s.raw_size - b * a.g.s.bsize);
        const uint64_t err = m.status != HUFE_OK ? (uint64_t)(uint32_t)m.status : (m.block_len != blen ? (uint64_t)HUFE_RW : 0ull);
        if (err) {
            atomicMax(&a.scount[SCAT_BAD_BLOCK], ~(unsigned long long)((b << 8) | (err & 0xffu)));
        } else {
            const uint64_t row = atomicAdd(&a.ucount[UPD_N_TOUCHED], 1ull);
            if (row < a.touched_cap) {          /* (a row behind the cap: SCAT_TOUCHED is above it as well, the call fails) */
                staged = true;
                o = row * a.stride;
                a.row_of[b] = (uint32_t)row;
                a.row_blk[row] = (uint32_t)b;
                a.pairs[2 * row] = o;
                a.pairs[2 * row + 1] = blen;
            }
        }
    }
    uint32_t kind = UPD_STAGED;
    if (!staged) {
        const uint64_t o0 = a.old_offsets[b], o1 = a.old_offsets[b + 1];
        kind = (o0 <= o1 && o1 <= a.stream_len) ? UPD_COPY : UPD_VOID;
        if (m.block_len != 0) a.dmeta[b].block_len = 0;
    }
    a.kind[b] = kind;
    a.obase[b] = o;
}

/* After the decoders: every part over its block's scratch entry.  The walk is gather_serve_kernel's - unit u is share
 * u % shares of touched block u / shares, the number of units is read from device memory.  Inside a block the work is
 * dealt by part and by 16-byte piece of the DESTINATION: 2^group_log2 neighbouring threads share a part, thread k of them
 * owns the k-th aligned 16-byte line the part has bytes in.  A line wholly inside the part is one 16-byte store (of the
 * fill word, or of a 16-byte load at any alignment of the source); the part's first and last line are written byte by
 * byte, so no byte outside the part is written - and the part lies inside [entry, entry + block_len) because
 * gather_place_kernel cut it at the block's borders and scat_class_kernel saw the header's length to be the layout's.
 * Ten thousand 5-byte parts are 128 parts a workgroup a step (group_log2 = 1); one part of 60 KiB is 3 841 lines over
 * the workgroups of its block.  Parts that overlap write the same bytes in any order: with fill the value is one, in
 * source mode each byte is one record's. */
__global__ __launch_bounds__(256) void scat_overlay_kernel(ScatterArgs a)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    typedef uint32_t v4u_any __attribute__((ext_vector_type(4), aligned(1)));
    const GatherArgs &g = a.g;
    const uint64_t units = (*g.scan.total >> 32) * a.shares;
    const uint32_t gsize = 1u << a.group_log2;
    const uint32_t sub = threadIdx.x >> a.group_log2, k_in = threadIdx.x & (gsize - 1u);
    const uint32_t per_step = 256u >> a.group_log2;
    const uint32_t w = a.fill * 0x01010101u;
    v4u fillv;
    fillv.x = w; fillv.y = w; fillv.z = w; fillv.w = w;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t share = (uint32_t)(u % a.shares);
        const uint64_t b = g.list[u / a.shares];
        if (a.kind[b] != UPD_STAGED) continue;
        const uint64_t nids = (uint64_t)g.cnt[b] * a.smax;          /* id = part * smax + the group's number inside the part */
        const uint32_t seg = (uint32_t)two_level_prefix(g.scan, b);
        uint8_t *entry = a.scratch + a.obase[b];
        const uint64_t p0 = b * g.s.bsize;
        for (uint64_t id = (uint64_t)share * per_step + sub; id < nids; id += (uint64_t)a.shares * per_step) {
            const uint64_t pi = a.smax == 1u ? id : id / a.smax;
            const uint64_t sg = a.smax == 1u ? 0ull : id % a.smax;
            const GatherPart part = g.parts[seg + pi];
            uint8_t *dst = entry + (part.start - p0);
            const uint64_t n = part.n;
            const uint64_t mis = (uint64_t)((uintptr_t)dst & 15u);
            const uint64_t k = sg * gsize + k_in;                   /* line k covers the part's bytes [16 k - mis, 16 k + 16 - mis) */
            if (16u * k >= mis + n) continue;
            const uint64_t lo = 16u * k < mis ? 0ull : 16u * k - mis;
            const uint64_t hi = dmin<uint64_t>(n, 16u * k + 16u - mis);
            if (hi - lo == 16u) {
                v4u v = fillv;
                if (!a.fill_on) v = *reinterpret_cast<const v4u_any *>(a.src + part.dst + lo);
                *reinterpret_cast<v4u *>(dst + lo) = v;
            } else if (a.fill_on) {
                for (uint64_t j = lo; j < hi; j++) dst[j] = (uint8_t)a.fill;
            } else {
                const uint8_t *from = a.src + part.dst;
                for (uint64_t j = lo; j < hi; j++) dst[j] = from[j];
            }
        }
    }
}

/* One thread per block, after the decoders: the first staged block that did not decode, in stream order, with what the
 * decoders say of it. */
__global__ __launch_bounds__(256) void scat_fail_kernel(ScatterArgs a)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.g.s.nblocks || a.kind[b] != UPD_STAGED) return;
    const int32_t st = a.status[b];
    if (st != HUFE_OK) atomicMax(&a.scount[SCAT_BAD_BLOCK], ~(unsigned long long)((b << 8) | ((uint64_t)(uint32_t)st & 0xffu)));
}

/* ---- the row kernels of update.hpp in grids as wide as the cap: a row at or above *rows does nothing ---- */

template <int THREADS>
__global__ __launch_bounds__(THREADS, HL_WAVES_PER_SIMD) void scat_hist_lanes_kernel(const uint8_t *__restrict__ base,
                                                                                     const uint64_t *__restrict__ pairs,
                                                                                     uint32_t *__restrict__ hist,
                                                                                     const unsigned long long *__restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) uint8_t hl_lds[HL_LDS_BYTES];
    const uint64_t row = blockIdx.x;
    if (row >= *rows) return;
    hl_count<THREADS>(hl_lds, base + pairs[2 * row], pairs[2 * row + 1], hist + row * HUF_NSYM);
}

__global__ __launch_bounds__(64, 8) void scat_tree_wave_kernel(const uint32_t *__restrict__ hist, hufcode_t *__restrict__ codetab,
                                                               int16_t *__restrict__ treebuf, HufBlockMeta *__restrict__ meta,
                                                               TwoLevel sizes, const unsigned long long *__restrict__ rows)
{
    __shared__ TreeLds L;
    const uint64_t blk = blockIdx.x;
    if (blk >= *rows) {
        two_level_arrive(sizes, blk, gridDim.x, 0);
        return;
    }
    const int lane = lane_id();
    uint32_t rate[4];
#pragma unroll
    for (int j = 0; j < 4; j++) rate[j] = hist[blk * HUF_NSYM + lane + 64 * j];
    const uint64_t bytes = tree_fast_wave(rate, L, blk, codetab, treebuf, meta);
    two_level_arrive(sizes, blk, gridDim.x, bytes);
}

template <int THREADS, bool PACKED>
__global__ __launch_bounds__(THREADS) void scat_hist_tree_kernel(const uint8_t *__restrict__ base, const uint64_t *__restrict__ pairs,
                                                                 hufcode_t *__restrict__ codetab, int16_t *__restrict__ treebuf,
                                                                 HufBlockMeta *__restrict__ meta, TwoLevel sizes,
                                                                 const unsigned long long *__restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_union[HistTreeLds<THREADS, PACKED>::UBYTES];
    __shared__ uint32_t s_side[2 * THREADS];
    const uint64_t row = blockIdx.x;
    if (row >= *rows) {
        if (threadIdx.x < 64) two_level_arrive(sizes, row, gridDim.x, 0);
        return;
    }
    hist_tree_block<THREADS, PACKED>(base + pairs[2 * row], pairs[2 * row + 1], row, codetab, treebuf, meta, sizes, s_union, s_side);
}

template <int THREADS, bool SHORT>
__global__ __launch_bounds__(THREADS, SHORT ? PACK_WAVES_PER_SIMD : 4) void scat_pack_rows_kernel(const uint8_t *__restrict__ base,
                                                                                           const uint64_t *__restrict__ pairs,
                                                                                           const uint32_t *__restrict__ row_blk,
                                                                                           const hufcode_t *__restrict__ codetab,
                                                                                           const int16_t *__restrict__ treebuf,
                                                                                           const HufBlockMeta *__restrict__ meta,
                                                                                           uint64_t *__restrict__ offsets, uint64_t nblocks,
                                                                                           uint64_t out_cap,
                                                                                           uint8_t *__restrict__ out, HufSubIndex sub,
                                                                                           const unsigned long long *__restrict__ rows)
{
    __shared__ hufcode_t s_code[HUF_NSYM];
    __shared__ uint32_t s_part[THREADS / 64];
    __shared__ uint32_t s_tail[THREADS / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[PACK_STAGE_WORDS];
#ifdef PACK_VGPR_SLACK      /* test builds only: as pack_kernel */
    asm volatile("; one VGPR more than the kernel uses" ::: PACK_VGPR_SLACK);
#endif
    const uint64_t row = blockIdx.x;
    if (row >= *rows || offsets[nblocks] > out_cap) return;
    TwoLevel sizes = {};                 /* local = NULL: the place comes from the finished index */
    pack_block_any<THREADS, SHORT>(base + pairs[2 * row], pairs[2 * row + 1], row, row_blk[row], codetab, treebuf, meta, offsets,
                                   sizes, out, sub, s_code, s_part, s_tail, s_stage);
}

/* One workgroup, last: the call's four result words - status, new length, touched blocks, the record or block that
 * caused the status - the first condition that holds, in the order of the header. */
__global__ __launch_bounds__(64) void scat_result_kernel(ScatterArgs a)
{
    if (threadIdx.x != 0) return;
    const uint64_t touched = a.scount[SCAT_TOUCHED], bad_len = a.scount[SCAT_BAD_LEN], bad_block = a.scount[SCAT_BAD_BLOCK];
    const uint64_t total = a.ucount[UPD_TOTAL];
    uint64_t status = HUFE_OK, who = ~0ull;
    if (bad_len) {
        status = HUFE_ARGUMENT;
        who = ~bad_len;
    } else if (touched > a.touched_cap) {
        status = HUFE_MEMORY;
    } else if (bad_block) {
        status = ~bad_block & 0xffu;
        if (status == HUFE_OK) status = HUFE_FATAL;
        who = ~bad_block >> 8;
    } else if (total > a.out_cap) {
        status = HUFE_MEMORY;
    }
    a.result[0] = status;
    a.result[1] = status ? 0ull : total;
    a.result[2] = touched;
    a.result[3] = who;
}

/* a call without records: the stream was copied (or did not fit) */
__global__ __launch_bounds__(64) void scat_copy_result_kernel(uint64_t *__restrict__ result, uint64_t status, uint64_t len)
{
    if (threadIdx.x != 0) return;
    result[0] = status;
    result[1] = status ? 0ull : len;
    result[2] = 0;
    result[3] = ~0ull;
}

}  // namespace hufgpu

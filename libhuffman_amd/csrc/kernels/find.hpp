/* find.hpp - the kernels of hufgpu_find_bytes (include/huffman_gpu.h): where in the original data the bytes of a set
   of byte values lie, straight from stream, block index and sub-index; no decoded byte reaches device memory and the
   host only enqueues.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   Positions are the layout's, as in gather.hpp: block b holds [b B, b B + min(B, raw_size - b B)).

     find_sub_kernel     workgroup = one (block, chunk of 65 536 symbols), decode_sub_kernel's geometry with eight waves;
                         a wave takes the chunk's tiles wave, wave + 8, ...  The header is parsed and its length must
                         be the layout's, the tables come from dsub_fast_tables (the claimed code lengths checked
                         against the stream's tree), and EVERY tile of EVERY chunk is the item of sub_tile.hpp, with
                         its checks: (a) the block's first tile starts at payload bit 0, (b) every group takes
                         exactly the bits it is said to have and no walk leaves tree or payload, (c) a tile ends where
                         the next tile of the block is said to start (the last: inside the payload).  The whole block
                         is walked, so the induction of decode_sub.hpp closes and the caller vouches for nothing: a
                         block is served exactly or its status says that it is not.
                         A lane's 32 decoded bytes lie in the wave's 2 KiB of LDS (dsub_tile_slow, the step-by-step
                         route of sub_tile.hpp: codes of any length, groups of any size) and are tested against the
                         set - eight words in LDS - there; what leaves the workgroup is ONE 32-bit match mask per
                         group (a bitmap row per block: block starts need not be 32-aligned raw positions) and the
                         tile's match count.  A block of one byte value has no sub-index rows: its payload bits are
                         seen to be 0 and its mask words are all ones or all zeros, the last one cut at the block's
                         end.
     find_scan_kernel    the tile counts, gated by their block's status, summed by the two-level / ticket scan of
                         offsets.hpp (as gather_scan_kernel): a tile's rank among the matches of the served blocks; the
                         grand total goes to d_totals[0], the blocks that are not served are counted into d_totals[2];
     find_finish_kernel  per-block counts as differences of the tiles' ranks, and d_totals[1];
     find_emit_kernel    one wave a tile, a lane a mask word: rank = the tile's + the wave's scan of popcounts, and
                         b B + 32 g + bit goes to d_pos[rank] for every set bit whose rank is below pos_cap.

   Any failed check of any chunk raises the block's status to HUF_ERROR_READ_WRITE (atomic max; the statuses are zero
   when the first kernel starts); nothing is decided on the host. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "sub_tile.hpp"

namespace hufgpu {

#define FIND_THREADS 512                    /* as RTILE_THREADS (range_tiles.hpp): decode_sub.hpp's step-by-step functions are instantiated for 512 threads already,
                                               and decode_sub_kernel<256>'s code does not depend on what is called from here */
#define FIND_WAVES (FIND_THREADS / 64)
#define FIND_EMIT_THREADS 256

struct FindArgs {
    SubStream s;
    uint32_t cpb;                           /* chunks a block */
    uint32_t set[8];                        /* bit v: byte value v is looked for */
    uint32_t *bitmap;                       /* [nblocks][wpb] match masks, one word a group */
    uint64_t wpb;
    uint32_t *tcnt;                         /* [nblocks][tpb] matches of a tile */
    uint64_t tpb, ntiles;                   /* ntiles = nblocks * tpb */
    TwoLevel scan;                          /* of the gated tile counts; scan.total = d_totals */
    uint64_t *pos;
    uint64_t pos_cap;
    uint64_t *block_counts;                 /* optional */
    uint64_t *totals;
    int32_t *errs;
};

__device__ __forceinline__ uint64_t find_block_len(const FindArgs &a, uint64_t b)
{
    return dmin<uint64_t>(a.s.bsize, a.s.raw_size - b * a.s.bsize);
}

/* grid nblocks * cpb */
__global__ __launch_bounds__(FIND_THREADS) void find_sub_kernel(FindArgs a)
{
    typedef DsubShared<FIND_THREADS> SH;
    __shared__ SH sh;
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[FIND_WAVES][HUF_SUB_TILE / 4];
    __shared__ uint32_t s_set[8];
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    const uint64_t b = blockIdx.x / a.cpb;
    const uint32_t c = blockIdx.x % a.cpb;
    const uint64_t blen = find_block_len(a, b);
    const uint64_t sym0 = (uint64_t)c * DSUB_CHUNK_SYMS;
    if (sym0 >= blen) return;                                       /* (the short last block has fewer chunks) */
    const uint64_t sym1 = dmin<uint64_t>(blen, sym0 + DSUB_CHUNK_SYMS);
    if (threadIdx.x < 8) s_set[threadIdx.x] = a.set[threadIdx.x];
    __syncthreads();
    /* ---- the header - and its length must be the layout's ---- */
    BlockHeader h;
    if (parse_block_header(a.s.stream, a.s.stream_len, a.s.offsets[b], a.s.offsets[b + 1], a.s.max_tree, h) != HUFE_OK || h.block_len != blen) {
        if (threadIdx.x == 0) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
        return;
    }
    const SubBlockView v = sub_block_view(h, a.s.sub, b);
    uint32_t *row = a.bitmap + b * a.wpb;
    uint32_t *trow = a.tcnt + b * a.tpb;
    const int leaf = h.tree_len == 5 ? single_leaf_symbol(h.tree) : -1;
    if (leaf >= 0) {
        /* ---- one byte value: every symbol is a 0 bit (decode.hpp); the chunk's bits are seen to be 0 ---- */
        if (blen > v.pay_bits) {
            if (threadIdx.x == 0) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
            return;
        }
        const bool match = ((s_set[(uint32_t)leaf >> 5] >> ((uint32_t)leaf & 31u)) & 1u) != 0u;
        bool set = false;
        for (uint64_t g = (sym0 >> 5) + threadIdx.x; 32ull * g < sym1; g += FIND_THREADS) {
            const uint32_t nsym = (uint32_t)dmin<uint64_t>(DSUB_SPL, blen - 32ull * g);
            uint32_t x = load_be32(v.pay, 4ull * g, v.pay_bytes);
            if (nsym < 32u) x &= 0xffffffffu << (32u - nsym);
            set |= x != 0u;
            row[g] = match ? (nsym < 32u ? (1u << nsym) - 1u : 0xffffffffu) : 0u;
        }
        for (uint64_t t = sym0 / HUF_SUB_TILE + threadIdx.x; t * HUF_SUB_TILE < sym1; t += FIND_THREADS)
            trow[t] = match ? (uint32_t)dmin<uint64_t>(HUF_SUB_TILE, blen - t * HUF_SUB_TILE) : 0u;
        if (set) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
        return;
    }
    /* ---- the block's tables ---- */
    const DsubTreeWords tw = dsub_tree_request<FIND_THREADS>(h.tree, h.tree_len, a.s.sub.lens + b * HUF_NSYM);
    if (!dsub_fast_tables<FIND_THREADS>(sh, h.tree_len, tw)) {      /* (workgroup-uniform) */
        if (threadIdx.x == 0) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
        return;
    }
    uint32_t *tile_words = s_tile[wave];
    uint32_t *top = DsubLds<FIND_THREADS>::slice(sh, (int)wave) + (SH::SLICE_WORDS - 1u);
    bool good = true;
    /* ---- the chunk's tiles, one wave each, every one of them ---- */
    for (uint64_t t = sym0 / HUF_SUB_TILE + wave; t * HUF_SUB_TILE < sym1; t += FIND_WAVES) {
        uint32_t nsym;
        if (!sub_tile_checked<FIND_THREADS>(sh, top, v, t, reinterpret_cast<uint8_t *>(tile_words), nsym)) {
            good = false;
            continue;
        }
        /* the lane's own 32 bytes (it wrote them itself) against the set */
        const uint4 lo4 = *reinterpret_cast<const uint4 *>(tile_words + 8u * lane);
        const uint4 hi4 = *reinterpret_cast<const uint4 *>(tile_words + 8u * lane + 4u);
        const uint32_t w[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t x = (w[j] >> (8 * i)) & 0xffu;
                m |= ((s_set[x >> 5] >> (x & 31u)) & 1u) << (4 * j + i);
            }
        }
        m = nsym == 0u ? 0u : (nsym < 32u ? m & ((1u << nsym) - 1u) : m);        /* (bytes behind a short group are stale) */
        if (nsym != 0u) row[t * 64u + lane] = m;
        const uint32_t cnt = wave_lane_u32(wave_incl_scan_u32((uint32_t)__popc(m)), 63);
        if (lane == 0) trow[t] = cnt;
    }
    if (!good && lane == 0) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
}

/* a workgroup = one SCAN_GROUP of tiles, as gather_scan_kernel sums the part counts */
__global__ __launch_bounds__(SCAN_GROUP) void find_scan_kernel(FindArgs a)
{
    __shared__ uint64_t s_part[SCAN_GROUP / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_GROUP + threadIdx.x;
    uint64_t c = 0;
    if (i < a.ntiles) {
        const uint64_t b = i / a.tpb, t = i % a.tpb;
        const bool served = a.errs[b] == HUFE_OK;
        if (served && t * HUF_SUB_TILE < find_block_len(a, b)) c = a.tcnt[i];
        if (!served && t == 0) atomicAdd((unsigned long long *)&a.totals[2], 1ull);
    }
    scan_group_publish<SCAN_GROUP>(a.scan, i, a.ntiles, c, s_part);
}

/* one thread per block */
__global__ __launch_bounds__(256) void find_finish_kernel(FindArgs a)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b == 0) a.totals[1] = dmin<uint64_t>(a.totals[0], a.pos_cap);
    if (b >= a.s.nblocks || !a.block_counts) return;
    const uint64_t end = b + 1 < a.s.nblocks ? two_level_prefix(a.scan, (b + 1) * a.tpb) : a.totals[0];
    a.block_counts[b] = end - two_level_prefix(a.scan, b * a.tpb);
}

/* a wave = one tile */
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_emit_kernel(FindArgs a)
{
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    const uint64_t i = (uint64_t)blockIdx.x * (FIND_EMIT_THREADS / 64) + wave;
    if (i >= a.ntiles) return;
    const uint64_t b = i / a.tpb, t = i % a.tpb;
    const uint64_t blen = find_block_len(a, b);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK) return;
    const uint64_t rank0 = two_level_prefix(a.scan, i);
    if (rank0 >= a.pos_cap) return;
    const uint64_t g = t * 64u + lane;
    uint32_t m = g * DSUB_SPL < blen ? a.bitmap[b * a.wpb + g] : 0u;
    uint64_t r = rank0 + (wave_incl_scan_u32((uint32_t)__popc(m)) - (uint32_t)__popc(m));
    const uint64_t base = b * a.s.bsize + g * DSUB_SPL;
    while (m != 0u && r < a.pos_cap) {
        a.pos[r++] = base + (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
    }
}

}  // namespace hufgpu

/* range_tiles.hpp - drange_tiles_kernel: the tile route of hufgpu_decode_ranges (HUFGPU_RANGES_TILES,
   include/huffman_gpu.h): of a block at a range's cut edge only the sub-index tiles of 2 048 symbols that hold bytes of the
   range are decoded, straight into the range's slot.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   Which blocks go this way is decided by drange_class_kernel (ranges.hpp, DRANGE_TILES): the caller vouches for the
   sub-index, the block's header length is the layout's (the sub-index rows are addressed by it), its tree has more than
   one leaf, and the (range, tile) pairs over it - counted by drange_mark_kernel - are no more than its tiles, so that
   this route never decodes more symbols than the whole block has.  With that rule a range that covers such a block
   whole is the only one over it and the block is direct: a tile-routed block is the FIRST or the LAST block of every
   range that touches it, and this kernel looks at those two blocks of each range only.

   One item = one (range, block, tile), taken by one wave.  Workgroup (i, y) builds the tables of range i's first block
   once (dsub_fast_tables: the claimed code lengths checked against the stream's tree) and its eight waves take the items
   8 y + wave, 8 (y + gridDim.y) + wave, ... of that block, then the same for the range's last block: a range of
   thousands of tiles inside one giant block is the work of all y workgroups, a workgroup without an item leaves before
   the table build.  Two ranges in one block build the block's tables once each.

   An item is the item of sub_tile.hpp (sub_tile_checked), with its checks - for EVERY group of the tile, also those
   outside the range: the lanes of a wave run in lockstep, so the groups outside the range cost LDS look-ups but no time,
   and with them damage anywhere in a touched tile is seen, not only in the groups that are delivered.  What cannot be
   checked is that tile_bits[t] is where the in-order decoder arrives: that is the caller's word (the flag).  No group
   fails over for being unusual.

   Any failure puts the block on the call's fail count, once (a bit in the block's pair word says it is listed); the host
   then serves the whole call again by the staged route.  The decoded tile lies in the wave's 2 KiB of LDS; the part
   inside [lo, hi) goes to slot + (position - lo): bytes up to the slot's first 16-byte boundary, 16-byte stores, bytes
   behind the last of them.  Nothing else is written. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "ranges.hpp"
#include "sub_tile.hpp"

namespace hufgpu {

/* Eight waves, not decode_sub_kernel's four: the step-by-step device functions of decode_sub.hpp are then instantiated
 * for this kernel alone, and decode_sub_kernel's code does not depend on what is called from here. */
#define RTILE_THREADS 512
#define RTILE_WAVES (RTILE_THREADS / 64)
#define RTILE_FAILED (1ull << 63)           /* in DecRangeArgs::tpairs[b]: the block is on the fail count */

__device__ __forceinline__ void rtile_fail(const DecRangeArgs &a, uint64_t b)
{
    if ((atomicOr(&a.tpairs[b], RTILE_FAILED) & RTILE_FAILED) == 0ull) atomicAdd(&a.counters[6], 1ull);
}

/* grid (nranges, y) */
__global__ __launch_bounds__(RTILE_THREADS) void drange_tiles_kernel(DecRangeArgs a, SubStream ta)
{
    typedef DsubShared<RTILE_THREADS> SH;
    __shared__ SH sh;
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[RTILE_WAVES][HUF_SUB_TILE / 4 + 8];
    const uint64_t i = blockIdx.x;
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1], fb = a.rplan[4 * i + 2], lb = a.rplan[4 * i + 3];
    if (fb > lb) return;                                            /* (also: a slot that is too short) */
    uint8_t *slot = a.dout + a.out_offsets[i];
    uint32_t *tile_words = s_tile[wave];
    uint32_t *top = DsubLds<RTILE_THREADS>::slice(sh, (int)wave) + (SH::SLICE_WORDS - 1u);
    for (int edge = 0; edge < 2; edge++) {
        if (edge == 1 && lb == fb) break;
        const uint64_t b = edge == 0 ? fb : lb;
        if (a.kind[b] != DRANGE_TILES) continue;                     /* (written by an earlier launch: the same for every thread) */
        const uint64_t p0 = a.bprefix[b], blen = a.bprefix[b + 1] - p0;     /* (dmeta's block_len is switched off for the decoders) */
        const uint64_t c0 = dmax<uint64_t>(lo, p0) - p0, c1 = dmin<uint64_t>(hi, p0 + blen) - p0;
        if (c0 >= c1) continue;
        const uint64_t t0 = c0 / HUF_SUB_TILE, nitems = (c1 - 1) / HUF_SUB_TILE - t0 + 1;
        if ((uint64_t)blockIdx.y * RTILE_WAVES >= nitems) continue;
        const HufDecodeMeta m = a.dmeta[b];
        const uint64_t o0 = ta.offsets[b], o1 = dmin<uint64_t>(ta.offsets[b + 1], ta.stream_len);
        const uint8_t *tree = ta.stream + o0 + HUF_HEADER_FIXED;
        const uint8_t *pay = tree + 2 * (int)m.tree_len;
        const BlockHeader h = {blen, m.tree_len, tree, pay, o1 - (o0 + HUF_HEADER_FIXED + 2ull * (uint64_t)m.tree_len)};    /* (the header parsed: it fits) */
        __syncthreads();                                            /* the waves are through with the tables of the other edge */
        const DsubTreeWords tw = dsub_tree_request<RTILE_THREADS>(tree, m.tree_len, ta.sub.lens + b * HUF_NSYM);
        if (!dsub_fast_tables<RTILE_THREADS>(sh, m.tree_len, tw)) {  /* (workgroup-uniform) */
            if (threadIdx.x == 0) rtile_fail(a, b);
            continue;
        }
        const SubBlockView v = sub_block_view(h, ta.sub, b);
        for (uint64_t j = (uint64_t)blockIdx.y * RTILE_WAVES + wave; j < nitems; j += (uint64_t)gridDim.y * RTILE_WAVES) {
            const uint64_t t = t0 + j;
            uint32_t nsym;
            if (!sub_tile_checked<RTILE_THREADS>(sh, top, v, t, reinterpret_cast<uint8_t *>(tile_words), nsym)) {
                if (lane == 0) rtile_fail(a, b);
                continue;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   /* the lanes' bytes are in LDS before other lanes read them */
            __builtin_amdgcn_wave_barrier();
            const uint64_t ts = t * HUF_SUB_TILE;
            const uint64_t s0 = dmax<uint64_t>(c0, ts), s1 = dmin<uint64_t>(c1, ts + HUF_SUB_TILE);
            rtile_store(slot + (p0 + s0 - lo), tile_words, (uint32_t)(s0 - ts), (uint32_t)(s1 - s0));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   /* ... and read before the next item overwrites them */
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace hufgpu

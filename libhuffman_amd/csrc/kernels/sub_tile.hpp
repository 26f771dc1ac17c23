/* sub_tile.hpp - what the routes that serve straight from a stream, its block index and its sub-index share
   (range_tiles.hpp, gather.hpp, find.hpp): their common arguments, a block's view of its sub-index rows, the ONE checked
   tile item, and the store of a decoded tile's bytes.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   An item = one tile of 2 048 symbols, taken by one wave as decode_sub_kernel takes a tile: lane l has group 64 t + l,
   its first bit is tile_bits[t] + the wave's exclusive scan of group_bits.  Checked per item:
     (a) tile_bits[t] lies inside the payload (and is 0 for the block's first tile), no group claims more than 32 codes
         of the longest length can have;
     (c) tile_bits[t] + the SUM of the tile's group_bits is the next tile's recorded start (the block's last tile: inside
         the payload) - summed, not decoded;
     (b) of decode_sub.hpp for EVERY group of the tile: a lane's codewords take exactly the bits its group is said to
         have, no walk leaves the tree or the payload.
   All groups go through decode_sub.hpp's step-by-step path (dsub_tile_slow: staged word by word, codes of any length,
   groups of any size) - there is no separate route for unusual groups.  What an item cannot check is that tile_bits[t]
   is where the in-order decoder arrives: a caller that does not walk the whole block takes that on the caller's word. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "decode_sub.hpp"

namespace hufgpu {

struct SubStream {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *offsets;                /* the block index */
    uint64_t nblocks;
    HufSubIndex sub;
    uint64_t raw_size, bsize;               /* the layout (bsize: never 0) */
    int max_tree;
};

/* block b of the layout, its header parsed and its length seen to be the layout's */
struct SubBlockView {
    const uint8_t *pay;
    uint64_t pay_bytes, pay_bits;
    uint64_t blen, ntiles, ngrp;
    const uint64_t *told;                   /* the block's rows of tile_bits and group_bits */
    const uint16_t *grp;
};

__device__ __forceinline__ SubBlockView sub_block_view(const BlockHeader &h, const HufSubIndex &sub, uint64_t b)
{
    const uint64_t blen = h.block_len;
    return {h.pay, h.pay_bytes, h.pay_bytes * 8ull, blen, (blen + HUF_SUB_TILE - 1) / HUF_SUB_TILE, (blen + DSUB_SPL - 1) / DSUB_SPL,
            sub.tile_bits + b * sub.tpb, sub.group_bits + b * sub.gpb};
}

/* Tile t of the block by the calling wave, the block's tables in sh (dsub_fast_tables), top = the wave's stage.  The
 * verdict is the same in every lane; when it is true the lane's nsym_out decoded bytes (0: no such group) lie at
 * tile_bytes + 32 lane - in LDS, not yet fenced for other lanes. */
template <int THREADS>
__device__ __forceinline__ bool sub_tile_checked(const DsubShared<THREADS> &sh, uint32_t *top, const SubBlockView &v, uint64_t t,
                                                 uint8_t *tile_bytes, uint32_t &nsym_out)
{
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t g = t * 64u + lane;
    uint32_t gb = 0, nsym = 0;
    if (g < v.ngrp) {
        gb = v.grp[g];
        nsym = (uint32_t)dmin<uint64_t>(DSUB_SPL, v.blen - g * DSUB_SPL);
    }
    nsym_out = nsym;
    const uint64_t tfirst = uni64(v.told[t]);
    const uint64_t tnext = uni64(v.told[t + 1 < v.ntiles ? t + 1 : t]);
    const bool wild = __ballot(gb > (uint32_t)DSUB_MAX_GROUP_BITS) != 0ull;
    gb = dmin<uint32_t>(gb, DSUB_MAX_GROUP_BITS);
    const uint32_t incl = wave_incl_scan_u32(gb);
    const uint64_t sum = wave_lane_u32(incl, 63);
    if (wild || tfirst > v.pay_bits || sum > v.pay_bits - tfirst || (t == 0 && tfirst != 0)) return false;        /* (a) */
    if (t + 1 < v.ntiles && tfirst + sum != tnext) return false;                                                   /* (c) */
    const bool ok = dsub_tile_slow<THREADS>(sh, top, v.pay, v.pay_bytes, tfirst, incl - gb, incl, nsym, true,
                                            tile_bytes + DSUB_SPL * lane);                                         /* (b) */
    return __ballot(!ok) == 0ull;
}

/* bytes [s0, s0 + n) of the wave's decoded tile (LDS, `words` 16-byte aligned, readable 8 words past the tile) to dst,
 * which has any alignment: 16-byte stores are aligned on the global side, their four words come from five aligned LDS
 * words shifted into place */
__device__ __forceinline__ void rtile_store(uint8_t *__restrict__ dst, const uint32_t *words, uint32_t s0, uint32_t n)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const uint32_t lane = (uint32_t)lane_id();
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
    const uint32_t head = dmin<uint32_t>(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint32_t chunks = (n - head) >> 4, tail = (n - head) & 15u;
    if (lane < head) dst[lane] = bytes[s0 + lane];
    if (lane < tail) dst[head + 16u * chunks + lane] = bytes[s0 + head + 16u * chunks + lane];
    v4u *d = reinterpret_cast<v4u *>(dst + head);
    for (uint32_t c = lane; c < chunks; c += 64u) {
        const uint32_t off = s0 + head + 16u * c;
        const uint32_t *w = words + (off >> 2);
        const uint32_t sh = 8u * (off & 3u);
        uint32_t x[5];
#pragma unroll
        for (int k = 0; k < 5; k++) x[k] = w[k];
        v4u v;
        /* (v_alignbit_b32 shifts by the amount's low five bits: 0 leaves x[k]) */
        v.x = __builtin_amdgcn_alignbit(x[1], x[0], sh);
        v.y = __builtin_amdgcn_alignbit(x[2], x[1], sh);
        v.z = __builtin_amdgcn_alignbit(x[3], x[2], sh);
        v.w = __builtin_amdgcn_alignbit(x[4], x[3], sh);
        d[c] = v;
    }
}

}  // namespace hufgpu

/* ranges.hpp - the kernels of hufgpu_decode_ranges (include/huffman_gpu.h): byte ranges of the original data out of one
   indexed stream, many ranges in one launch sequence.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   decode_prepare_kernel parses every header and sums the block lengths: block b covers the raw positions
   [P[b], P[b + 1]).  drange_plan_kernel finds every range's first and last block in P, drange_mark_kernel counts the
   ranges over every block, drange_class_kernel sorts the blocks into untouched (switched off: block_len = 0 in the
   context's copy of the headers), direct (wholly inside the one range that touches it: decoded straight into that
   range's slot) and staged (an edge that is cut, a block several ranges share: decoded once, whole, into the context's
   scratch area).  With HUFGPU_RANGES_TILES a block that would be staged may instead be served tile by tile
   (DRANGE_TILES: range_tiles.hpp; drange_mark_kernel counts the (range, tile) pairs that decide it) - the decoders
   below do not see it.  drange_place_kernel turns that into the output offsets the indexed decoders read, which then run
   unchanged.  drange_result_kernel reduces the block states to one result per range and drange_gather_kernel copies
   the clipped pieces of the staged blocks into the slots. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "pack.hpp"

namespace hufgpu {

#define DRANGE_UNTOUCHED 0u
#define DRANGE_DIRECT    1u
#define DRANGE_STAGED    2u
#define DRANGE_TILES     3u         /* switched off for the decoders like an untouched block: drange_tiles_kernel serves it */
#define DRANGE_FLAG_MEMORY 1u       /* the slot is shorter than the range: nothing of it is decoded */
#define DRANGE_FLAG_HEADER 2u       /* the range reaches the first block whose header does not parse */
#define DRANGE_PIECE_CHUNKS 1024u   /* a gather workgroup's piece: 1 024 accesses of 16 bytes */

struct DecRangeArgs {
    const uint64_t *range_lo, *range_hi;    /* [nranges] as the caller gave them */
    const uint64_t *out_offsets;            /* [nranges + 1] range i's slot: [out_offsets[i], out_offsets[i + 1]) */
    uint64_t nranges, nblocks;
    HufDecodeMeta *dmeta;                   /* decode_prepare_kernel's (the context's copy: untouched blocks get block_len = 0) */
    const int32_t *status;
    TwoLevel lens;                          /* decode_prepare_kernel's sums of the block lengths */
    const unsigned long long *first_bad;    /* the first block whose header does not parse (~0: none), read before the decoders run */
    uint64_t *bprefix;                      /* [nblocks + 1] out: P */
    uint64_t *obase;                        /* [nblocks] out: where each block's output starts, from `base` */
    unsigned long long *cover;              /* [nblocks] (ranges over the block << 32) + the sum of their numbers */
    uint64_t *rel;                          /* [nblocks] direct: the offset in d_out, staged: the place in the scratch area */
    uint32_t *kind;                         /* [nblocks] DRANGE_* */
    uint64_t *rplan;                        /* [4 nranges] the clipped range [lo, hi), its first and last block (first > last: none) */
    uint32_t *rflag;                        /* [nranges] DRANGE_FLAG_* */
    unsigned long long *counters;           /* [7] staged blocks, the longest of them, the first block whose header does not parse; direct
                                               blocks, tile-routed blocks, their (range, tile) pairs, tile-routed blocks that failed a check */
    unsigned long long *range_fail;         /* [nranges] the first failing touched block (~0: none) */
    uint64_t *range_res;                    /* [3 nranges] out: error, bytes delivered, failing block (~0: none) */
    /* known once the scratch area is: */
    uint64_t dout_off, scratch_off, stride; /* d_out and the scratch area from the decoders' base; bytes per staged block */
    const uint8_t *scratch;
    uint8_t *dout;
    /* the tile route (NULL: none - no flag, no sub-index, or hufgpu_update_ranges' plan) */
    unsigned long long *tpairs;             /* [nblocks] (range, tile) pairs over the block; bit 63: it failed a tile check */
    uint64_t raw_size, blocksize;           /* the layout the sub-index rows are addressed by */
};

__device__ __forceinline__ uint64_t drange_pos(const DecRangeArgs &a, uint64_t b)
{
    return b >= a.nblocks ? *a.lens.total : a.lens.gprefix[b / SCAN_GROUP] + a.lens.local[b];
}

/* One thread per block: P, an empty cover.  One thread per range: the range cut at the end of the data (or at the first
 * header that does not parse: behind it positions are not known), the slot check, and the blocks that hold its first
 * and its last byte - binary searches in P, which repeats where a block is empty. */
__global__ __launch_bounds__(256) void drange_plan_kernel(DecRangeArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        a.counters[0] = 0; a.counters[1] = 0; a.counters[2] = *a.first_bad;
        a.counters[3] = 0; a.counters[4] = 0; a.counters[5] = 0; a.counters[6] = 0;
    }
    if (t <= a.nblocks) a.bprefix[t] = drange_pos(a, t);
    if (t < a.nblocks) {
        a.cover[t] = 0;
        if (a.tpairs) a.tpairs[t] = 0;
    }
    if (t >= a.nranges) return;
    const uint64_t kb = *a.first_bad;
    const bool bad = kb < a.nblocks;
    const uint64_t end = bad ? drange_pos(a, kb) : *a.lens.total;
    const uint64_t lo0 = a.range_lo[t], hi0 = a.range_hi[t];
    const uint64_t hi = dmin<uint64_t>(hi0, end), lo = dmin<uint64_t>(lo0, hi);
    const uint64_t need = hi - lo, slot = a.out_offsets[t + 1] - a.out_offsets[t];
    uint32_t flag = 0;
    if (slot < need) flag = DRANGE_FLAG_MEMORY;
    else if (bad && hi0 > end) flag = DRANGE_FLAG_HEADER;
    uint64_t fb = 1, lb = 0;
    if (need != 0 && flag != DRANGE_FLAG_MEMORY) {
        uint64_t x = 0, y = a.nblocks + 1;              /* the last b with P[b] <= lo (lo < P[nblocks]) */
        while (y - x > 1) {
            const uint64_t mid = (x + y) >> 1;
            if (drange_pos(a, mid) <= lo) x = mid;
            else y = mid;
        }
        fb = x;
        x = 0, y = a.nblocks + 1;                       /* the last b with P[b] < hi (0 < hi <= P[nblocks]) */
        while (y - x > 1) {
            const uint64_t mid = (x + y) >> 1;
            if (drange_pos(a, mid) < hi) x = mid;
            else y = mid;
        }
        lb = x;
    }
    a.rplan[4 * t] = lo;
    a.rplan[4 * t + 1] = hi;
    a.rplan[4 * t + 2] = fb;
    a.rplan[4 * t + 3] = lb;
    a.rflag[t] = flag;
}

/* grid (nranges, y): range blockIdx.x adds itself to the cover of each of its blocks - and, for the tile route, the
 * sub-index tiles of the block that hold bytes of it to the block's pairs */
__global__ __launch_bounds__(256) void drange_mark_kernel(DecRangeArgs a)
{
    asm volatile("; one VGPR more than the kernel uses (the build's ISA check: a 64-bit shift by the last of sixteen)" ::: "v16");
    const uint64_t i = blockIdx.x;
    const uint64_t fb = a.rplan[4 * i + 2], lb = a.rplan[4 * i + 3];
    if (fb > lb) return;
    const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1];
    for (uint64_t b = fb + (uint64_t)blockIdx.y * 256 + threadIdx.x; b <= lb; b += (uint64_t)gridDim.y * 256) {
        atomicAdd(&a.cover[b], (1ull << 32) + i);
        if (a.tpairs) {
            const uint64_t p0 = a.bprefix[b], p1 = a.bprefix[b + 1];
            const uint64_t c0 = dmax<uint64_t>(lo, p0), c1 = dmin<uint64_t>(hi, p1);
            if (c0 < c1) atomicAdd(&a.tpairs[b], (unsigned long long)((c1 - 1 - p0) / HUF_SUB_TILE - (c0 - p0) / HUF_SUB_TILE + 1));
        }
    }
}

/* One thread per block: untouched, direct, staged - or, for the tile route, served by tiles: a block that would be
 * staged, whose header length is the layout's (the sub-index rows are addressed by it), whose tree has more than one
 * leaf (the encoder writes no rows for one-symbol blocks) and over which the ranges make no more (range, tile) pairs
 * than it has tiles - the tile route then decodes no more symbols than the block has. */
__global__ __launch_bounds__(256) void drange_class_kernel(DecRangeArgs a)
{
    asm volatile("; one VGPR more than the kernel uses (the build's ISA check: a 64-bit shift by the last of sixteen)" ::: "v16");
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.nblocks) return;
    const unsigned long long v = a.cover[b];
    const uint32_t cnt = (uint32_t)(v >> 32);
    const HufDecodeMeta m = a.dmeta[b];
    uint32_t kind = DRANGE_STAGED;
    uint64_t rel = 0;
    if (cnt == 0 || m.block_len == 0 || m.status != HUFE_OK) {
        kind = DRANGE_UNTOUCHED;
        if (m.block_len != 0) a.dmeta[b].block_len = 0;
    } else if (cnt == 1) {
        const uint64_t i = (uint32_t)v;                 /* one range over the block: the sum of the numbers is its number */
        const uint64_t p = a.bprefix[b];
        const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1];
        if (lo <= p && p + m.block_len <= hi) {
            kind = DRANGE_DIRECT;
            rel = a.out_offsets[i] + (p - lo);
        }
    }
    if (kind == DRANGE_STAGED && a.tpairs) {
        const uint64_t pairs = a.tpairs[b];
        const uint64_t ntiles = (m.block_len + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
        if (b * a.blocksize < a.raw_size && m.block_len == dmin<uint64_t>(a.blocksize, a.raw_size - b * a.blocksize) &&
            m.leaf < 0 && pairs <= ntiles) {
            kind = DRANGE_TILES;
            a.dmeta[b].block_len = 0;
            atomicAdd(&a.counters[4], 1ull);
            atomicAdd(&a.counters[5], (unsigned long long)pairs);
        }
    }
    if (kind == DRANGE_STAGED) {
        rel = atomicAdd(&a.counters[0], 1ull);
        atomicMax(&a.counters[1], (unsigned long long)m.block_len);
    }
    {   /* (one addition a wave: a long range is thousands of direct blocks) */
        const unsigned long long dm = __ballot(kind == DRANGE_DIRECT);
        if (dm != 0ull && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(dm)) atomicAdd(&a.counters[3], (unsigned long long)__builtin_popcountll(dm));
    }
    a.kind[b] = kind;
    a.rel[b] = rel;
}

/* One thread per block, once the scratch area is there: the offset the indexed decoders add to their output base. */
__global__ __launch_bounds__(256) void drange_place_kernel(DecRangeArgs a)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint32_t kind = a.kind[b];
    uint64_t o = 0;
    if (kind == DRANGE_DIRECT) o = a.dout_off + a.rel[b];
    else if (kind == DRANGE_STAGED) o = a.scratch_off + a.rel[b] * a.stride;
    a.obase[b] = o;
}

/* After the decoders, one workgroup per range: the first failing block among its blocks, in stream order, its error and
 * the range's bytes in front of it - hufgpu_decode_batch's reduction, keyed by range (a block that several ranges
 * share fails each of them). */
__global__ __launch_bounds__(256) void drange_result_kernel(DecRangeArgs a)
{
    __shared__ unsigned long long s_fail;
    const uint64_t i = blockIdx.x;
    const uint32_t flag = a.rflag[i];
    const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1], fb = a.rplan[4 * i + 2], lb = a.rplan[4 * i + 3];
    if (threadIdx.x == 0) s_fail = ~0ull;
    __syncthreads();
    unsigned long long mine = ~0ull;
    if (fb <= lb) {
        /* (no early way out: the loads of a long range must not wait for one another) */
#pragma unroll 8
        for (uint64_t b = fb + threadIdx.x; b <= lb; b += 256)
            if (a.status[b] != HUFE_OK) mine = dmin<unsigned long long>(mine, b);
    }
    if (mine != ~0ull) atomicMin(&s_fail, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long f = s_fail;
    uint64_t err = HUFE_OK, raw = hi - lo;
    if (flag == DRANGE_FLAG_MEMORY) {
        err = HUFE_MEMORY;
        raw = 0;
    } else if (f != ~0ull) {
        err = (uint64_t)(uint32_t)a.status[f];
        raw = dmax<uint64_t>(a.bprefix[f], lo) - lo;
    } else if (flag == DRANGE_FLAG_HEADER) {
        err = (uint64_t)(uint32_t)a.status[a.counters[2]];
    }
    a.range_fail[i] = f;
    a.range_res[3 * i] = err;
    a.range_res[3 * i + 1] = raw;
    a.range_res[3 * i + 2] = f;
}

/* n bytes from src to dst, both at any byte alignment, piece `piece` of `npieces`: the body in 16-byte accesses that
 * are aligned on the store side (loads need no alignment on gfx950), four in flight per lane; the bytes in front of the
 * first aligned store go with piece 0, those behind the last one with the last piece. */
__device__ __forceinline__ void drange_copy_piece(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n,
                                                  uint64_t piece, uint64_t npieces)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    typedef v4u __attribute__((aligned(1))) v4u_unaligned;
    const uint32_t tid = threadIdx.x;
    const uint64_t head = dmin<uint64_t>(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint64_t chunks = (n - head) >> 4;
    const uint64_t tail = (n - head) & 15u;
    if (piece == 0 && tid < head) dst[tid] = src[tid];
    if (piece == npieces - 1 && tid < tail) dst[head + 16 * chunks + tid] = src[head + 16 * chunks + tid];
    const uint64_t c0 = piece * DRANGE_PIECE_CHUNKS;
    const uint64_t c1 = dmin<uint64_t>(chunks, c0 + DRANGE_PIECE_CHUNKS);
    v4u *d = reinterpret_cast<v4u *>(dst + head);
    const v4u_unaligned *s = reinterpret_cast<const v4u_unaligned *>(src + head);
    for (uint64_t c = c0 + tid; c < c1; c += 4 * 256) {
        v4u v[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c + 256u * k < c1) v[k] = s[c + 256u * k];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c + 256u * k < c1) d[c + 256u * k] = v[k];
    }
}

/* grid (nranges, y): for every staged block of range blockIdx.x in front of the range's first failing block, the part
 * of it inside the range goes from the scratch area to the slot.  A copy is cut into pieces of 16 KiB that the y
 * workgroups of the range take in turn, so one long edge is not one workgroup's work. */
__global__ __launch_bounds__(256) void drange_gather_kernel(DecRangeArgs a)
{
    __shared__ uint32_t s_list[256];
    __shared__ uint32_t s_n;
    const uint64_t i = blockIdx.x;
    if (a.rflag[i] == DRANGE_FLAG_MEMORY) return;
    const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1], fb = a.rplan[4 * i + 2], lb = a.rplan[4 * i + 3];
    if (fb > lb) return;
    const unsigned long long f = a.range_fail[i];
    uint8_t *slot = a.dout + a.out_offsets[i];
    for (uint64_t b0 = fb; b0 <= lb; b0 += 256) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const uint64_t mine = b0 + threadIdx.x;
        if (mine <= lb && mine < f && a.kind[mine] == DRANGE_STAGED) s_list[atomicAdd(&s_n, 1u)] = threadIdx.x;
        __syncthreads();
        const uint32_t n = s_n;
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t b = b0 + s_list[j];
            const uint64_t p0 = a.bprefix[b], p1 = p0 + a.dmeta[b].block_len;
            const uint64_t c0 = dmax<uint64_t>(lo, p0), c1 = dmin<uint64_t>(hi, p1);
            if (c0 >= c1) continue;
            const uint8_t *src = a.scratch + a.rel[b] * a.stride + (c0 - p0);
            uint8_t *dst = slot + (c0 - lo);
            const uint64_t len = c1 - c0;
            const uint64_t head = dmin<uint64_t>(len, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
            const uint64_t chunks = (len - head) >> 4;
            const uint64_t npieces = chunks == 0 ? 1 : (chunks + DRANGE_PIECE_CHUNKS - 1) / DRANGE_PIECE_CHUNKS;
            for (uint64_t p = 0; p < npieces; p++)                  /* (the list's order differs from workgroup to workgroup: the turn goes by block) */
                if ((b - fb + p) % gridDim.y == blockIdx.y) drange_copy_piece(dst, src, len, p, npieces);
        }
        __syncthreads();
    }
}

}  // namespace hufgpu

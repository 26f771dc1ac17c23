/* update.hpp - the kernels of hufgpu_update_ranges (include/huffman_gpu.h): byte ranges of the original data
   overwritten in one indexed stream, out of place.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   An overwrite changes no length, so every block keeps its block_len and only the blocks a range touches get a new
   record.  decode_prepare_kernel, drange_plan_kernel and drange_mark_kernel (ranges.hpp) run as they are: P, every
   range's first and last block, the ranges over every block.  upd_class_kernel sorts the blocks into
     copy    untouched: the record moves to its new place byte for byte (update_copy_kernel),
     void    untouched, and its index entry names no bytes of the stream: it gets no bytes in the new stream either,
     direct  wholly inside the one range that touches it: encoded straight from the caller's new bytes, the old record
             is not looked at beyond its header (the decoders are switched off for it: block_len = 0 in the context's
             copy of the headers, as for every untouched block),
     staged  an edge that is cut, a block several ranges share: decoded once, whole, into the context's scratch area
             by the indexed decoders, overwritten there by upd_overlay_kernel, encoded from there,
   and numbers the touched blocks: a compact list of rows (block, source, length).  The sources are 64-bit offsets from
   one base - the lower of the caller's new bytes and the scratch area.  hist_lanes_pairs_kernel / hist_tree_pairs_kernel
   count and build the trees of the rows (the bodies of hist_lanes_kernel / hist_tree_kernel; tree_wave_kernel runs on
   the rows unchanged), upd_index_kernel writes the new block index - a touched block's encoded size, any other block's
   old size - and pack_pairs_kernel packs every row into its block's new place (the body of pack_kernel).

   update_copy_kernel moves everything else.  Between two touched blocks all records move by one byte shift, which is
   in general no multiple of 16.  The destination is cut into pieces of 16 KiB at 16-byte aligned addresses, one
   workgroup each, so neither one long run nor a million tiny blocks is one workgroup's work; upd_piece_kernel finds
   every piece's first block by binary search in the new index.  A workgroup walks the blocks of its piece 256 at a
   time, and every maximal run of copy blocks inside the piece moves as one segment: 16-byte stores aligned on the
   destination, 16-byte non-temporal loads at any byte of the source, four in flight per lane, single bytes in front
   of the first and behind the last aligned store.  A segment is a whole number of untouched records cut at the
   piece's (aligned) borders, so a workgroup never writes a byte of a touched record or of another piece: copy and
   pack may run in either order or side by side (pack byte-masks its first and last word, pack.hpp). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "hist_lanes.hpp"
#include "hist_tree.hpp"
#include "pack.hpp"
#include "ranges.hpp"

namespace hufgpu {

#define UPD_COPY   0u
#define UPD_DIRECT 1u
#define UPD_STAGED 2u
#define UPD_VOID   3u
#define UPD_PIECE  16384u           /* a copy workgroup's piece of the destination: four 16-byte accesses a lane */

/* ucount[]: what the kernels hand to the host */
#define UPD_N_TOUCHED 0             /* touched blocks = rows */
#define UPD_LONGEST   1             /* the longest touched block */
#define UPD_RANGE_ERR 2             /* ~((range << 8) | error) of the first range that cannot be served (0: none) */
#define UPD_FAILED    3             /* ~(the first staged block that did not decode) (0: none) */
#define UPD_TOTAL     4             /* the length of the new stream */
#define UPD_WORDS     8

struct UpdateArgs {
    DecRangeArgs r;                         /* the plan of ranges.hpp; r.out_offsets: the exclusive sums of the range lengths */
    const uint64_t *src_offsets;            /* [nranges] range i's new bytes start at d_src + src_offsets[i] */
    const uint64_t *old_offsets;            /* [nblocks + 1] the old block index */
    uint64_t *new_offsets;                  /* [nblocks + 1] out */
    uint64_t stream_len;
    uint32_t *row_of;                       /* [nblocks] a touched block's row */
    uint32_t *row_blk;                      /* [rows] the block of a row */
    uint64_t *pairs;                        /* [2 rows] (source offset from the common base, length) */
    const HufBlockMeta *meta;               /* [rows] tree_wave_kernel's */
    unsigned long long *ucount;             /* [UPD_WORDS] */
    /* known once the scratch area is: */
    uint64_t src_off, scratch_off;          /* d_src and the scratch area from the common base */
    const uint8_t *src;
    uint8_t *scratch_w;
};

/* One thread per block: its kind, and for a touched block its row.  One thread per range: a range that reaches past
 * the end of the data cannot be written (HUF_ERROR_INVALID_ARGUMENT), one that reaches the first header that does not
 * parse fails with that header's error - drange_plan_kernel has cut both at that point. */
__global__ __launch_bounds__(256) void upd_class_kernel(UpdateArgs u)
{
    const DecRangeArgs &a = u.r;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.nranges) {
        const uint64_t lo0 = a.range_lo[t], hi0 = a.range_hi[t];
        if (lo0 < hi0 && a.rplan[4 * t + 1] != hi0) {
            const uint64_t kb = a.counters[2];
            const uint64_t err = kb < a.nblocks ? (uint64_t)(uint32_t)a.status[kb] : (uint64_t)HUFE_ARGUMENT;
            atomicMax(&u.ucount[UPD_RANGE_ERR], ~(unsigned long long)((t << 8) | (err & 0xffu)));
        }
    }
    const uint64_t b = t;
    if (b >= a.nblocks) return;
    const unsigned long long v = a.cover[b];
    const uint32_t cnt = (uint32_t)(v >> 32);
    const HufDecodeMeta m = a.dmeta[b];
    uint32_t kind;
    if (cnt == 0 || m.block_len == 0 || m.status != HUFE_OK) {
        const uint64_t o0 = u.old_offsets[b], o1 = u.old_offsets[b + 1];
        kind = (o0 <= o1 && o1 <= u.stream_len) ? UPD_COPY : UPD_VOID;
        if (m.block_len != 0) a.dmeta[b].block_len = 0;
    } else {
        const uint32_t row = (uint32_t)atomicAdd(&u.ucount[UPD_N_TOUCHED], 1ull);
        atomicMax(&u.ucount[UPD_LONGEST], (unsigned long long)m.block_len);
        u.row_of[b] = row;
        u.row_blk[row] = (uint32_t)b;
        u.pairs[2 * (uint64_t)row + 1] = m.block_len;
        kind = UPD_STAGED;
        const uint64_t p = a.bprefix[b];
        if (cnt == 1) {
            const uint64_t i = (uint32_t)v;                 /* one range over the block: the sum of the numbers is its number */
            const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1];
            if (lo <= p && p + m.block_len <= hi) {
                kind = UPD_DIRECT;
                u.pairs[2 * (uint64_t)row] = u.src_offsets[i] + (p - lo);
                a.dmeta[b].block_len = 0;                   /* nothing of the old record is decoded */
            }
        }
        if (kind == UPD_STAGED) {
            const uint64_t entry = atomicAdd(&a.counters[0], 1ull);
            atomicMax(&a.counters[1], (unsigned long long)m.block_len);
            a.rel[b] = entry;
        }
    }
    a.kind[b] = kind;
}

/* One thread per block, once the scratch area is there: where the decoders write a staged block (they count from the
 * scratch area), and every row's source from the common base. */
__global__ __launch_bounds__(256) void upd_place_kernel(UpdateArgs u)
{
    const DecRangeArgs &a = u.r;
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint32_t kind = a.kind[b];
    uint64_t o = 0;
    if (kind == UPD_STAGED) {
        o = a.rel[b] * a.stride;
        u.pairs[2 * (uint64_t)u.row_of[b]] = u.scratch_off + o;
    } else if (kind == UPD_DIRECT) {
        u.pairs[2 * (uint64_t)u.row_of[b]] += u.src_off;
    }
    a.obase[b] = o;
}

/* grid (nranges, y), after the decoders: the mirror of drange_gather_kernel.  For every staged block of range
 * blockIdx.x the part of the range inside the block goes from the caller's new bytes over the block's scratch entry;
 * head, body and tail of a piece lie inside that part, so nothing outside the entry is written. */
__global__ __launch_bounds__(256) void upd_overlay_kernel(UpdateArgs u)
{
    __shared__ uint32_t s_list[256];
    __shared__ uint32_t s_n;
    const DecRangeArgs &a = u.r;
    const uint64_t i = blockIdx.x;
    const uint64_t lo = a.rplan[4 * i], hi = a.rplan[4 * i + 1], fb = a.rplan[4 * i + 2], lb = a.rplan[4 * i + 3];
    if (fb > lb) return;
    const uint8_t *from = u.src + u.src_offsets[i];
    for (uint64_t b0 = fb; b0 <= lb; b0 += 256) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        const uint64_t mine = b0 + threadIdx.x;
        if (mine <= lb && a.kind[mine] == UPD_STAGED) s_list[atomicAdd(&s_n, 1u)] = threadIdx.x;
        __syncthreads();
        const uint32_t n = s_n;
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t b = b0 + s_list[j];
            const uint64_t p0 = a.bprefix[b], p1 = p0 + a.dmeta[b].block_len;
            const uint64_t c0 = dmax<uint64_t>(lo, p0), c1 = dmin<uint64_t>(hi, p1);
            if (c0 >= c1) continue;
            uint8_t *dst = u.scratch_w + a.rel[b] * a.stride + (c0 - p0);
            const uint8_t *src = from + (c0 - lo);
            const uint64_t len = c1 - c0;
            const uint64_t head = dmin<uint64_t>(len, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
            const uint64_t chunks = (len - head) >> 4;
            const uint64_t npieces = chunks == 0 ? 1 : (chunks + DRANGE_PIECE_CHUNKS - 1) / DRANGE_PIECE_CHUNKS;
            for (uint64_t p = 0; p < npieces; p++)
                if ((b - fb + p) % gridDim.y == blockIdx.y) drange_copy_piece(dst, src, len, p, npieces);
        }
        __syncthreads();
    }
}

/* One thread per block, after the decoders: the first staged block that did not decode, in stream order. */
__global__ __launch_bounds__(256) void upd_fail_kernel(UpdateArgs u)
{
    const DecRangeArgs &a = u.r;
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b < a.nblocks && a.kind[b] == UPD_STAGED && a.status[b] != HUFE_OK) atomicMax(&u.ucount[UPD_FAILED], ~(unsigned long long)b);
}

/* ---- counts and trees of the rows: the batch's twins reading (source, length) pairs ---- */

template <int THREADS>
__global__ __launch_bounds__(THREADS, HL_WAVES_PER_SIMD) void hist_lanes_pairs_kernel(const uint8_t *__restrict__ base,
                                                                                      const uint64_t *__restrict__ pairs,
                                                                                      uint32_t *__restrict__ hist)
{
    __shared__ __attribute__((aligned(16))) uint8_t hl_lds[HL_LDS_BYTES];
    const uint64_t row = blockIdx.x;
    hl_count<THREADS>(hl_lds, base + pairs[2 * row], pairs[2 * row + 1], hist + row * HUF_NSYM);
}

template <int THREADS, bool PACKED>
__global__ __launch_bounds__(THREADS) void hist_tree_pairs_kernel(const uint8_t *__restrict__ base, const uint64_t *__restrict__ pairs,
                                                                  hufcode_t *__restrict__ codetab, int16_t *__restrict__ treebuf,
                                                                  HufBlockMeta *__restrict__ meta, TwoLevel sizes)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_union[HistTreeLds<THREADS, PACKED>::UBYTES];
    __shared__ uint32_t s_side[2 * THREADS];
    const uint64_t row = blockIdx.x;
    hist_tree_block<THREADS, PACKED>(base + pairs[2 * row], pairs[2 * row + 1], row, codetab, treebuf, meta, sizes, s_union, s_side);
}

/* The new block index, by one workgroup (scan_sizes_kernel's sweep): a touched block has the size its tree and its
 * counts give it, a copy block its old size, a void block none. */
template <int THREADS>
__global__ __launch_bounds__(THREADS) void upd_index_kernel(UpdateArgs u)
{
    const uint64_t nb = u.r.nblocks;
    const uint64_t total = chunked_excl_scan<THREADS>(nb, u.new_offsets, [&u](uint64_t b) -> uint64_t {
        const uint32_t kind = u.r.kind[b];
        if (kind == UPD_COPY) return u.old_offsets[b + 1] - u.old_offsets[b];
        if (kind == UPD_VOID) return 0ull;
        return encoded_block_bytes(u.meta[u.row_of[b]]);
    });
    if (threadIdx.x == 0) {
        u.new_offsets[nb] = total;
        u.ucount[UPD_TOTAL] = total;
    }
}

/* One workgroup per row: pack_kernel's body for the row's block, into the place the new index gives it.  A stream
 * that does not fit the output is not written at all. */
template <int THREADS, bool SHORT>
__global__ __launch_bounds__(THREADS, SHORT ? PACK_WAVES_PER_SIMD : 4) void pack_pairs_kernel(const uint8_t *__restrict__ base,
                                                                                            const uint64_t *__restrict__ pairs,
                                                                                            const uint32_t *__restrict__ row_blk,
                                                                                            const hufcode_t *__restrict__ codetab,
                                                                                            const int16_t *__restrict__ treebuf,
                                                                                            const HufBlockMeta *__restrict__ meta,
                                                                                            uint64_t *__restrict__ offsets, uint64_t nblocks,
                                                                                            uint64_t out_cap,
                                                                                            uint8_t *__restrict__ out, HufSubIndex sub)
{
    __shared__ hufcode_t s_code[HUF_NSYM];
    __shared__ uint32_t s_part[THREADS / 64];
    __shared__ uint32_t s_tail[THREADS / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[PACK_STAGE_WORDS];
#ifdef PACK_VGPR_SLACK      /* test builds only: as pack_kernel */
    asm volatile("; one VGPR more than the kernel uses" ::: PACK_VGPR_SLACK);
#endif
    if (offsets[nblocks] > out_cap) return;
    const uint64_t row = blockIdx.x;
    TwoLevel sizes = {};                 /* local = NULL: the place comes from the finished index */
    pack_block_any<THREADS, SHORT>(base + pairs[2 * row], pairs[2 * row + 1], row, row_blk[row], codetab, treebuf, meta, offsets,
                                   sizes, out, sub, s_code, s_part, s_tail, s_stage);
}

/* ---- the untouched records ---- */

struct UpdCopyArgs {
    const uint8_t *stream;
    uint8_t *out;
    const uint64_t *old_offsets, *new_offsets;      /* [nblocks + 1] */
    const uint32_t *kind;                           /* [nblocks] */
    uint32_t *piece_first;                          /* [npieces] the last block that starts at or in front of the piece */
    uint64_t nblocks, npieces, out_cap;
    uint64_t align;                                 /* d_out & 15: pieces are cut at aligned ADDRESSES */
};

__device__ __forceinline__ uint64_t upd_piece_lo(const UpdCopyArgs &a, uint64_t p)
{
    return p ? p * UPD_PIECE - a.align : 0;
}

__global__ __launch_bounds__(256) void upd_piece_kernel(UpdCopyArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npieces) return;
    const uint64_t lo = upd_piece_lo(a, p);
    uint64_t x = 0, y = a.nblocks;                      /* the last b with new[b] <= lo (new[0] = 0) */
    while (y - x > 1) {
        const uint64_t mid = (x + y) >> 1;
        if (a.new_offsets[mid] <= lo) x = mid;
        else y = mid;
    }
    a.piece_first[p] = (uint32_t)x;
}

/* n bytes from src (any alignment) to dst (any alignment) by the whole workgroup */
__device__ __forceinline__ void upd_copy_segment(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    typedef uint32_t v4u_any __attribute__((ext_vector_type(4), aligned(1)));
    const uint32_t tid = threadIdx.x;
    const uint64_t head = dmin<uint64_t>(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint64_t chunks = (n - head) >> 4;
    const uint64_t tail = (n - head) & 15u;
    if (tid < head) dst[tid] = src[tid];
    if (tid < tail) dst[head + 16 * chunks + tid] = src[head + 16 * chunks + tid];
    v4u *d = reinterpret_cast<v4u *>(dst + head);
    const v4u_any *s = reinterpret_cast<const v4u_any *>(src + head);
    for (uint64_t c = tid; c < chunks; c += 4 * 256) {
        v4u v[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c + 256u * k < chunks) v[k] = __builtin_nontemporal_load(s + c + 256u * k);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c + 256u * k < chunks) d[c + 256u * k] = v[k];
    }
}

/* One workgroup per piece of the destination. */
__global__ __launch_bounds__(256) void update_copy_kernel(UpdCopyArgs a)
{
    __shared__ uint64_t s_new[257], s_old[256];
    __shared__ unsigned long long s_copy[4], s_in[4];
    const uint64_t total = a.new_offsets[a.nblocks];
    if (total > a.out_cap) return;
    const uint64_t p = blockIdx.x;
    const uint64_t lo = upd_piece_lo(a, p), hi = dmin<uint64_t>(upd_piece_lo(a, p + 1), total);
    if (lo >= hi) return;
    const uint32_t tid = threadIdx.x;
    for (uint64_t b0 = a.piece_first[p];; b0 += 256) {
        const uint64_t b = b0 + tid;
        uint64_t nw = ~0ull, od = 0;
        uint32_t kind = UPD_VOID;
        if (b < a.nblocks) {
            nw = a.new_offsets[b];
            od = a.old_offsets[b];
            kind = a.kind[b];
        } else if (b == a.nblocks) {
            nw = total;
        }
        s_new[tid] = nw;
        s_old[tid] = od;
        if (tid == 255) s_new[256] = b + 1 <= a.nblocks ? a.new_offsets[b + 1] : ~0ull;
        const bool in = b < a.nblocks && nw < hi;
        const unsigned long long m_in = __ballot(in), m_copy = __ballot(in && kind == UPD_COPY);
        if ((tid & 63u) == 0) {
            s_in[tid >> 6] = m_in;
            s_copy[tid >> 6] = m_copy;
        }
        __syncthreads();
        uint32_t nin = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            nin += (uint32_t)__popcll(s_in[w]);
            unsigned long long m = s_copy[w];
            while (m) {                                   /* the runs of copy blocks among these 64, first to last */
                const uint32_t j = (uint32_t)__builtin_ctzll(m);
                const unsigned long long rest = ~(m >> j);
                const uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
                m = run >= 64u ? 0ull : (m & ~(((1ull << run) - 1ull) << j));
                const uint32_t first = 64u * w + j, end = first + run;
                const uint64_t n0 = s_new[first];
                const uint64_t d0 = dmax<uint64_t>(n0, lo), d1 = dmin<uint64_t>(s_new[end], hi);
                if (d0 < d1) upd_copy_segment(a.out + d0, a.stream + s_old[first] + (d0 - n0), d1 - d0);
            }
        }
        __syncthreads();
        if (nin < 256u) break;
    }
}

/* One thread per block, for a call without ranges: P and every block a copy block (what upd_sub_rows_kernel reads). */
__global__ __launch_bounds__(256) void upd_positions_kernel(TwoLevel lens, uint64_t nblocks, uint64_t *__restrict__ bprefix,
                                                            uint32_t *__restrict__ kind)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b > nblocks) return;
    bprefix[b] = b == nblocks ? *lens.total : lens.gprefix[b / SCAN_GROUP] + lens.local[b];
    if (b < nblocks) kind[b] = UPD_COPY;
}

/* The sub-index rows of the blocks that keep their record, old buffer to new buffer, same layout: one workgroup per
 * block, and of a row only the entries the encoder writes (no row of a one-symbol block, no padding, nothing behind a
 * short block's last tile and group). */
__global__ __launch_bounds__(256) void upd_sub_rows_kernel(HufSubIndex from, HufSubIndex to, const uint32_t *__restrict__ kind,
                                                           const HufDecodeMeta *__restrict__ dmeta,
                                                           const uint64_t *__restrict__ bprefix, uint64_t row_syms)
{
    const uint64_t b = blockIdx.x;
    const uint32_t k = kind[b];
    if (k == UPD_DIRECT || k == UPD_STAGED) return;
    const HufDecodeMeta m = dmeta[b];
    const uint64_t len = bprefix[b + 1] - bprefix[b];
    if (m.status != HUFE_OK || m.tree_len == 5 || len == 0 || len > row_syms) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t nt = (len + HUF_SUB_TILE - 1) / HUF_SUB_TILE, ng = (len + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP;
    for (uint64_t t = tid; t < nt; t += 256) to.tile_bits[b * to.tpb + t] = from.tile_bits[b * from.tpb + t];
    const uint64_t *g_from = reinterpret_cast<const uint64_t *>(from.group_bits + b * from.gpb);    /* rows of 16-byte multiples */
    uint64_t *g_to = reinterpret_cast<uint64_t *>(to.group_bits + b * to.gpb);
    for (uint64_t w = tid; w < ng / 4; w += 256) g_to[w] = g_from[w];
    if (tid < (ng & 3u)) to.group_bits[b * to.gpb + (ng & ~3ull) + tid] = from.group_bits[b * from.gpb + (ng & ~3ull) + tid];
    if (tid < HUF_NSYM / 8)
        reinterpret_cast<uint64_t *>(to.lens + b * HUF_NSYM)[tid] = reinterpret_cast<const uint64_t *>(from.lens + b * HUF_NSYM)[tid];
}

}  // namespace hufgpu

/* select.hpp - hufgpu_select_spans: grep -o's non-overlapping leftmost-longest matches, chosen from the spans that
   hufgpu_find_any_spans reports (include/huffman_gpu.h).
   Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   The selection is a chain: rank 0 is taken, and behind a taken rank s the next one is succ(s), the least r > s with
   pos[r] >= pos[s] + len[s].  Positions rise by at least 1 a rank and no length is above 64, so succ(i) lies in
   (i, i + 64]: a chain ENTERS a tile of SEL_TILE ranks at one of its first 64 ranks, and what a tile does to a chain is a
   map of 64 entry offsets to 64 exit offsets - the offset of the first taken rank in the NEXT tile.  Maps compose.

     select_tile_kernel     a workgroup a tile: positions of the tile and of the 64 ranks behind it to LDS, order and lengths
                            checked (the lowest offending rank by atomic minimum), succ() of every rank by a binary search over
                            its window of 64, then pointer jumping in LDS until every rank points out of the tile: the map.
     select_compose_kernel  a wave a group of SEL_FAN maps of one level, a lane an entry offset: the maps in front of member j
                            composed - the PREFIX map of j - take j's place, the whole group's map goes one level up.  One
                            ds_bpermute a member.  Launched once a level; the top level has one group.
     select_mark_kernel     a workgroup a tile: its true entry offset is one look-up a level, top down, starting from offset 0
                            - rank 0 is taken -; succ() once more, and the walk from the entry by doubling: in round k the
                            ranks marked so far mark the rank 2^k steps on.  The marks go to memory as bits, their count into
                            the two-level ticket scan of kernels/offsets.hpp.
     select_emit_kernel     a workgroup a tile: rank in the output = the scan's prefix + the marks in front; the taken spans,
                            compacted, below sel_cap.
     select_finish_kernel   the four totals, and the pad rows.

   Nothing at or behind rank n = min(*d_n, n_cap) is read: those ranks count as positions beyond every end.  Whatever the
   input holds, every successor is clamped to its window and every map entry is below 64, so no index leaves its array; on
   invalid input the answer is the status, and nothing of the maps is used for output. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "util.hpp"
#include "offsets.hpp"

namespace hufgpu {

#define SEL_THREADS 256
#define SEL_PER 4u                          /* ranks a thread: rank k * SEL_THREADS + thread of the tile, k < SEL_PER */
#define SEL_TILE (SEL_THREADS * SEL_PER)    /* 1 024 ranks a tile */
#define SEL_WINDOW 64u                      /* = HUFGPU_FIND_PATTERN_MAX: succ(i) <= i + SEL_WINDOW */
#define SEL_FAN 64u                         /* maps a composition group */
#define SEL_ROUNDS 10                       /* 2^SEL_ROUNDS >= SEL_TILE: no chain has more steps in a tile */
#define SEL_LEVELS_MAX 4
#define SEL_MARK_WORDS (SEL_TILE / 64u)     /* 64-bit words of marks a tile: word k * 4 + wave, bit = lane */
#define SEL_NONE (~0ull)
static_assert(SEL_TILE == (1u << SEL_ROUNDS) && SEL_WINDOW == 64u && SEL_FAN == 64u, "a lane an entry offset, a lane a member");

struct SelectArgs {
    const uint64_t *pos;                    /* [n_cap] */
    const uint32_t *len;                    /* [n_cap] */
    const uint64_t *n_word;                 /* NULL: n = n_cap */
    uint64_t n_cap, ntiles;
    uint64_t *sel_pos;                      /* [sel_cap] */
    uint32_t *sel_len;                      /* [sel_cap] */
    uint64_t *sel_rank;                     /* [sel_cap], optional */
    uint64_t sel_cap, pad_pos;
    uint64_t *totals;                       /* [4] */
    uint32_t flags, levels;
    uint8_t *maps[SEL_LEVELS_MAX + 1];      /* level k: count[k] maps of 64 bytes; level 0 = the tiles */
    uint64_t count[SEL_LEVELS_MAX + 1];
    uint64_t *marks;                        /* [ntiles * SEL_MARK_WORDS] */
    unsigned long long *bad;                /* the lowest offending rank, SEL_NONE: none.  NULL with n_cap = 0 */
    TwoLevel scan;                          /* of the tiles' counts; scan.total: how many are selected */
};

__device__ __forceinline__ uint64_t select_n(const SelectArgs &a)
{
    return a.n_word ? dmin<uint64_t>(*a.n_word, a.n_cap) : a.n_cap;
}

/* The tile's positions to s_pos - [0] is the rank in front of the tile, [1 + i] rank i of the tile, up to the window behind
 * it; SEL_NONE for a rank that does not exist - and succ() of the thread's ranks, as indices into the tile (>= SEL_TILE: out
 * of it, by that much), to nxt[].  `worst` is the thread's lowest offending rank.  Ends with a barrier behind s_pos's last
 * read. */
__device__ __forceinline__ void select_successors(const SelectArgs &a, uint64_t tile, uint64_t n, uint64_t *s_pos, uint32_t nxt[SEL_PER],
                                                  uint64_t &worst)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = tile * SEL_TILE;
    uint32_t mylen[SEL_PER];
#pragma unroll
    for (uint32_t k = 0; k < SEL_PER; k++) {
        const uint64_t g = g0 + k * SEL_THREADS + tid;
        s_pos[1u + k * SEL_THREADS + tid] = g < n ? a.pos[g] : SEL_NONE;
        mylen[k] = g < n ? a.len[g] : 1u;
    }
    if (tid < SEL_WINDOW) {
        const uint64_t g = g0 + SEL_TILE + tid;
        s_pos[1u + SEL_TILE + tid] = g < n ? a.pos[g] : SEL_NONE;
    }
    if (tid == SEL_WINDOW) s_pos[0] = g0 > 0 ? a.pos[g0 - 1] : 0ull;       /* (g0 < n: the caller has seen to it) */
    __syncthreads();
    worst = SEL_NONE;
#pragma unroll
    for (uint32_t k = 0; k < SEL_PER; k++) {
        const uint32_t i = k * SEL_THREADS + tid;
        const uint64_t g = g0 + i, p = s_pos[1u + i];
        if (g >= n) {
            nxt[k] = i + 1u;
            continue;
        }
        const bool offends = mylen[k] - 1u >= SEL_WINDOW || (g > 0 && p <= s_pos[i]);
        if (offends) worst = dmin(worst, g);
        /* the least j in (i, i + 64] with pos[j] >= end: how many of i + 1 ... i + 63 lie in front of the end */
        const uint64_t end = p + mylen[k];
        uint32_t lo = i + 1u;
#pragma unroll
        for (uint32_t step = SEL_WINDOW / 2; step > 0; step >>= 1)
            if (s_pos[1u + lo + step - 1u] < end) lo += step;
        nxt[k] = lo;
    }
    __syncthreads();
}

/* ---- the tiles' maps ------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(SEL_THREADS) void select_tile_kernel(SelectArgs a)
{
    __shared__ uint64_t s_pos[1u + SEL_TILE + SEL_WINDOW];
    __shared__ uint16_t s_j[SEL_TILE];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x, n = select_n(a);
    uint8_t *map = a.maps[0] + tile * SEL_WINDOW;
    if (tile * SEL_TILE >= n) {             /* no chain comes here; the map stays a map */
        if (tid < SEL_WINDOW) map[tid] = (uint8_t)tid;
        return;
    }
    uint32_t nxt[SEL_PER];
    uint64_t worst;
    select_successors(a, tile, n, s_pos, nxt, worst);
    if (worst != SEL_NONE) atomicMin(a.bad, (unsigned long long)worst);
#pragma unroll
    for (uint32_t k = 0; k < SEL_PER; k++) s_j[k * SEL_THREADS + tid] = (uint16_t)nxt[k];
    __syncthreads();
    /* pointer jumping in place: whatever a read sees, the old pointer or the new one, lies further along the same chain,
     * so a round at least doubles the steps a pointer spans; a pointer out of the tile stays */
    for (int r = 0; r < SEL_ROUNDS; r++) {
#pragma unroll
        for (uint32_t k = 0; k < SEL_PER; k++) {
            const uint32_t j = nxt[k];
            if (j < SEL_TILE) nxt[k] = s_j[j];
        }
#pragma unroll
        for (uint32_t k = 0; k < SEL_PER; k++) s_j[k * SEL_THREADS + tid] = (uint16_t)nxt[k];
        __syncthreads();
    }
    if (tid < SEL_WINDOW) map[tid] = (uint8_t)((nxt[0] - SEL_TILE) & (SEL_WINDOW - 1u));      /* (k = 0: rank `tid` of the tile) */
}

/* ---- one level of composition ------------------------------------------------------------------------------------------
 * Level `k` has count[k] maps.  The wave's group is members g * SEL_FAN ... ; lane l holds entry offset l.  `cur` is the
 * composition of the members in front of j: it takes j's place in memory (all members are in registers by then), then
 * cur[l] = M_j[cur[l]], a ds_bpermute of the lanes' M_j.  What is left behind the last member is the group's map. */
__global__ __launch_bounds__(SEL_THREADS) void select_compose_kernel(SelectArgs a, uint32_t k)
{
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t g = (uint64_t)blockIdx.x * (SEL_THREADS / 64) + (threadIdx.x >> 6);
    const uint64_t first = g * SEL_FAN;
    if (first >= a.count[k]) return;
    const uint32_t members = (uint32_t)dmin<uint64_t>(SEL_FAN, a.count[k] - first);
    uint8_t *maps = a.maps[k] + first * SEL_WINDOW;
    uint32_t m[SEL_FAN];
#pragma unroll
    for (uint32_t j = 0; j < SEL_FAN; j++) m[j] = j < members ? (uint32_t)maps[j * SEL_WINDOW + lane] & (SEL_WINDOW - 1u) : lane;
    uint32_t cur = lane;
#pragma unroll
    for (uint32_t j = 0; j < SEL_FAN; j++) {
        if (j < members) maps[j * SEL_WINDOW + lane] = (uint8_t)cur;
        cur = (uint32_t)__shfl((int)m[j], (int)cur);
    }
    a.maps[k + 1][g * SEL_WINDOW + lane] = (uint8_t)cur;
}

/* ---- the walk from the true entry, the marks and their count ----------------------------------------------------------- */
__global__ __launch_bounds__(SEL_THREADS) void select_mark_kernel(SelectArgs a)
{
    __shared__ uint64_t s_pos[1u + SEL_TILE + SEL_WINDOW];
    __shared__ uint16_t s_j[SEL_TILE];
    __shared__ uint8_t s_mark[SEL_TILE];
    __shared__ uint32_t s_cnt[SEL_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = tid >> 6;
    const uint64_t tile = blockIdx.x, n = select_n(a);
    uint32_t count = 0;
    if (tile * SEL_TILE < n && *a.bad == SEL_NONE) {        /* (uniform over the workgroup) */
        /* the entry: through the prefix maps, top down; rank 0 is taken.  One dependent load a level */
        uint32_t e = 0;
        for (int k = (int)a.levels - 1; k >= 0; k--) e = a.maps[k][(tile >> (6 * k)) * SEL_WINDOW + e] & (SEL_WINDOW - 1u);
        uint32_t nxt[SEL_PER];
        uint64_t worst;
        select_successors(a, tile, n, s_pos, nxt, worst);
#pragma unroll
        for (uint32_t k = 0; k < SEL_PER; k++) {
            const uint32_t i = k * SEL_THREADS + tid;
            s_j[i] = (uint16_t)nxt[k];
            s_mark[i] = i == e;
        }
        __syncthreads();
        /* round r: s_j spans exactly 2^r steps, the marks are the ranks 0 ... 2^r - 1 steps from the entry; each marks the
         * rank 2^r steps on and every pointer doubles.  Reads in front of the barrier, writes behind it */
        for (int r = 0; r < SEL_ROUNDS; r++) {
            uint32_t two[SEL_PER];
            bool marked[SEL_PER];
#pragma unroll
            for (uint32_t k = 0; k < SEL_PER; k++) {
                const uint32_t j = nxt[k];
                two[k] = j < SEL_TILE ? s_j[j] : j;
                marked[k] = s_mark[k * SEL_THREADS + tid] != 0;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < SEL_PER; k++) {
                if (marked[k] && nxt[k] < SEL_TILE) s_mark[nxt[k]] = 1;
                nxt[k] = two[k];
                s_j[k * SEL_THREADS + tid] = (uint16_t)two[k];
            }
            __syncthreads();
        }
#pragma unroll
        for (uint32_t k = 0; k < SEL_PER; k++) {
            const uint32_t i = k * SEL_THREADS + tid;
            const uint64_t bits = __ballot(s_mark[i] != 0 && tile * SEL_TILE + i < n);
            if (lane == 0) a.marks[tile * SEL_MARK_WORDS + k * (SEL_THREADS / 64) + wave] = bits;
            count += (uint32_t)__popcll(bits);
        }
    }
    if (lane == 0) s_cnt[wave] = count;
    __syncthreads();
    if (wave != 0) return;
    uint32_t total = 0;
#pragma unroll
    for (uint32_t w = 0; w < SEL_THREADS / 64; w++) total += s_cnt[w];
    two_level_arrive(a.scan, tile, a.ntiles, total);
}

/* ---- the selected spans, compacted -------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(SEL_THREADS) void select_emit_kernel(SelectArgs a)
{
    __shared__ uint64_t s_bits[SEL_MARK_WORDS];
    __shared__ uint32_t s_before[SEL_MARK_WORDS];
    const uint32_t tid = threadIdx.x, lane = (uint32_t)lane_id(), wave = tid >> 6;
    const uint64_t tile = blockIdx.x, n = select_n(a);
    if (tile * SEL_TILE >= n || *a.bad != SEL_NONE) return;
    const uint64_t rank0 = two_level_prefix(a.scan, tile);
    if (rank0 >= a.sel_cap) return;
    if (tid < SEL_MARK_WORDS) s_bits[tid] = a.marks[tile * SEL_MARK_WORDS + tid];
    __syncthreads();
    if (tid < SEL_MARK_WORDS) {
        uint32_t before = 0;
        for (uint32_t q = 0; q < tid; q++) before += (uint32_t)__popcll(s_bits[q]);
        s_before[tid] = before;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SEL_PER; k++) {
        const uint32_t w = k * (SEL_THREADS / 64) + wave;
        const uint64_t bits = s_bits[w];
        if (!((bits >> lane) & 1ull)) continue;
        const uint64_t r = rank0 + s_before[w] + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));
        if (r >= a.sel_cap) continue;
        const uint64_t g = tile * SEL_TILE + k * SEL_THREADS + tid;
        a.sel_pos[r] = a.pos[g];
        a.sel_len[r] = a.len[g];
        if (a.sel_rank) a.sel_rank[r] = g;
    }
}

/* ---- the totals and the pad rows ---------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void select_finish_kernel(SelectArgs a)
{
    const uint64_t bad = a.bad ? (uint64_t)*a.bad : SEL_NONE;
    const uint64_t selected = a.bad && bad == SEL_NONE ? *a.scan.total : 0ull;
    const uint64_t written = dmin<uint64_t>(selected, a.sel_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.totals[0] = selected;
        a.totals[1] = written;
        a.totals[2] = bad == SEL_NONE ? (uint64_t)HUFE_OK : (uint64_t)HUFE_ARGUMENT;
        a.totals[3] = bad == SEL_NONE ? 0ull : bad;
    }
    if (!(a.flags & 1u)) return;            /* HUFGPU_SELECT_PAD */
    for (uint64_t r = written + (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.sel_cap; r += (uint64_t)gridDim.x * 256) {
        a.sel_pos[r] = a.pad_pos;
        a.sel_len[r] = 0;
    }
}

}  // namespace hufgpu

/* batch.hpp - the kernels of hufgpu_encode_batch / hufgpu_decode_batch (include/huffman_gpu.h): many independent
   inputs, one launch sequence.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   Encode: the inputs lie back to back and their blocks tile the concatenation, so a batch is one stream whose
   blocks are ragged.  The host uploads the table of block starts (nblocks + 1 input offsets); the kernels below
   read a block's (base, len) from it and run the same force-inlined bodies as hist_lanes_kernel, hist_tree_kernel
   and pack_kernel.  tree_wave_kernel and the two-level size sums serve the batch unchanged.

   Decode: decode_prepare_kernel parses every header of the batch and sums the block lengths over the whole
   stream.  dbatch_rebase_kernel moves each block's output into its item's slot and marks blocks that do not fit
   their slot; the indexed decoders then run unchanged on a TwoLevel whose group prefixes are zero and whose local
   entries are the rebased offsets.  dbatch_fail_kernel and dbatch_result_kernel reduce the block states to one
   result per item. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "hist_lanes.hpp"
#include "hist_tree.hpp"
#include "pack.hpp"

namespace hufgpu {

/* ---- encode ---- */

template <int THREADS>
__global__ __launch_bounds__(THREADS, HL_WAVES_PER_SIMD) void hist_lanes_batch_kernel(const uint8_t *__restrict__ in,
                                                                                      const uint64_t *__restrict__ starts,
                                                                                      uint32_t *__restrict__ hist)
{
    __shared__ __attribute__((aligned(16))) uint8_t hl_lds[HL_LDS_BYTES];
    const uint64_t blk = blockIdx.x;
    const uint64_t base = starts[blk];
    const uint64_t len = starts[blk + 1] - base;
    hl_count<THREADS>(hl_lds, in + base, len, hist + blk * HUF_NSYM);
}

template <int THREADS, bool PACKED>
__global__ __launch_bounds__(THREADS) void hist_tree_batch_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ starts,
                                                                  hufcode_t *__restrict__ codetab, int16_t *__restrict__ treebuf,
                                                                  HufBlockMeta *__restrict__ meta, TwoLevel sizes)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_union[HistTreeLds<THREADS, PACKED>::UBYTES];
    __shared__ uint32_t s_side[2 * THREADS];
    const uint64_t blk = blockIdx.x;
    const uint64_t base = starts[blk];
    const uint64_t len = starts[blk + 1] - base;
    hist_tree_block<THREADS, PACKED>(in + base, len, blk, codetab, treebuf, meta, sizes, s_union, s_side);
}

template <int THREADS, bool SHORT>
__global__ __launch_bounds__(THREADS, SHORT ? PACK_WAVES_PER_SIMD : 4) void pack_batch_kernel(const uint8_t *__restrict__ in,
                                                                                            const uint64_t *__restrict__ starts,
                                                                                            const hufcode_t *__restrict__ codetab,
                                                                                            const int16_t *__restrict__ treebuf,
                                                                                            const HufBlockMeta *__restrict__ meta,
                                                                                            uint64_t *__restrict__ offsets, TwoLevel sizes,
                                                                                            uint8_t *__restrict__ out, HufSubIndex sub)
{
    __shared__ hufcode_t s_code[HUF_NSYM];
    __shared__ uint32_t s_part[THREADS / 64];
    __shared__ uint32_t s_tail[THREADS / 64 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[PACK_STAGE_WORDS];
#ifdef PACK_VGPR_SLACK      /* test builds only: as pack_kernel */
    asm volatile("; one VGPR more than the kernel uses" ::: PACK_VGPR_SLACK);
#endif
    const uint64_t blk = blockIdx.x;
    const uint64_t base = starts[blk];
    const uint64_t len = starts[blk + 1] - base;
    pack_block_any<THREADS, SHORT>(in + base, len, blk, codetab, treebuf, meta, offsets, sizes, out, sub,
                                   s_code, s_part, s_tail, s_stage);
}

/* item_offsets[i] = offsets[item_blocks[i]], i = 0 .. nitems (an empty item starts where the next one does) */
__global__ __launch_bounds__(256) void ebatch_item_offsets_kernel(const uint64_t *__restrict__ offsets,
                                                                   const uint64_t *__restrict__ item_blocks, uint64_t nitems,
                                                                   uint64_t *__restrict__ item_offsets)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= nitems) item_offsets[i] = offsets[item_blocks[i]];
}

/* v[0 .. count) += add: an item's block index, encoded on its own, moved to its place in the batch */
__global__ __launch_bounds__(256) void ebatch_shift_kernel(uint64_t *__restrict__ v, uint64_t count, uint64_t add)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) v[i] += add;
}

/* ---- decode ---- */

struct DecBatchArgs {
    const uint64_t *item_blocks;    /* [nitems + 1] item i = blocks [item_blocks[i], item_blocks[i + 1]); [0] = 0 */
    const uint64_t *out_offsets;    /* [nitems + 1] item i's slot in the output: [out_offsets[i], out_offsets[i + 1]) */
    uint64_t nitems, nblocks;
    HufDecodeMeta *dmeta;           /* decode_prepare_kernel's */
    int32_t *status;
    TwoLevel lens;                  /* decode_prepare_kernel's sums of the block lengths (lens.total: their grand total) */
    uint64_t *bprefix;              /* [nblocks + 1] out: the stream-wide exclusive sums of the block lengths */
    uint64_t *obase;                /* [nblocks] out: where each block's output starts in the batch's output */
    uint32_t *blk_item;             /* [nblocks] out: the item each block belongs to */
    unsigned long long *item_fail;  /* [nitems] first failing block of each item (~0: none) */
    uint64_t *item_res;             /* [3 nitems] out: error, bytes delivered, failing block (~0: none) */
};

/* One thread per block: its item (a binary search in item_blocks), its output offset inside the item - what
 * hufgpu_decode() of the item alone computes - moved to the item's slot, and HUF_ERROR_MEMORY_ALLOCATION for a
 * block that would pass the end of the slot (the check decode_fast / decode_sub make against out_cap).  The first
 * nitems threads also start the items' failure minima. */
__global__ __launch_bounds__(256) void dbatch_rebase_kernel(DecBatchArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.nitems) a.item_fail[t] = ~0ull;
    if (t == a.nblocks) a.bprefix[t] = *a.lens.total;
    if (t >= a.nblocks) return;
    uint64_t lo = 0, hi = a.nitems;                     /* item_blocks[lo] <= t < item_blocks[hi] */
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.item_blocks[mid] <= t) lo = mid;
        else hi = mid;
    }
    const uint64_t first = a.item_blocks[lo];
    const uint64_t g = a.lens.gprefix[t / SCAN_GROUP] + a.lens.local[t];
    const uint64_t g0 = a.lens.gprefix[first / SCAN_GROUP] + a.lens.local[first];
    const uint64_t rel = g - g0;
    const uint64_t slot = a.out_offsets[lo + 1] - a.out_offsets[lo];
    a.bprefix[t] = g;
    a.obase[t] = a.out_offsets[lo] + rel;
    a.blk_item[t] = (uint32_t)lo;
    const HufDecodeMeta m = a.dmeta[t];
    if (m.status == HUFE_OK && m.block_len != 0 && rel + m.block_len > slot) {
        a.dmeta[t].status = HUFE_MEMORY;
        a.status[t] = HUFE_MEMORY;
    }
}

/* after the decoders: every failing block lowers its item's minimum */
__global__ __launch_bounds__(256) void dbatch_fail_kernel(DecBatchArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.nblocks && a.status[t] != HUFE_OK) atomicMin(&a.item_fail[a.blk_item[t]], (unsigned long long)t);
}

/* one thread per item: its error (the first failing block's, in stream order) and the bytes in front of it -
 * hufgpu_decode_result()'s answer before the host replays a failing block */
__global__ __launch_bounds__(256) void dbatch_result_kernel(DecBatchArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nitems) return;
    const uint64_t f = a.item_fail[i];
    const uint64_t lo = a.item_blocks[i];
    uint64_t err = HUFE_OK, raw;
    if (f == ~0ull) {
        raw = a.bprefix[a.item_blocks[i + 1]] - a.bprefix[lo];
    } else {
        err = (uint64_t)(uint32_t)a.status[f];
        raw = a.bprefix[f] - a.bprefix[lo];
    }
    a.item_res[3 * i] = err;
    a.item_res[3 * i + 1] = raw;
    a.item_res[3 * i + 2] = f;
}

}  // namespace hufgpu

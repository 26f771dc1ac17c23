/* append.hpp - the kernels of hufgpu_append and hufgpu_truncate (include/huffman_gpu.h): an indexed stream made longer
   or shorter IN PLACE.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   The records in front of block nb_keep stay where they are and are neither read nor written, so the work is a short
   list of rows, known to the host before any launch: row 0 is the joined block - the `head` bytes of the old block
   that is opened again (an append's tail block, the block a truncate cuts), decoded into the context's scratch area
   by the indexed decoders as they are, with the first new bytes behind them - and every further row is a whole block
   of the new bytes.  With head = 0 every row reads the new bytes.

     decode_prepare_kernel   on a view of ONE block: the header of the block that is opened again (or, with head = 0,
                             of the last block: the canonical check reads it all the same)
     app_plan_kernel         the canonical check - the header's block_len is what (raw_size, blocksize) say - and the
                             rows: (source, length) pairs from one base as in update.hpp, row_blk[r] = r.  A header
                             that fails switches the decoders off for it (block_len = 0)
     the indexed decoders    decode_sub_kernel or decode_fast_kernel, then decode_fix_kernel, on the same view
     app_join_kernel         the head of the new bytes behind the decoded bytes (drange_copy_piece: any alignment)
     hist_*_pairs / tree_wave_kernel (update.hpp, tree.hpp) on the rows
     app_index_kernel        one workgroup: the exclusive sums of the rows' encoded sizes, based at old_index[nb_keep],
                             into CONTEXT memory, and the verdict: the first of the header's error, the decoders'
                             error, a new length over the capacity.  On an error the entry behind the last row is ~0,
                             which pack_pairs_kernel takes for a stream that does not fit: it returns at once
     pack_pairs_kernel       (update.hpp) every row into its place in the caller's stream
     app_commit_kernel       the new index entries into the caller's index, on success only
     app_sub_rows_kernel     the sub-index rows of the blocks that stay, old layout to new layout

   Nothing of the caller's is written before pack, and nothing can fail after app_index_kernel: all or nothing. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "pack.hpp"
#include "ranges.hpp"

namespace hufgpu {

/* acount[]: what the kernels hand to one another and to the host */
#define APP_PLAN_ERR 0              /* the canonical check's verdict (HUFE_*) */
#define APP_ERR      1              /* the call's verdict */
#define APP_TOTAL    2              /* the length of the new stream (0 on an error) */
#define APP_WORDS    4

struct AppendArgs {
    const uint64_t *old_offsets;            /* the caller's block index */
    uint64_t *index_w;                      /* the same, for app_commit_kernel */
    uint64_t nb_keep, rows;                 /* blocks that stay, rows that are encoded */
    uint32_t empty;                         /* the old stream holds no data: its index is not read, the rows start at 0 */
    uint64_t stream_len, stream_cap;
    uint64_t blocksize;
    uint64_t head;                          /* bytes of row 0 that come from the block that is opened again (0: none) */
    uint64_t expect_len;                    /* the block_len its header must show (0: there is no header to check) */
    uint64_t new_bytes;                     /* head + the length of the new bytes = what the rows hold */
    uint64_t src_off, scratch_off;          /* the new bytes and the scratch area from the common base */
    const uint8_t *src;
    uint8_t *scratch_w;
    HufDecodeMeta *dmeta;                   /* [1] decode_prepare_kernel's, of the view */
    const int32_t *status;                  /* [1] */
    const HufBlockMeta *meta;               /* [rows] tree_wave_kernel's */
    uint64_t *pairs;                        /* [2 rows] */
    uint32_t *row_blk;                      /* [rows] */
    uint64_t *sums;                         /* [rows + 2] sums[1 + r]: where row r starts, sums[1 + rows]: the new length or ~0 */
    unsigned long long *acount;             /* [APP_WORDS] */
};

__device__ __forceinline__ uint64_t app_base(const AppendArgs &a) { return a.empty ? 0ull : a.old_offsets[a.nb_keep]; }

/* One thread per row; thread 0 also checks the header. */
__global__ __launch_bounds__(256) void app_plan_kernel(AppendArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0) {
        unsigned long long err = HUFE_OK;
        if (a.expect_len) {
            const HufDecodeMeta m = a.dmeta[0];
            if (m.status != HUFE_OK) err = (unsigned long long)(uint32_t)m.status;
            else if (m.block_len != a.expect_len) err = HUFE_ARGUMENT;
            if (err != HUFE_OK || a.head == 0) a.dmeta[0].block_len = 0;      /* nothing is decoded */
        }
        if (err == HUFE_OK && app_base(a) > a.stream_len) err = HUFE_ARGUMENT;
        a.acount[APP_PLAN_ERR] = err;
    }
    if (r >= a.rows) return;
    const uint64_t at = r * a.blocksize;                      /* of head ++ the new bytes */
    a.pairs[2 * r] = (r == 0 && a.head) ? a.scratch_off : a.src_off + (at - a.head);
    a.pairs[2 * r + 1] = dmin<uint64_t>(a.blocksize, a.new_bytes - at);
    a.row_blk[r] = (uint32_t)r;
}

/* grid (pieces): n bytes of the new bytes behind the decoded head, when the header passed. */
__global__ __launch_bounds__(256) void app_join_kernel(AppendArgs a, uint64_t n)
{
    if (a.acount[APP_PLAN_ERR] != HUFE_OK) return;
    drange_copy_piece(a.scratch_w + a.head, a.src, n, blockIdx.x, gridDim.x);
}

/* One workgroup (scan_sizes_kernel's sweep).  Element 0 of the scan is the base, element 1 + r row r's size. */
template <int THREADS>
__global__ __launch_bounds__(THREADS) void app_index_kernel(AppendArgs a)
{
    const uint64_t base = app_base(a);
    const uint64_t total = chunked_excl_scan<THREADS>(a.rows + 1, a.sums, [&a, base](uint64_t i) -> uint64_t {
        return i == 0 ? base : encoded_block_bytes(a.meta[i - 1]);
    });
    if (threadIdx.x == 0) {
        unsigned long long err = a.acount[APP_PLAN_ERR];
        if (err == HUFE_OK && a.head && a.status[0] != HUFE_OK) err = (unsigned long long)(uint32_t)a.status[0];
        if (err == HUFE_OK && total > a.stream_cap) err = HUFE_MEMORY;
        a.sums[a.rows + 1] = err == HUFE_OK ? total : ~0ull;
        a.acount[APP_ERR] = err;
        a.acount[APP_TOTAL] = err == HUFE_OK ? total : 0ull;
    }
}

/* One thread per row: the entry behind the row.  Entry nb_keep is the base and stays (an empty stream has none: 0). */
__global__ __launch_bounds__(256) void app_commit_kernel(AppendArgs a)
{
    if (a.acount[APP_ERR] != HUFE_OK) return;
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r == 0 && a.empty) a.index_w[a.nb_keep] = a.sums[1];
    if (r < a.rows) a.index_w[a.nb_keep + r + 1] = a.sums[r + 2];
}

/* One workgroup per block that stays: its sub-index row from the old layout to the new one (the arrays of a sub-index
 * are sized by the block count, so every row has another place).  These are whole blocks of row_syms bytes whose
 * headers are not read: a one-symbol block's row, which the encoder does not write, is carried over as it is. */
__global__ __launch_bounds__(256) void app_sub_rows_kernel(HufSubIndex from, HufSubIndex to, uint64_t row_syms,
                                                           const unsigned long long *__restrict__ acount)
{
    if (acount[APP_ERR] != HUFE_OK) return;
    const uint64_t b = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint64_t nt = (row_syms + HUF_SUB_TILE - 1) / HUF_SUB_TILE, ng = (row_syms + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP;
    for (uint64_t t = tid; t < nt; t += 256) to.tile_bits[b * to.tpb + t] = from.tile_bits[b * from.tpb + t];
    const uint64_t *g_from = reinterpret_cast<const uint64_t *>(from.group_bits + b * from.gpb);    /* rows of 16-byte multiples */
    uint64_t *g_to = reinterpret_cast<uint64_t *>(to.group_bits + b * to.gpb);
    for (uint64_t w = tid; w < ng / 4; w += 256) g_to[w] = g_from[w];
    if (tid < (ng & 3u)) to.group_bits[b * to.gpb + (ng & ~3ull) + tid] = from.group_bits[b * from.gpb + (ng & ~3ull) + tid];
    if (tid < HUF_NSYM / 8)
        reinterpret_cast<uint64_t *>(to.lens + b * HUF_NSYM)[tid] = reinterpret_cast<const uint64_t *>(from.lens + b * HUF_NSYM)[tid];
}

}  // namespace hufgpu

/*
 * hufgpu_kernels.hip - CDNA4 (gfx950) kernels of the Huffman block codec.
 *
 * One libhuffman block (config->blocksize input bytes, src/encoder.c:288-293) is the unit of
 * parallelism everywhere: blocks never exchange data, so every kernel maps blocks to
 * workgroups and the grid is simply the block count.
 *
 *   encode:  hist_tree_kernel -> pack_kernel
 *            (blocks >= 4 MiB are cut into chunks of 256 KiB, one workgroup each: chunk_hist -> block_hist ->
 *            tree -> scan_sizes -> chunk_total -> chunk_scan -> pack_chunk)
 *   decode:  decode_prepare_kernel -> decode_kernel (block index known)
 *            decode_prepare_kernel -> decode_sub_kernel -> decode_fix_kernel (block index and the
 *            encoder's sub-index known), or decode_chain_kernel (raw stream, blocks in order)
 *   sub-index of a stream that came without one: sub_lens_kernel -> sub_groups_kernel (-> sub_chunk_scan_kernel ->
 *            sub_tile_add_kernel for blocks of 2 MiB and more)
 *   overwrite of byte ranges: decode_prepare_kernel -> drange_plan / drange_mark -> upd_class -> the indexed decoders on
 *            the staged blocks -> upd_overlay -> hist_*_pairs -> upd_index -> pack_pairs, update_copy_kernel
 *   overwrite of records at device-resident positions, enqueue-only (hufgpu_scatter): decode_prepare_kernel, scat_mark ->
 *            gather_scan / gather_place -> scat_class -> the indexed decoders on the staged blocks -> scat_overlay ->
 *            scat_hist_* -> upd_index -> scat_pack, update_copy_kernel -> scat_result
 *   served straight from stream, block index and sub-index, tile by tile (sub_tile.hpp: the one checked tile item):
 *            drange_tiles_kernel, gather_serve_kernel, find_sub_kernel, find_pat_sub_kernel, find_rec_sub_kernel
 *   byte values looked for (hufgpu_find_bytes): find_sub -> find_scan -> find_finish (-> find_emit), no decoded byte stored
 *   a pattern of bytes looked for (hufgpu_find_pattern): find_pat_sub (-> find_seam: the matches that leave their tile, from
 *            the tiles' edge bytes) -> find_scan -> find_finish (-> find_emit)
 *   the records that hold a pattern (hufgpu_find_records): find_rec_sub (match and delimiter masks of one walk) (-> find_seam)
 *            -> find_rec_dscan -> find_rec_mark -> find_scan -> find_finish (-> find_rec_emit)
 *   grep -o's non-overlapping matches chosen from the spans of a search (hufgpu_select_spans): select_tile -> select_compose
 *            (once a level) -> select_mark -> select_emit -> select_finish
 *   append / truncate in place: decode_prepare_kernel on the one block that is opened again -> app_plan -> the indexed
 *            decoders on it -> app_join -> hist_*_pairs -> app_index -> pack_pairs -> app_commit (-> app_sub_rows)
 *
 * Wave size is 64 throughout (hard-coded, gfx950 only).  All arithmetic is integer.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hufgpu_common.h"

#include "kernels/util.hpp"
#include "kernels/histogram.hpp"
#include "kernels/tree.hpp"
#include "kernels/offsets.hpp"
#include "kernels/hist_tree.hpp"
#include "kernels/hist_lanes.hpp"
#include "kernels/pack.hpp"
#include "kernels/hist_chunk.hpp"
#include "kernels/pack_chunk.hpp"
#include "kernels/decode.hpp"
#include "kernels/decode_sub.hpp"
#include "kernels/sub_tile.hpp"
#include "kernels/decode_fast.hpp"
#include "kernels/decode_regs.hpp"
#include "kernels/spec_index.hpp"
#include "kernels/discover.hpp"
#include "kernels/fill.hpp"
#include "kernels/batch.hpp"
#include "kernels/ranges.hpp"
#include "kernels/range_tiles.hpp"
#include "kernels/gather.hpp"
#include "kernels/find.hpp"
#include "kernels/select.hpp"
#include "kernels/sub_build.hpp"
#include "kernels/update.hpp"
#include "kernels/scatter.hpp"
#include "kernels/append.hpp"

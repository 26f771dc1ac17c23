/* find.hpp - the kernels of the search family (include/huffman_gpu.h): where in the original data the bytes of a set of
   byte values lie, where a pattern of 1 to 64 bytes - or of 1 to 64 sets of byte values, or any of several such patterns -
   starts, or which records between delimiters hold it (or do not), straight from stream, block index and sub-index.  No
   decoded byte reaches device memory (the pattern calls keep at most 126 edge bytes a tile) and the host only enqueues.
   Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   Positions are the layout's: block b holds [b B, b B + min(B, raw_size - b B)).  Tile: 2048 symbols; group: a lane's 32.
   call                            chain of kernels ([..]: only when positions / records are asked for)
   hufgpu_find_bytes               find_sub                        -> find_scan -> find_finish [-> find_emit]
   hufgpu_find_pattern             find_pat_sub     -> find_seam     -> find_scan -> find_finish [-> find_emit]
   hufgpu_find_classes             find_cls_sub     -> find_cls_seam -> find_scan -> find_finish [-> find_emit]
   hufgpu_find_any                 find_alt_sub     -> find_alt_seam -> find_scan -> find_finish [-> find_emit]
   hufgpu_find_records             find_rec_sub     -> find_seam     -> RECORDS
   hufgpu_find_records_classes     find_rec_cls_sub -> find_cls_seam -> RECORDS
   hufgpu_find_records_any         find_rec_alt_sub -> find_alt_seam -> RECORDS
   hufgpu_find_records_select      find_rec_alt_sub -> find_alt_seam -> RECORDS with [find_rec_invert] behind find_rec_mark
                                   and, for the numbers, find_rec_first_bad -> find_rec_emit_no in the place of find_rec_emit
   hufgpu_find_records_context     the select call's chain with find_ctx_dscan in the place of find_rec_dscan and, behind
                                   find_rec_mark [-> find_rec_invert], find_scan (of the selected records' counts, into a scan
                                   of its own) -> find_rec_ctx, whose second mask the rest of the chain takes; with d_rec_sel
                                   find_ctx_emit / find_ctx_emit_no in the place of the emit kernel.  before = after = 0:
                                   the select call's launches but for that emit kernel
   hufgpu_find_any_anchored        anchors = 0: hufgpu_find_any's chain.  EOL / WORD: find_anc_seam in the place of
                                   find_alt_seam (the table has one position more an alternative).  BOL / WORD: the walk is
                                   find_rec_alt_sub with the boundary set in the delimiters' place, and find_anchor runs
                                   behind the seam kernel; then find_scan -> find_finish [-> find_emit] as ever
   hufgpu_find_records_anchored    anchors = 0: the context call's chain.  EOL / WORD: find_anc_seam.  BOL alone:
                                   find_anchor on the delimiters' mask, behind the seam kernel and in front of dscan / mark.
                                   WORD: find_sub walks the stream a second time, behind find_rec_alt_sub, for a third mask -
                                   the bytes that may stand in front of a match -, which find_anchor takes
   hufgpu_find_records_terms       n_terms = 1: the context call's chain.  2 to 4 terms: find_rec_term_sub -> find_term_seam ->
                                   dscan -> find_rec_mark ONCE A TERM (term t's match mask into term t's record mask) ->
                                   find_rec_all (the AND of the record masks, into the mask that mark leaves for the other
                                   calls) [-> find_scan once a term (of the terms' match counts, into scans of their own) ->
                                   find_rec_seq: ORDERED only], then the context call's chain from [find_rec_invert] on
   hufgpu_find_any_quant           no optional position: hufgpu_find_any's chain.  Else find_opt_sub -> find_opt_seam in the
                                   place of find_alt_sub -> find_alt_seam: the any-of automaton closed over the optional
                                   positions a byte (find_opt_step); the seam kernel runs it on a window of the edge bytes in LDS
   hufgpu_find_records_quant       no optional position: the context call's chain.  Else find_rec_opt_sub -> find_opt_seam in
                                   the place of find_rec_alt_sub -> find_alt_seam, then that chain as it is
   hufgpu_find_any_expr            one of anchors and optional positions alone: the anchored call's, the quant call's chain.
                                   Both: find_opt_sub - find_rec_opt_sub when the byte in front is tested - and, with EOL / WORD,
                                   find_opt_anc_seam in the place of find_opt_seam: the window with the end of the data as a
                                   boundary; BOL / WORD: find_anchor behind the seam kernel
   hufgpu_find_records_expr        one term: as the positions call, on the context call's chain (WORD: find_sub a second time).
                                   2 to 4 terms without an optional position or an anchor: the terms call's chain.  Else
                                   find_rec_term_opt_sub -> find_term_opt_seam in the place of find_rec_term_sub -> find_term_seam,
                                   and - ORDERED with BOL / WORD - find_anchor over term 0's mask in front of dscan / mark
   hufgpu_find_any_spans           the expr positions call's chain to its end, then find_span: the walk's grid once more, for the
                                   tiles with a start below pos_cap.  No optional position and one length for all alternatives:
                                   find_emit_len in the place of find_emit, and no find_span
   RECORDS = find_rec_dscan -> find_rec_mark -> find_scan -> find_finish [-> find_rec_emit]; no seam kernel for 1 byte

   The walk: find_sub_body, the nine *_sub kernels, find_rec_term_sub_kernel and find_rec_term_opt_sub_kernel
     Workgroup = one (block, chunk of 65 536 symbols), decode_sub_kernel's geometry with eight waves; a wave takes the
     chunk's tiles wave, wave + 8, ...  The header is parsed and its length must be the layout's, the tables come from
     dsub_fast_tables (the claimed code lengths checked against the stream's tree), and EVERY tile of EVERY chunk is the
     item of sub_tile.hpp, with its checks: (a) the block's first tile starts at payload bit 0, (b) every group takes
     exactly the bits it is said to have and no walk leaves tree or payload, (c) a tile ends where the next tile of the
     block is said to start (the last: inside the payload).  The whole block is walked, so the induction of
     decode_sub.hpp closes and the caller vouches for nothing: a block is served exactly or its status says that it is
     not.  A lane's 32 decoded bytes lie in the wave's 2 KiB of LDS (dsub_tile_slow: codes of any length, groups of any
     size); what leaves the workgroup is ONE 32-bit match mask per group (a bitmap row per block: block starts need not
     be 32-aligned raw positions) and the tile's match count.  A block of one byte value has no sub-index rows: its
     payload bits are seen to be 0 and its mask words are all ones or all zeros, cut where the block or the tile ends.
       bytes     the lane's 32 bytes against the set, eight words in LDS;
       pattern   a set bit is a match's START.  A lane tests the starts s among its 32 with s + pattern_len <= the tile's
                 symbols, reading on into its neighbours' bytes of the wave's slice (find_pat_lane): the matches INSIDE
                 one tile.  The wave also stores the tile's edges: its first and its last min(symbols, pattern_len - 1)
                 bytes, in a slot of 2 x 64 bytes a tile;
       classes   the 2 KiB table (FindClsTable, transposed: a 64-bit set of positions a byte value) lies in LDS in the
                 place of the 64 pattern bytes, and the lane matcher is a Shift-And automaton over the reversed pattern
                 (find_cls_lane): one table look-up a byte, 32 + pattern_len - 1 (+ 3) a lane, whatever the data;
       any-of    the alternatives lie one below the other in the 64 bits of the same table (FindAltArgs); a start is a
                 byte at which the start bit of ANY alternative is set.  A lane warms up over the longest alternative's
                 length - 1 bytes, the edges are that many, and the walk sets the starts at which the LONGEST
                 alternative fits in the tile, whichever alternative lies there;
       records   next to all that a DELIMITER mask word a group - the lane's 32 bytes against the delimiter set in
                 LDS - and the tile's delimiter count;
       terms     the any-of records' walk with the alternatives in 2 to 4 TERMS: the start bits are kept apart by term
                 (FindTerms::starts), and a match mask word a group and a count a tile leave the workgroup for EVERY term,
                 term-major; plen, the edges and the walk / seam split are the longest alternative's of all terms;
       anchored  no walk kernel of its own.  The byte BEHIND a match needs no kernel: it is one position more an
                 alternative in the table - its class the delimiters, the bytes that are no word byte, or both -, plen is
                 the longest alternative + 1, and edges, warm-up and the walk / seam split follow it as they always did.

   The seams: find_seam_kernel, find_cls_seam_kernel, find_alt_seam_kernel, find_anc_seam_kernel
     One wave a tile, a lane a start among the tile's last plen - 1 (plen: the pattern's length, the LONGEST one of
     alternatives): the matches that leave their tile.  find_seam_lane locates the lane's start, find_seam_candidate
     answers for one pattern whether it lies there, and it holds the layout walk, the only one there is: byte k comes
     from the tile's own tail slot while it lies in the tile, then from the HEAD of whichever later tile holds it (it
     lies within plen - 1 of that tile's start), over the layout's tile lengths across chunks and blocks.  A start is
     dropped when it would end behind raw_size or when any block it touches is not served.  The any-of kernel asks once
     per alternative - a short one that ends inside the tile included - until one lies there: one bit and one count a
     start however many do.  find_seam_end ORs the starts into the start tile's mask words and adds them to its count,
     BEFORE the scan.  find_anc_seam_kernel is the any-of kernel for tables with a boundary position: the one case that a
     table cannot express is the match that ends where the data ends - no byte to look up -, and that start lies among its
     tile's last plen - 1, so the kernel asks for such an alternative without its last position.
     find_anchor_kernel    the byte in FRONT of a match, behind the seam kernel: a wave a tile, a lane a word,
                           m &= (b << 1) | carry with b the walk's mask of the bytes that may stand there; the carry comes
                           from the lane below, the tile in front, the block in front (0 when that one is not served, 1
                           at byte 0); then the tile's count anew.

   Behind them
     find_scan_kernel      the tile counts, gated by their block's status, summed by the two-level / ticket scan of
                           offsets.hpp: a tile's rank among the matches of the served blocks; the grand total goes to
                           d_totals[0], the blocks that are not served are counted into d_totals[2];
     find_finish_kernel    per-block counts as differences of the tiles' ranks, and d_totals[1];
     find_emit_kernel      one wave a tile, a lane a mask word: rank = the tile's + the wave's scan of popcounts, and
                           b B + 32 g + bit goes to d_pos[rank] for every set bit whose rank is below pos_cap.

     find_span_kernel      hufgpu_find_any_spans: the length of the longest form at every reported start.  The walk's geometry; a
                           chunk without a start below the cap leaves before it builds tables, a tile with one is decoded
                           again into LDS (the checked item, as in the walk) and every set bit of the FINAL mask starts a
                           forward Shift-And run - seeded once, find_opt_step over a table of the reversed positions - that
                           remembers the last accepting step; bytes behind the tile come from the head edges of the tiles
                           behind, by the seam kernels' layout walk.  d_len, d_open by the emit kernel's ranks; d_totals[3].
     find_emit_len_kernel  find_emit_kernel with a constant length a start: the span call for patterns of one length.

   Records.  A record is [s, e) between two delimiters (or byte 0, or raw_size) and is reported once, when it holds a
   match and every block from the delimiter in front of it to the one that ends it is served.
     find_rec_dscan_kernel the second two-level scan: the delimiters in front of every tile.
     find_rec_mark_kernel  a wave a tile: every match sets the bit of its record's start in a third mask, by atomic OR -
                           which is what makes a record with many matches one entry.  The start is the bit behind the last
                           delimiter in front of the match: in the lane's own word, else in the tile's words (one ballot
                           and two shuffles a lane), else - for the matches in front of the tile's first delimiter only,
                           so once a TILE - in the nearest tile in front that has a delimiter, found by a binary search in
                           the scanned counts: O(log tiles) reads however far away it is, then a bit scan of that tile's
                           64 words.  The end is looked for in the same way, forward, to drop the records whose end is
                           unknown BEFORE anything is counted.  Whoever turns a bit from 0 to 1 counts it for the tile
                           that holds it; find_scan_kernel and find_finish_kernel run on those counts: ranks,
                           d_totals[0..2], and d_block_counts by the block that holds the record's START.
     find_rec_invert_kernel   the non-empty records of known extent WITHOUT a match: local to its tile, plain stores over
                           mark's words and counts.
     find_rec_emit_kernel  find_emit_kernel with a length: the end is the first delimiter behind the start; pos and
                           min(e - s, clip) go to the record's rank, the cut ones are counted into d_totals[3].  With
                           find_rec_first_bad_kernel in front, find_rec_emit_no_kernel adds the record's number: the
                           delimiters in front of it, known while no block in front of the record's is unserved.
     find_rec_ctx_kernel   hufgpu_find_records_context: the records AROUND the selected ones.  A dilation of rbits in
                           record-number space into a second mask and count array, on which scan, finish and emit then
                           run; a record's number comes from find_ctx_dscan_kernel's scan, in which a tile of a block that
                           is not served weighs more than either distance, and the nearest selected record of other tiles
                           from a scan of rcnt: three look-ups a tile at most.  find_ctx_emit_kernel and
                           find_ctx_emit_no_kernel are the emit kernels with a flag a record: is it one of the selected.

   Invariants
     Zeroed by the host before the first kernel: the statuses d_block_errs, d_totals, and for the records rbits and rcnt
     (the terms' call: every term's rbits and rcnt in their place - find_rec_all_kernel writes the call's own with plain stores).
     Every other word that a later kernel reads is written by the walk: the mask word of every group and the count of every
     tile of every block whose header parses (the rest is never read: every reader looks at the status first).
     Any failed check of any chunk raises the block's status to HUF_ERROR_READ_WRITE (atomic max, find_raise); nothing is
     decided on the host.  The statuses are FINAL when the walk kernel has ended: later kernels read them, none writes them.
     A virtual delimiter: find_rec_dscan_kernel counts ONE delimiter that is nowhere for every tile of a block that is not
     served.  A look-up that lands on one learns that the record's start or end is unknown, and the record is dropped; a
     record's number is unknown behind one. */
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

#define FIND_PAT_MAX 64                     /* = HUFGPU_FIND_PATTERN_MAX (include/huffman_gpu.h) */
#define FIND_EDGE_SLOT 128                  /* bytes a tile: its head at 0, its tail at 64, pattern_len - 1 <= 63 bytes each */
#define FIND_SEAM_THREADS 256

struct FindPatArgs {
    FindArgs f;
    uint32_t pat[FIND_PAT_MAX / 4];         /* the pattern, byte k in bits 8 (k & 3) of word k >> 2; zeros behind it */
    uint32_t plen;
    uint8_t *edges;                         /* [ntiles][FIND_EDGE_SLOT] */
};

/* hufgpu_find_records: the pattern route with a second mask.  p.f.set is the delimiter set, p.f.pos / p.f.pos_cap are the
 * records' starts and their cap, p.f.bitmap / p.f.tcnt hold the match starts and their counts; scan, finish and emit get a
 * copy whose tcnt is rcnt */
struct FindRecArgs {
    FindPatArgs p;
    uint32_t *dbits;                        /* [nblocks][wpb] delimiter masks, one word a group */
    uint32_t *dcnt;                         /* [nblocks][tpb] delimiters of a tile */
    uint32_t *rbits;                        /* [nblocks][wpb] the starts of the records to report; zero when the first kernel starts */
    uint32_t *rcnt;                         /* [nblocks][tpb] ... and how many of them a tile holds; zero as well */
    TwoLevel dscan;                         /* of the tiles' delimiter counts, 1 for a tile of a block that is not served */
    uint32_t *len;
    uint32_t clip;                          /* max_len, or 2^32 - 1 */
};

__device__ __forceinline__ uint64_t find_block_len(const FindArgs &a, uint64_t b)
{
    return dmin<uint64_t>(a.s.bsize, a.s.raw_size - b * a.s.bsize);
}

/* tile (b, t) of the layout: its symbols */
__device__ __forceinline__ uint32_t find_tile_syms(uint64_t blen, uint64_t t) { return (uint32_t)dmin<uint64_t>(HUF_SUB_TILE, blen - t * HUF_SUB_TILE); }

/* the bits 0 ... n - 1 of a word; all of them for n >= 32 */
__device__ __forceinline__ uint32_t find_low_bits(uint32_t n) { return n < 32u ? (1u << n) - 1u : 0xffffffffu; }

/* the block is not served: `who` raises its status */
__device__ __forceinline__ void find_raise(const FindArgs &a, uint64_t b, bool who)
{
    if (who) atomicMax(&a.errs[b], (int32_t)HUFE_RW);
}

/* a wave = one tile, for the kernels of THREADS threads behind the walk: the wave's index i - no such tile from ntiles on -
 * and for i < ntiles the tile (b, t) and its block's length.  The exits, and whether the block is served, are the caller's. */
struct FindTile {
    uint64_t b, t, blen;                    /* i = b * tpb + t; there is such a tile while t * HUF_SUB_TILE < blen */
};
template <uint32_t THREADS>
__device__ __forceinline__ uint64_t find_tile_index()
{
    const uint32_t wave = uni32(threadIdx.x >> 6);
    return (uint64_t)blockIdx.x * (THREADS / 64) + wave;
}
__device__ __forceinline__ FindTile find_tile(const FindArgs &a, uint64_t i)
{
    const uint64_t b = i / a.tpb;
    return {b, i % a.tpb, find_block_len(a, b)};
}

/* how many of the lane's 32 starts - its first 0 to 32 - are starts at which plen bytes still lie inside the tile's tsym symbols */
__device__ __forceinline__ uint32_t find_fit(uint32_t plen, uint32_t tsym, uint32_t lane)
{
    const uint32_t fit = tsym >= plen ? tsym - plen + 1u : 0u;      /* starts of the tile at which the pattern fits */
    return fit > 32u * lane ? dmin<uint32_t>(32u, fit - 32u * lane) : 0u;
}

/* the starts among the lane's 32 at which the pattern lies, all of it inside the tile's tsym symbols: candidates by
 * the first byte (the lane's own words w), each verified word by word against the wave's slice; bytes behind
 * start + plen never reach a comparison, so what is stale behind a short tile does not either */
__device__ __forceinline__ uint32_t find_pat_lane(const uint32_t *tile_words, const uint32_t (&w)[8], const uint32_t *s_pat, uint32_t plen,
                                                  uint32_t tsym, uint32_t lane)
{
    const uint32_t first = s_pat[0] & 0xffu;
    uint32_t cand = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int i = 0; i < 4; i++) cand |= (uint32_t)(((w[j] >> (8 * i)) & 0xffu) == first) << (4 * j + i);
    }
    const uint32_t mine = find_fit(plen, tsym, lane);
    cand = mine == 0u ? 0u : (mine < 32u ? cand & ((1u << mine) - 1u) : cand);
    const uint32_t nw = (plen + 3u) >> 2;
    const uint32_t last = (plen & 3u) ? (1u << (8u * (plen & 3u))) - 1u : 0xffffffffu;
    uint32_t m = 0;
    while (cand != 0u) {
        const uint32_t bit = (uint32_t)__builtin_ctz(cand);
        cand &= cand - 1u;
        const uint32_t s = 32u * lane + bit, sh = 8u * (s & 3u);
        uint32_t idx = s >> 2, lo = tile_words[idx];
        bool same = true;
        for (uint32_t k = 0; k < nw; k++) {
            idx = dmin<uint32_t>(idx + 1u, HUF_SUB_TILE / 4 - 1u);  /* (the slice's last word again: those bytes lie behind the pattern) */
            const uint32_t hi = tile_words[idx];
            const uint32_t x = __builtin_amdgcn_alignbit(hi, lo, sh);
            if (((x ^ s_pat[k]) & (k + 1u == nw ? last : 0xffffffffu)) != 0u) {
                same = false;
                break;
            }
            lo = hi;
        }
        m |= (uint32_t)same << bit;
    }
    return m;
}

/* hufgpu_find_classes / hufgpu_find_records_classes: every position k of the pattern is a SET of byte values.  The table
 * is transposed: m[v] holds the positions that byte value v may take, position k at bit 63 - k, as two 32-bit halves
 * (m[v][0] the low one).  `full` has the bits 63 ... 64 - plen of all positions, `first` the lowest of them - that of the
 * pattern's LAST position, where the automaton of find_cls_lane starts.  2 KiB, carried in the kernels' arguments. */
struct FindClsTable {
    uint32_t first[2], full[2];
    uint32_t m[256][2];
};
struct FindClsArgs {
    FindRecArgs r;                          /* r.p.pat is not looked at; the pattern call leaves r's own members 0 */
    FindClsTable t;
};
static_assert(sizeof(FindClsArgs) <= 4096, "a kernel's arguments end at 4 KiB");

/* hufgpu_find_any / hufgpu_find_records_any: SEVERAL class patterns - alternatives - share the 64 bits of the automaton's
 * state.  Alternative 0 takes the bits 63 ... 64 - len_0 of the table, alternative 1 the next len_1 bits down, and so on:
 * position k of alternative j is bit hi_j - k.  `starts` has bit hi_j of every alternative (a match of j starts at this
 * byte), t.first holds the bits of all the alternatives' LAST positions, where the automaton starts them: the bit that
 * the shift moves out of alternative j's start lands on alternative j - 1's last position, which is set there anyway, so
 * no bits are needed between two alternatives.  r.p.plen is the LONGEST alternative's length: the edge bytes a tile
 * keeps, a lane's warm-up and the split of the starts between the walk and the seam kernel follow it.  hl[j] is
 * hi_j | len_j << 8, for the seam kernel. */
struct FindAltArgs {
    FindRecArgs r;
    FindClsTable t;                         /* t.first: the last positions' bits; t.full: every used bit */
    uint32_t starts[2];                     /* ([0] the low half) */
    uint32_t n_alts;
    uint16_t hl[FIND_PAT_MAX];
};
static_assert(sizeof(FindAltArgs) <= 4096, "a kernel's arguments end at 4 KiB");

/* hufgpu_find_records_terms: the alternatives of the any-of table in 2 to FIND_TERMS_MAX TERMS, a term the alternatives
 * j with bits 6 and 7 of hl[j] equal to its index.  starts[t] has the start bits of term t's alternatives only, so
 * (state & starts[t]) != 0 says "a match of term t starts at this byte"; len[t] is the one length of an ordered call's term.
 * The walk and the seam kernel write a match mask and tile counts a term, find_rec_mark_kernel makes a record mask and
 * counts a term of them: all term-major, [n_terms][nwords] words and [n_terms][ntiles] counts (ntiles is the FindArgs'). */
#define FIND_TERMS_MAX 4                    /* = HUFGPU_FIND_TERMS_MAX (include/huffman_gpu.h) */
struct FindTerms {
    uint32_t n_terms;
    uint32_t len[FIND_TERMS_MAX];
    uint32_t starts[FIND_TERMS_MAX][2];     /* ([0] the low half) */
    uint32_t *mbits, *mcnt;                 /* the terms' match starts and how many a tile holds */
    uint32_t *rbits, *rcnt;                 /* the terms' record starts and how many a tile holds; zero when the first kernel starts */
    uint64_t nwords;                        /* nblocks * wpb */
};
struct FindTermArgs {
    FindAltArgs a;                          /* a.r.p.f.bitmap / tcnt are not looked at: the terms have their own */
    FindTerms t;
};
static_assert(sizeof(FindTermArgs) <= 4096, "a kernel's arguments end at 4 KiB");

#define FIND_CLS_WORDS 512                  /* the table's words in LDS: m[v] at words 2 v and 2 v + 1 */

/* one byte of the Shift-And automaton that runs over the REVERSED pattern, from high addresses to low ones: bit 63 - k of
 * the state says that the bytes read so far, the last one being byte i, end with positions k ... plen - 1 of the pattern
 * at i; bit 63 - the sign of `hi` - that the pattern STARTS at i.  Shifts by constants, 32 bits at a time. */
__device__ __forceinline__ void find_cls_step(uint32_t &lo, uint32_t &hi, const uint32_t *s_m, uint32_t first_lo, uint32_t first_hi, uint32_t x)
{
    const uint2 mv = *reinterpret_cast<const uint2 *>(s_m + 2u * x);
    hi = ((hi << 1) | (lo >> 31) | first_hi) & mv.y;
    lo = ((lo << 1) | first_lo) & mv.x;
}

/* hufgpu_find_any_quant / hufgpu_find_records_quant: some positions of the any-of table are OPTIONAL, so an alternative
 * stands for all its forms - every way of leaving optional positions out.  The table, `starts` and hl are the any-of call's
 * (r.p.plen: the longest alternative's POSITION count, the length of its longest form); t.first is wider: the bits of all
 * positions that may hold a form's LAST byte - an alternative's last position and, while that one is optional, the one in
 * front of it, up to the first required one.  Three masks describe the maximal runs of optional positions top ... low (top
 * the higher bit): o has the run's bits, i the bit just below the run (position low + 1), f the bit of top.  A run that
 * ends its alternative has no position below it: its lowest bit comes in through t.first, is that run's i and is left out
 * of o.  So no borrow of find_opt_step's subtraction leaves an alternative, and no bits are needed between two of them. */
struct FindOpt {
    uint32_t o[2], i[2], f[2];              /* ([0] the low half) */
};
struct FindOptArgs {
    FindAltArgs a;
    FindOpt q;
};
static_assert(sizeof(FindOptArgs) == sizeof(FindAltArgs) + 24 && sizeof(FindOptArgs) <= 4096, "a kernel's arguments end at 4 KiB");

/* hufgpu_find_any_expr / hufgpu_find_records_expr, where they cross what the older calls keep apart: optional positions
 * in a table with boundary positions (anchors), in several terms, or anchors around ordered terms.  qa is the quant calls'
 * - with no optional position its three masks are 0 and find_opt_step is find_cls_step -, t the terms' (n_terms = 0: one
 * term, and the one mask and count of qa.a.r.p.f), and bnd has the bits of the BOUNDARY positions: those of every alternative
 * whose byte behind a match is tested, which the seam kernel takes as met where the data ends. */
struct FindExprArgs {
    FindOptArgs qa;
    uint32_t bnd[2];                        /* ([0] the low half) */
    FindTerms t;
};
static_assert(sizeof(FindTermArgs) + sizeof(FindOpt) <= 4096 && sizeof(FindExprArgs) <= 4096, "a kernel's arguments end at 4 KiB");

/* find_cls_step and the closure over the optional positions (Navarro and Raffinot's extended patterns): a set bit just
 * below or inside a run of optional positions sets every bit of the run above it - "those positions are left out".
 * Df - I clears the lowest set bit of every block i ... f and sets the bits below it, so ~(Df - I) ^ Df has exactly the bits
 * above that lowest one; f bounds the borrow.  One subtraction with borrow out, one with borrow in, four logic operations a
 * half; o, i and f are the kernel's arguments, the same for every lane. */
__device__ __forceinline__ void find_opt_close(uint32_t &lo, uint32_t &hi, const FindOpt &q)
{
    const uint32_t dl = lo | q.f[0], dh = hi | q.f[1];
    const uint64_t d = (((uint64_t)dh << 32) | dl) - (((uint64_t)q.i[1] << 32) | q.i[0]);
    lo |= q.o[0] & (~(uint32_t)d ^ dl);
    hi |= q.o[1] & (~(uint32_t)(d >> 32) ^ dh);
}
__device__ __forceinline__ void find_opt_step(uint32_t &lo, uint32_t &hi, const uint32_t *s_m, uint32_t first_lo, uint32_t first_hi, uint32_t x,
                                              const FindOpt &q)
{
    find_cls_step(lo, hi, s_m, first_lo, first_hi, x);
    find_opt_close(lo, hi, q);
}

/* the automaton's step of a walk: OPT, the one with the closure */
template <bool OPT>
__device__ __forceinline__ void find_step(uint32_t &lo, uint32_t &hi, const uint32_t *s_m, uint32_t first_lo, uint32_t first_hi, uint32_t x,
                                          [[maybe_unused]] const FindOpt *q)
{
    if constexpr (OPT) find_opt_step(lo, hi, s_m, first_lo, first_hi, x, *q);
    else find_cls_step(lo, hi, s_m, first_lo, first_hi, x);
}

/* find_pat_lane for classes: the starts among the lane's 32 at which every byte is in its position's class, all of it
 * inside the tile's tsym symbols.  The lane warms the automaton up on the (plen - 1 rounded up to words) bytes behind
 * its 32 - its neighbours' bytes of the wave's slice, read from the far end - and then takes its own 32 from the last to
 * the first, so that a match is seen AT its start and every lane writes its own word only: 32 + plen - 1 (+ 3) table
 * look-ups a lane whatever the data and the classes are.  Bit 63 of the state depends on the plen bytes from the start on
 * and on nothing else, and the starts with start + plen > tsym are masked: what is stale behind a short tile - or the
 * slice's last word read again behind the tile's end - reaches no decision.
 * ALT (hufgpu_find_any): the state holds several alternatives, plen is the longest one's length, and a start is a byte at
 * which ANY bit of `starts` is set.  Alternative j's start bit depends on the len_j <= plen bytes from the start on and on
 * nothing else, so the same mask of the starts serves: the walk sets the starts with start + plen <= tsym, whichever
 * alternative lies there, and find_alt_seam_kernel has the tile's last plen - 1 starts for every alternative.
 * OPT (hufgpu_find_any_quant): the step is find_opt_step with q's masks, and plen is the longest alternative's position
 * count.  A start bit behind byte i depends on the bytes i ... i + plen - 1 and on nothing else - no form is longer -, so
 * warm-up, find_fit and the mask of the starts are the any-of walk's; find_opt_seam_kernel has the tile's last plen - 1 starts. */
template <bool ALT = false, bool OPT = false>
__device__ __forceinline__ uint32_t find_cls_lane(const uint32_t *tile_words, const uint32_t (&w)[8], const uint32_t *s_m, uint32_t first_lo,
                                                  uint32_t first_hi, uint32_t plen, uint32_t tsym, uint32_t lane,
                                                  [[maybe_unused]] uint32_t starts_lo = 0, [[maybe_unused]] uint32_t starts_hi = 0,
                                                  [[maybe_unused]] const FindOpt *q = nullptr)
{
    static_assert(ALT || !OPT, "optional positions: the any-of route's");
    uint32_t lo = 0, hi = 0;
    for (uint32_t k = (plen + 2u) >> 2; k-- > 0u;) {                /* the words that hold the plen - 1 bytes behind the lane's */
        const uint32_t x = tile_words[dmin<uint32_t>(8u * lane + 8u + k, HUF_SUB_TILE / 4 - 1u)];
#pragma unroll
        for (int i = 3; i >= 0; i--) find_step<OPT>(lo, hi, s_m, first_lo, first_hi, (x >> (8 * i)) & 0xffu, q);
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
#pragma unroll
        for (int i = 3; i >= 0; i--) {
            find_step<OPT>(lo, hi, s_m, first_lo, first_hi, (w[j] >> (8 * i)) & 0xffu, q);
            /* (the bytes come last first: the mask is shifted up under each new bit - a bit set by its own constant would
             * keep 25 constants and 32 partial masks in registers, 34 VGPRs more) */
            if constexpr (ALT) m = (m << 1) | dmin<uint32_t>((hi & starts_hi) | (lo & starts_lo), 1u);
            else m |= (hi >> 31) << (4 * j + i);
        }
    }
    const uint32_t mine = find_fit(plen, tsym, lane);
    return mine == 0u ? 0u : (mine < 32u ? m & ((1u << mine) - 1u) : m);
}

/* find_cls_lane<true> with a mask word a TERM: the automaton is the same one, and in the place of "any start bit" the lane
 * asks NT times "a start bit of term t".  NT, the number of terms, is the kernel's at compile time: the masks stay in registers.
 * OPT (the expr call): the step is find_opt_step, as in find_cls_lane<true, true>. */
template <uint32_t NT, bool OPT = false>
__device__ __forceinline__ void find_term_lane(const uint32_t *tile_words, const uint32_t (&w)[8], const uint32_t *s_m, uint32_t first_lo,
                                               uint32_t first_hi, uint32_t plen, uint32_t tsym, uint32_t lane, const FindTerms &tm,
                                               uint32_t (&m)[NT], [[maybe_unused]] const FindOpt *q = nullptr)
{
    uint32_t lo = 0, hi = 0;
    for (uint32_t k = (plen + 2u) >> 2; k-- > 0u;) {                /* the words that hold the plen - 1 bytes behind the lane's */
        const uint32_t x = tile_words[dmin<uint32_t>(8u * lane + 8u + k, HUF_SUB_TILE / 4 - 1u)];
#pragma unroll
        for (int i = 3; i >= 0; i--) find_step<OPT>(lo, hi, s_m, first_lo, first_hi, (x >> (8 * i)) & 0xffu, q);
    }
#pragma unroll
    for (uint32_t t = 0; t < NT; t++) m[t] = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
#pragma unroll
        for (int i = 3; i >= 0; i--) {
            find_step<OPT>(lo, hi, s_m, first_lo, first_hi, (w[j] >> (8 * i)) & 0xffu, q);
#pragma unroll
            for (uint32_t t = 0; t < NT; t++) m[t] = (m[t] << 1) | dmin<uint32_t>((hi & tm.starts[t][1]) | (lo & tm.starts[t][0]), 1u);
        }
    }
    const uint32_t mine = find_fit(plen, tsym, lane);
#pragma unroll
    for (uint32_t t = 0; t < NT; t++) m[t] = mine == 0u ? 0u : (mine < 32u ? m[t] & ((1u << mine) - 1u) : m[t]);
}

/* the body of the seven walk kernels, grid nblocks * cpb, in one piece: the key into LDS, the header, then either the
 * branch of a block of one byte value or the tables and the loop over the chunk's tiles.  PAT = false: the bytes' call, p
 * is not looked at.  REC: r's delimiter masks and counts next to the pattern's work.  CLS: the class table
 * ct in the place of the pattern's bytes.  ALT: ct holds several alternatives, alt says where they start, and p->plen is
 * the longest one's length.  NT != 0 (find_rec_term_sub_kernel): the alternatives stand in NT terms, and what leaves the
 * workgroup is a match mask word a group and a count a tile for every TERM, into tm's term-major arrays, in the place of the one
 * mask and count: the delimiter mask, the edges, the checks and the status are as they are.  OPT (find_opt_sub_kernel,
 * find_rec_opt_sub_kernel): the any-of walk with find_opt_step and q's masks in the place of find_cls_step; with NT
 * (find_rec_term_opt_sub_kernel) the terms' walk with it. */
template <bool PAT, bool REC = false, bool CLS = false, bool ALT = false, uint32_t NT = 0, bool OPT = false>
__device__ __forceinline__ void find_sub_body(const FindArgs &a, const FindPatArgs *p, const FindRecArgs *r = nullptr, const FindClsTable *ct = nullptr,
                                              [[maybe_unused]] const FindAltArgs *alt = nullptr, [[maybe_unused]] const FindTerms *tm = nullptr,
                                              [[maybe_unused]] const FindOpt *q = nullptr)
{
    static_assert(!OPT || ALT, "optional positions: the any-of route's");
    static_assert(PAT || !REC, "the records' route is the pattern's");
    static_assert(NT == 0 || (ALT && REC && NT <= FIND_TERMS_MAX), "the terms' route is the any-of records'");
    static_assert(PAT || !CLS, "the classes' route is the pattern's");
    static_assert(CLS || !ALT, "the alternatives' route is the classes'");
    constexpr uint32_t KEY_WORDS = CLS ? FIND_CLS_WORDS : (PAT ? FIND_PAT_MAX / 4 : 8);      /* the delimiter set lies behind them */
    typedef DsubShared<FIND_THREADS> SH;
    __shared__ SH sh;
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[FIND_WAVES][HUF_SUB_TILE / 4];
    __shared__ alignas(CLS ? 8 : 4) uint32_t s_set[KEY_WORDS + (REC ? 8 : 0)];  /* the set, the pattern or the class table (and the delimiter set behind it) */
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    const uint64_t b = blockIdx.x / a.cpb;
    const uint32_t c = blockIdx.x % a.cpb;
    const uint64_t blen = find_block_len(a, b);
    const uint64_t sym0 = (uint64_t)c * DSUB_CHUNK_SYMS;
    if (sym0 >= blen) return;                                       /* (the short last block has fewer chunks) */
    const uint64_t sym1 = dmin<uint64_t>(blen, sym0 + DSUB_CHUNK_SYMS);
    if constexpr (PAT) {
        if constexpr (CLS) {
            static_assert(FIND_THREADS == FIND_CLS_WORDS, "a thread a word of the table");
            s_set[threadIdx.x] = ct->m[threadIdx.x >> 1][threadIdx.x & 1u];
        } else {
            if (threadIdx.x < FIND_PAT_MAX / 4) s_set[threadIdx.x] = p->pat[threadIdx.x];
        }
        if constexpr (REC) {
            if (threadIdx.x >= 64 && threadIdx.x < 72) s_set[KEY_WORDS + threadIdx.x - 64] = a.set[threadIdx.x - 64];
        }
    } else {
        if (threadIdx.x < 8) s_set[threadIdx.x] = a.set[threadIdx.x];
    }
    __syncthreads();
    /* ---- the header - and its length must be the layout's ---- */
    BlockHeader h;
    if (parse_block_header(a.s.stream, a.s.stream_len, a.s.offsets[b], a.s.offsets[b + 1], a.s.max_tree, h) != HUFE_OK || h.block_len != blen)
        return find_raise(a, b, threadIdx.x == 0);
    const SubBlockView v = sub_block_view(h, a.s.sub, b);
    uint32_t *row = a.bitmap + b * a.wpb;
    uint32_t *trow = a.tcnt + b * a.tpb;
    const int leaf = h.tree_len == 5 ? single_leaf_symbol(h.tree) : -1;
    if (leaf >= 0) {
        /* ---- one byte value: every symbol is a 0 bit (decode.hpp); the chunk's bits are seen to be 0 ---- */
        if (blen > v.pay_bits) return find_raise(a, b, threadIdx.x == 0);
        bool match;
        [[maybe_unused]] bool tmatch[NT ? NT : 1];                  /* NT: ... of at least one alternative of term t */
        uint32_t plen = 1;
        if constexpr (PAT) {
            /* the pattern is plen copies of the leaf, or it starts nowhere in this block; as for other blocks only
             * the starts whose match stays inside its tile are set here, find_seam_kernel has the rest */
            plen = p->plen;
            if constexpr (ALT) {
                /* ... the leaf is in every class of at least ONE alternative: m[leaf] has all of that alternative's bits,
                 * which is what the automaton's start bits say after plen copies of the leaf (after len_j of them
                 * alternative j's start bit is set iff the leaf is in all its classes, and it stays as it is from then on).
                 * The starts of a tile at which the LONGEST alternative fits are set here, as in other blocks;
                 * find_alt_seam_kernel has the rest, alternative by alternative.  OPT: the same question to the automaton
                 * with the closure - the state only grows under copies of one byte, and after plen of them every form has
                 * had its length; find_opt_seam_kernel has the rest. */
                uint32_t lo = 0, hi = 0;
                for (uint32_t k = 0; k < plen; k++) find_step<OPT>(lo, hi, s_set, ct->first[0], ct->first[1], (uint32_t)leaf, q);
                match = ((hi & alt->starts[1]) | (lo & alt->starts[0])) != 0u;
                if constexpr (NT != 0) {
#pragma unroll
                    for (uint32_t k = 0; k < NT; k++) tmatch[k] = ((hi & tm->starts[k][1]) | (lo & tm->starts[k][0])) != 0u;
                }
            } else if constexpr (CLS) {                             /* ... the leaf is in every class, or there is no start */
                match = (s_set[2u * (uint32_t)leaf] & ct->full[0]) == ct->full[0] && (s_set[2u * (uint32_t)leaf + 1u] & ct->full[1]) == ct->full[1];
            } else {
                match = true;
                for (uint32_t k = 0; k < plen; k++) match &= ((s_set[k >> 2] >> (8u * (k & 3u))) & 0xffu) == (uint32_t)leaf;
            }
        } else {
            match = ((s_set[(uint32_t)leaf >> 5] >> ((uint32_t)leaf & 31u)) & 1u) != 0u;
        }
        bool delim = false;                                         /* the leaf is a delimiter (then the pattern is not its copies) */
        if constexpr (REC) delim = ((s_set[KEY_WORDS + ((uint32_t)leaf >> 5)] >> ((uint32_t)leaf & 31u)) & 1u) != 0u;
        bool set = false;
        for (uint64_t g = (sym0 >> 5) + threadIdx.x; 32ull * g < sym1; g += FIND_THREADS) {
            uint32_t nsym = (uint32_t)dmin<uint64_t>(DSUB_SPL, blen - 32ull * g);
            uint32_t x = load_be32(v.pay, 4ull * g, v.pay_bytes);
            if (nsym < 32u) x &= 0xffffffffu << (32u - nsym);
            set |= x != 0u;
            if constexpr (REC) r->dbits[b * a.wpb + g] = delim ? find_low_bits(nsym) : 0u;
            if constexpr (PAT) {                                    /* the starts of this group at which the pattern fits in the tile */
                const uint64_t tend = dmin<uint64_t>(blen, (g / 64u + 1u) * HUF_SUB_TILE), s0 = 32ull * g + plen;
                nsym = s0 > tend ? 0u : (uint32_t)dmin<uint64_t>(DSUB_SPL, tend - s0 + 1u);
            }
            if constexpr (NT != 0) {
#pragma unroll
                for (uint32_t k = 0; k < NT; k++)
                    tm->mbits[k * tm->nwords + b * a.wpb + g] = tmatch[k] ? find_low_bits(nsym) : 0u;
            } else {
                row[g] = match ? find_low_bits(nsym) : 0u;
            }
        }
        for (uint64_t t = sym0 / HUF_SUB_TILE + threadIdx.x; t * HUF_SUB_TILE < sym1; t += FIND_THREADS) {
            const uint32_t tsym = find_tile_syms(blen, t);
            if constexpr (NT != 0) {
#pragma unroll
                for (uint32_t k = 0; k < NT; k++)
                    tm->mcnt[k * a.ntiles + b * a.tpb + t] = tmatch[k] ? (tsym >= plen ? tsym - plen + 1u : 0u) : 0u;
            } else {
                trow[t] = match ? (tsym >= plen ? tsym - plen + 1u : 0u) : 0u;
            }
            if constexpr (REC) r->dcnt[b * a.tpb + t] = delim ? tsym : 0u;
        }
        if constexpr (PAT) {                                        /* the tiles' edges: the leaf */
            const uint64_t t0 = sym0 / HUF_SUB_TILE, nt = (sym1 - sym0 + HUF_SUB_TILE - 1) / HUF_SUB_TILE;
            for (uint64_t i = threadIdx.x; i < nt * FIND_EDGE_SLOT; i += FIND_THREADS) {
                const uint64_t t = t0 + i / FIND_EDGE_SLOT;
                const uint32_t tsym = find_tile_syms(blen, t);
                if (((uint32_t)i & 63u) < dmin<uint32_t>(tsym, plen - 1u))
                    p->edges[(b * a.tpb + t0) * FIND_EDGE_SLOT + i] = (uint8_t)leaf;
            }
        }
        return find_raise(a, b, set);
    }
    /* ---- the block's tables ---- */
    const DsubTreeWords tw = dsub_tree_request<FIND_THREADS>(h.tree, h.tree_len, a.s.sub.lens + b * HUF_NSYM);
    if (!dsub_fast_tables<FIND_THREADS>(sh, h.tree_len, tw)) return find_raise(a, b, threadIdx.x == 0);     /* (workgroup-uniform) */
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
        if constexpr (PAT) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   /* the lanes' bytes are in LDS before other lanes read them */
            __builtin_amdgcn_wave_barrier();
        }
        /* the lane's own 32 bytes (it wrote them itself) against the set */
        const uint4 lo4 = *reinterpret_cast<const uint4 *>(tile_words + 8u * lane);
        const uint4 hi4 = *reinterpret_cast<const uint4 *>(tile_words + 8u * lane + 4u);
        const uint32_t w[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
        uint32_t m = 0;
        [[maybe_unused]] uint32_t mt[NT ? NT : 1];
        if constexpr (PAT) {
            const uint32_t tsym = find_tile_syms(blen, t), plen = p->plen;
            if constexpr (NT != 0) find_term_lane<NT, OPT>(tile_words, w, s_set, ct->first[0], ct->first[1], plen, tsym, lane, *tm, mt, q);
            else if constexpr (OPT) m = find_cls_lane<true, true>(tile_words, w, s_set, ct->first[0], ct->first[1], plen, tsym, lane, alt->starts[0], alt->starts[1], q);
            else if constexpr (ALT) m = find_cls_lane<true>(tile_words, w, s_set, ct->first[0], ct->first[1], plen, tsym, lane, alt->starts[0], alt->starts[1]);
            else if constexpr (CLS) m = find_cls_lane(tile_words, w, s_set, ct->first[0], ct->first[1], plen, tsym, lane);
            else m = find_pat_lane(tile_words, w, s_set, plen, tsym, lane);         /* (0 for a lane without symbols) */
            /* the edges: the tile's first and last min(tsym, plen - 1) bytes */
            const uint32_t ne = dmin<uint32_t>(tsym, plen - 1u);
            uint8_t *slot = p->edges + (b * a.tpb + t) * FIND_EDGE_SLOT;
            const uint8_t *bytes = reinterpret_cast<const uint8_t *>(tile_words);
            if (lane < ne) {
                slot[lane] = bytes[lane];
                slot[64u + lane] = bytes[tsym - ne + lane];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   /* ... and read before the next tile overwrites them */
            __builtin_amdgcn_wave_barrier();
            if constexpr (REC) {                                    /* the lane's own 32 bytes against the delimiter set */
                uint32_t d = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t x = (w[j] >> (8 * i)) & 0xffu;
                        d |= ((s_set[KEY_WORDS + (x >> 5)] >> (x & 31u)) & 1u) << (4 * j + i);
                    }
                }
                d = nsym == 0u ? 0u : (nsym < 32u ? d & ((1u << nsym) - 1u) : d);
                if (nsym != 0u) r->dbits[b * a.wpb + t * 64u + lane] = d;
                const uint32_t dc = wave_total_u32((uint32_t)__popc(d));
                if (lane == 0) r->dcnt[b * a.tpb + t] = dc;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t x = (w[j] >> (8 * i)) & 0xffu;
                    m |= ((s_set[x >> 5] >> (x & 31u)) & 1u) << (4 * j + i);
                }
            }
            m = nsym == 0u ? 0u : (nsym < 32u ? m & ((1u << nsym) - 1u) : m);    /* (bytes behind a short group are stale) */
        }
        if constexpr (NT != 0) {
#pragma unroll
            for (uint32_t k = 0; k < NT; k++) {
                if (nsym != 0u) tm->mbits[k * tm->nwords + b * a.wpb + t * 64u + lane] = mt[k];
                const uint32_t cnt = wave_total_u32((uint32_t)__popc(mt[k]));
                if (lane == 0) tm->mcnt[k * a.ntiles + b * a.tpb + t] = cnt;
            }
        } else {
            if (nsym != 0u) row[t * 64u + lane] = m;
            const uint32_t cnt = wave_total_u32((uint32_t)__popc(m));
            if (lane == 0) trow[t] = cnt;
        }
    }
    find_raise(a, b, !good && lane == 0);
}

__global__ __launch_bounds__(FIND_THREADS) void find_sub_kernel(FindArgs a) { find_sub_body<false>(a, nullptr); }
__global__ __launch_bounds__(FIND_THREADS) void find_pat_sub_kernel(FindPatArgs a) { find_sub_body<true>(a.f, &a); }
__global__ __launch_bounds__(FIND_THREADS) void find_rec_sub_kernel(FindRecArgs a) { find_sub_body<true, true>(a.p.f, &a.p, &a); }
__global__ __launch_bounds__(FIND_THREADS) void find_cls_sub_kernel(FindClsArgs a) { find_sub_body<true, false, true>(a.r.p.f, &a.r.p, nullptr, &a.t); }
__global__ __launch_bounds__(FIND_THREADS) void find_rec_cls_sub_kernel(FindClsArgs a) { find_sub_body<true, true, true>(a.r.p.f, &a.r.p, &a.r, &a.t); }
__global__ __launch_bounds__(FIND_THREADS) void find_alt_sub_kernel(FindAltArgs a) { find_sub_body<true, false, true, true>(a.r.p.f, &a.r.p, nullptr, &a.t, &a); }
__global__ __launch_bounds__(FIND_THREADS) void find_rec_alt_sub_kernel(FindAltArgs a) { find_sub_body<true, true, true, true>(a.r.p.f, &a.r.p, &a.r, &a.t, &a); }
/* hufgpu_find_any_quant / hufgpu_find_records_quant with an optional position */
__global__ __launch_bounds__(FIND_THREADS) void find_opt_sub_kernel(FindOptArgs a)
{
    find_sub_body<true, false, true, true, 0, true>(a.a.r.p.f, &a.a.r.p, nullptr, &a.a.t, &a.a, nullptr, &a.q);
}
__global__ __launch_bounds__(FIND_THREADS) void find_rec_opt_sub_kernel(FindOptArgs a)
{
    find_sub_body<true, true, true, true, 0, true>(a.a.r.p.f, &a.a.r.p, &a.a.r, &a.a.t, &a.a, nullptr, &a.q);
}
/* hufgpu_find_records_terms with two terms or more: NT is the call's n_terms, a kernel each */
template <uint32_t NT>
__global__ __launch_bounds__(FIND_THREADS) void find_rec_term_sub_kernel(FindTermArgs ta)
{
    find_sub_body<true, true, true, true, NT>(ta.a.r.p.f, &ta.a.r.p, &ta.a.r, &ta.a.t, &ta.a, &ta.t);
}

/* hufgpu_find_records_expr with two terms or more and an optional position or an anchor: the terms' walk with the closure */
template <uint32_t NT>
__global__ __launch_bounds__(FIND_THREADS) void find_rec_term_opt_sub_kernel(FindExprArgs xa)
{
    find_sub_body<true, true, true, true, NT, true>(xa.qa.a.r.p.f, &xa.qa.a.r.p, &xa.qa.a.r, &xa.qa.a.t, &xa.qa.a, &xa.t, &xa.qa.q);
}

/* ---- the seams: the matches that leave their tile (launched for plen >= 2 only) ---------------------------------------- */

/* a seam kernel's lane: the tile, and one of its last ne = min(symbols, plen - 1) starts - s in the tile, pos in the data.
 * The lanes from ne on have no start. */
struct FindSeam {
    uint64_t i;
    FindTile k;
    uint32_t lane, ne, s;
    uint64_t pos;
};

/* the pattern (or CLS: the class table c) into the workgroup's s_key */
template <bool CLS>
__device__ __forceinline__ void find_seam_key(const FindPatArgs &pa, const FindClsTable *c, uint32_t *s_key)
{
    if constexpr (CLS) {
        for (uint32_t i = threadIdx.x; i < FIND_CLS_WORDS; i += FIND_SEAM_THREADS) s_key[i] = c->m[i >> 1][i & 1u];
    } else {
        if (threadIdx.x < FIND_PAT_MAX / 4) s_key[threadIdx.x] = pa.pat[threadIdx.x];
    }
    __syncthreads();
}

/* the lane's start in tile i = k (which the layout has, in a block that is served: another one counts nothing) */
__device__ __forceinline__ FindSeam find_seam_lane(const FindPatArgs &pa, uint64_t i, const FindTile &k)
{
    const uint32_t lane = (uint32_t)lane_id(), tsym = find_tile_syms(k.blen, k.t);
    const uint32_t ne = dmin<uint32_t>(tsym, pa.plen - 1u), s = tsym - ne + lane;
    return {i, k, lane, ne, s, k.b * pa.f.s.bsize + k.t * HUF_SUB_TILE + s};
}

/* Do the len bytes from the lane's start (lane < ne) match - the pattern's bytes in s_key, or CLS: byte k against the bit
 * hi - k of its entry of the table in s_key - without ending behind raw_size, and is every block they touch served?  Byte k
 * comes from the tile's own tail slot, then from the heads of the tiles behind: THE walk over the layout's tile lengths. */
template <bool CLS>
__device__ __forceinline__ bool find_seam_candidate(const FindPatArgs &pa, const uint32_t *s_key, const FindSeam &m, uint32_t len,
                                                    [[maybe_unused]] uint32_t hi = 63u)
{
    const FindArgs &a = pa.f;
    if (m.pos + len > a.s.raw_size) return false;
    const uint8_t *e = pa.edges + m.i * FIND_EDGE_SLOT + 64u;     /* the own tail, then the heads of the tiles behind */
    uint64_t cb = m.k.b, ct = m.k.t, cblen = m.k.blen;
    uint32_t off = m.lane, csym = m.ne;                             /* byte k is e[off]; csym bytes there belong to this tile */
    [[maybe_unused]] uint32_t kbit = 1u << (hi & 31u), khalf = (hi >> 5) & 1u;      /* CLS: class k is bit kbit of half khalf of a table entry */
    for (uint32_t k = 0; k < len; k++, off++) {
        while (off == csym) {                                       /* on into the next tile of the layout */
            if ((ct + 1) * HUF_SUB_TILE < cblen) {
                ct++;
            } else {
                cb++;                                               /* (pos + len <= raw_size: there is such a block) */
                ct = 0;
                cblen = find_block_len(a, cb);
                if (a.errs[cb] != HUFE_OK) return false;
            }
            e = pa.edges + (cb * a.tpb + ct) * FIND_EDGE_SLOT;
            off = 0;
            csym = find_tile_syms(cblen, ct);
        }
        if constexpr (CLS) {
            if ((s_key[2u * e[off] + khalf] & kbit) == 0u) return false;
            kbit >>= 1;                                             /* class k + 1: the next bit down, shifted by a constant */
            if (kbit == 0u) {
                kbit = 0x80000000u;
                khalf = 0u;
            }
        } else {
            if (e[off] != ((s_key[k >> 2] >> (8u * (k & 3u))) & 0xffu)) return false;
        }
    }
    return true;
}

/* the starts that were found, into the tile's mask words and its count: before the scan */
__device__ __forceinline__ void find_seam_end(const FindArgs &a, const FindSeam &m, bool hit)
{
    if (hit) atomicOr(&a.bitmap[m.k.b * a.wpb + m.k.t * 64u + (m.s >> 5)], 1u << (m.s & 31u));
    const uint32_t cnt = (uint32_t)__popcll(__ballot(hit));
    if (m.lane == 0 && cnt != 0u) a.tcnt[m.i] += cnt;
}

template <bool CLS>
__device__ __forceinline__ void find_seam_body(const FindPatArgs &pa, const FindClsTable *c = nullptr)
{
    __shared__ uint32_t s_key[CLS ? FIND_CLS_WORDS : FIND_PAT_MAX / 4];
    find_seam_key<CLS>(pa, c, s_key);
    const uint64_t i = find_tile_index<FIND_SEAM_THREADS>();
    if (i >= pa.f.ntiles) return;
    const FindTile tl = find_tile(pa.f, i);
    if (tl.t * HUF_SUB_TILE >= tl.blen || pa.f.errs[tl.b] != HUFE_OK) return;
    const FindSeam m = find_seam_lane(pa, i, tl);
    find_seam_end(pa.f, m, m.lane < m.ne && find_seam_candidate<CLS>(pa, s_key, m, pa.plen));
}

__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_seam_kernel(FindPatArgs pa) { find_seam_body<false>(pa); }
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_cls_seam_kernel(FindClsArgs a) { find_seam_body<true>(a.r.p, &a.t); }

/* hufgpu_find_any: plen is the LONGEST alternative's length, and the tile's last plen - 1 starts are this kernel's for
 * EVERY alternative, a short one that ends inside the tile included: the tile's tail slot holds all the bytes it needs.
 * The wave goes through the alternatives together (hi_j and len_j are the wave's, in scalar registers); a lane takes part
 * until one alternative lies at its start, and then sets ONE bit and counts ONE match. */
/* find_anc_seam_kernel: the positions to ask for of an alternative of `len`, its boundary position included - without that
 * one when the data ends where the boundary byte would lie */
__device__ __forceinline__ uint32_t find_anc_len(const FindArgs &a, const FindSeam &m, uint32_t len)
{
    return m.pos + len == a.s.raw_size + 1u ? len - 1u : len;
}

template <bool ANC>
__device__ __forceinline__ void find_alt_seam_body(const FindAltArgs &aa)
{
    __shared__ uint32_t s_key[FIND_CLS_WORDS];
    __shared__ uint32_t s_hl[FIND_PAT_MAX];
    const FindPatArgs &pa = aa.r.p;
    if (threadIdx.x < FIND_PAT_MAX) s_hl[threadIdx.x] = aa.hl[threadIdx.x];
    find_seam_key<true>(pa, &aa.t, s_key);
    const uint64_t i = find_tile_index<FIND_SEAM_THREADS>();
    if (i >= pa.f.ntiles) return;
    const FindTile tl = find_tile(pa.f, i);
    if (tl.t * HUF_SUB_TILE >= tl.blen || pa.f.errs[tl.b] != HUFE_OK) return;
    const FindSeam m = find_seam_lane(pa, i, tl);
    /* the byte AT the start, read once: an alternative whose first class does not hold it starts no walk, so a lane
     * that no alternative can start at - nearly every lane - costs this one load however many alternatives there are */
    const uint32_t at = m.lane < m.ne ? pa.edges[m.i * FIND_EDGE_SLOT + 64u + m.lane] : 0u;
    const uint32_t m0 = s_key[2u * at], m1 = s_key[2u * at + 1u];
    bool hit = false;
    for (uint32_t j = 0; j < aa.n_alts; j++) {
        const uint32_t hl = uni32(s_hl[j]), hi = hl & 63u;
        if (m.lane < m.ne && !hit && ((((hi >> 5) ? m1 : m0) >> (hi & 31u)) & 1u) != 0u)
            hit = find_seam_candidate<true>(pa, s_key, m, ANC ? find_anc_len(pa.f, m, hl >> 8) : hl >> 8, hi);
    }
    find_seam_end(pa.f, m, hit);
}
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_alt_seam_kernel(FindAltArgs aa) { find_alt_seam_body<false>(aa); }

/* The anchored calls with HUFGPU_ANCHOR_EOL or HUFGPU_ANCHOR_WORD: every alternative ends with one position more, the class
 * of the bytes that may stand BEHIND a match, so the walk and the kernel above need not know of anchors - but for the match
 * that ends where the data ends: there is no byte to look up, and nothing behind the data stands in the way.  That start
 * lies among the last plen - 1 of its tile (plen - 1 is the longest alternative's own length now), so it is this kernel's:
 * an alternative whose boundary position would be the byte AT raw_size is asked for without it (len_j >= 1 positions are
 * left).  Every other start is find_alt_seam_kernel's word for word. */
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_anc_seam_kernel(FindAltArgs aa) { find_alt_seam_body<true>(aa); }

/* hufgpu_find_records_terms: find_alt_seam_kernel with a hit a TERM.  A lane goes through the alternatives as there, each
 * with its own seam rule, and an alternative is asked for until ITS term has a hit at the lane's start; then find_seam_end
 * once a term, into that term's mask words and counts. */
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_term_seam_kernel(FindTermArgs ta)
{
    __shared__ uint32_t s_key[FIND_CLS_WORDS];
    __shared__ uint32_t s_hl[FIND_PAT_MAX];
    const FindAltArgs &aa = ta.a;
    const FindPatArgs &pa = aa.r.p;
    if (threadIdx.x < FIND_PAT_MAX) s_hl[threadIdx.x] = aa.hl[threadIdx.x];
    find_seam_key<true>(pa, &aa.t, s_key);
    const uint64_t i = find_tile_index<FIND_SEAM_THREADS>();
    if (i >= pa.f.ntiles) return;
    const FindTile tl = find_tile(pa.f, i);
    if (tl.t * HUF_SUB_TILE >= tl.blen || pa.f.errs[tl.b] != HUFE_OK) return;
    const FindSeam m = find_seam_lane(pa, i, tl);
    const uint32_t at = m.lane < m.ne ? pa.edges[m.i * FIND_EDGE_SLOT + 64u + m.lane] : 0u;     /* the byte AT the start, read once */
    const uint32_t m0 = s_key[2u * at], m1 = s_key[2u * at + 1u];
    uint32_t hits = 0;                                              /* bit t: an alternative of term t lies at the lane's start */
    for (uint32_t j = 0; j < aa.n_alts; j++) {
        const uint32_t hl = uni32(s_hl[j]), hi = hl & 63u, term = (hl >> 6) & 3u;
        if (m.lane < m.ne && ((hits >> term) & 1u) == 0u && ((((hi >> 5) ? m1 : m0) >> (hi & 31u)) & 1u) != 0u)
            hits |= (uint32_t)find_seam_candidate<true>(pa, s_key, m, hl >> 8, hi) << term;
    }
    for (uint32_t t = 0; t < ta.t.n_terms; t++) {
        FindArgs f = pa.f;
        f.bitmap = ta.t.mbits + t * ta.t.nwords;
        f.tcnt = ta.t.mcnt + t * pa.f.ntiles;
        find_seam_end(f, m, ((hits >> t) & 1u) != 0u);
    }
}

/* hufgpu_find_any_quant: the tile's last plen - 1 starts (plen: the longest alternative's position count) for every form of
 * every alternative.  A form's length is not known in advance, so "byte k against bit hi - k" does not carry over.  What
 * does: let e be the end of the bytes within [p, p + plen) that exist and lie in served blocks; the automaton of the walk, run
 * with an empty state from byte e - 1 down to byte p, has a start bit set behind byte p iff a form lies at p that ends at or
 * in front of e - the shortest form that lies there decides, as its span is the one that touches the fewest blocks.
 * The wave copies its window once - the tile's tail slot, then the heads of the tiles behind it over the layout's tile
 * lengths, up to raw_size or the first block that is not served: at most 63 + 63 bytes, `filled` of them - into LDS, and
 * every lane runs its at most plen steps on LDS bytes.  One bit and one count a start through find_seam_end. */
template <bool SEED, bool TERMS>
__device__ __forceinline__ void find_win_seam_body(const FindOptArgs &qa, [[maybe_unused]] const uint32_t *bnd = nullptr,
                                                   [[maybe_unused]] const FindTerms *tm = nullptr)
{
    __shared__ uint32_t s_key[FIND_CLS_WORDS];
    __shared__ uint8_t s_win[FIND_SEAM_THREADS / 64][FIND_EDGE_SLOT];
    const FindAltArgs &aa = qa.a;
    const FindPatArgs &pa = aa.r.p;
    const FindArgs &a = pa.f;
    find_seam_key<true>(pa, &aa.t, s_key);
    const uint64_t i = find_tile_index<FIND_SEAM_THREADS>();
    if (i >= a.ntiles) return;
    const FindTile tl = find_tile(a, i);
    if (tl.t * HUF_SUB_TILE >= tl.blen || a.errs[tl.b] != HUFE_OK) return;
    const FindSeam m = find_seam_lane(pa, i, tl);
    uint8_t *win = s_win[uni32(threadIdx.x >> 6)];
    if (m.lane < m.ne) win[m.lane] = pa.edges[i * FIND_EDGE_SLOT + 64u + m.lane];
    const uint32_t want = m.ne + pa.plen - 1u;                      /* the last start's bytes end here: at most 126 */
    uint32_t filled = m.ne;
    uint64_t cb = tl.b, ct = tl.t, cblen = tl.blen;
    while (filled < want) {                                         /* (the wave's: a tile of the layout a round, a byte at least) */
        if ((ct + 1) * HUF_SUB_TILE < cblen) {
            ct++;
        } else {
            cb++;
            ct = 0;
            if (cb >= a.s.nblocks || a.errs[cb] != HUFE_OK) break;  /* the data ends, or a block is not served: e */
            cblen = find_block_len(a, cb);
        }
        const uint32_t n = dmin<uint32_t>(find_tile_syms(cblen, ct), want - filled);    /* (<= plen - 1: the head slot holds them) */
        if (m.lane < n) win[filled + m.lane] = pa.edges[(cb * a.tpb + ct) * FIND_EDGE_SLOT + m.lane];
        filled += n;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");           /* the window is in LDS before other lanes read it */
    __builtin_amdgcn_wave_barrier();
    uint32_t lo = 0, hi = 0;
    if (m.lane < m.ne) {
        if constexpr (SEED) {
            /* The window ends where the DATA ends - not at a block that is not served, which lies in front of raw_size, and
             * not at `want` short of it - and the lane's scan begins there: a form that ends at raw_size has nothing behind
             * it, which meets its boundary position.  So the scan starts from "the boundary positions are met", closed over
             * the optional positions in front of them (a form may leave those out), in the place of the empty state.  A seed
             * bit stands for a boundary position and for optional positions that a form drops: for no byte.  Every position
             * above them is reached by find_opt_step alone, one byte of the window each, and the window holds no byte from
             * raw_size on - so no form that needs a byte behind the data gets its start bit. */
            const uint64_t wend = m.pos - m.lane + filled;          /* (m.pos - m.lane: the window's first byte) */
            if (wend == a.s.raw_size && m.lane + pa.plen > filled) {
                lo = bnd[0];
                hi = bnd[1];
                find_opt_close(lo, hi, qa.q);
            }
        }
        for (uint32_t k = dmin<uint32_t>(m.lane + pa.plen, filled); k-- > m.lane;)
            find_opt_step(lo, hi, s_key, aa.t.first[0], aa.t.first[1], win[k], qa.q);
    }
    if constexpr (TERMS) {                                          /* a hit a term, read off the term's start bits */
        for (uint32_t t = 0; t < tm->n_terms; t++) {
            FindArgs f = a;
            f.bitmap = tm->mbits + t * tm->nwords;
            f.tcnt = tm->mcnt + t * a.ntiles;
            find_seam_end(f, m, ((hi & tm->starts[t][1]) | (lo & tm->starts[t][0])) != 0u);
        }
    } else {
        find_seam_end(a, m, ((hi & aa.starts[1]) | (lo & aa.starts[0])) != 0u);
    }
}
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_opt_seam_kernel(FindOptArgs qa) { find_win_seam_body<false, false>(qa); }

/* The expr calls' seam kernels: find_opt_seam_kernel's window, with the end of the data as a boundary (SEED, above) - a
 * form that ends exactly at raw_size has its start among its tile's last plen - 1, as plen counts the boundary position -
 * and, for two terms or more, find_term_seam_kernel in window form: the automaton runs ONCE a lane whatever the number of
 * alternatives, and find_seam_end runs once a term. */
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_opt_anc_seam_kernel(FindExprArgs xa) { find_win_seam_body<true, false>(xa.qa, xa.bnd); }
__global__ __launch_bounds__(FIND_SEAM_THREADS) void find_term_opt_seam_kernel(FindExprArgs xa) { find_win_seam_body<true, true>(xa.qa, xa.bnd, &xa.t); }

/* The anchored calls with HUFGPU_ANCHOR_BOL or HUFGPU_ANCHOR_WORD, behind the seam kernel and in front of everything that
 * reads the match mask: a wave = one tile, a lane = one word.  `bound` is a mask of the walk's, a bit a byte: may this byte
 * stand in FRONT of a match - the delimiters' mask for BOL in a records call, for WORD there the mask that find_sub_kernel
 * writes in a second walk with that set (a records walk has room for ONE set next to the table, and the record kernels need
 * the delimiters' there), and for the positions call the records' walk's "delimiter" mask, written with the boundary set in the place
 * of the delimiters.  A start stays when the byte in front of it is one of those: m &= (bound << 1) | carry, the carry being
 * the bit of the symbol in front of the lane's word - the lane below's, and for lane 0 the last symbol of the tile in front
 * (a full one), for a block's first tile that of block b - 1 (a full block; its row ends where it ends), 1 at byte 0, where
 * nothing stands in front, and 0 when block b - 1 is not served: left out on doubt.  Then the tile's count anew: nobody else
 * writes tcnt behind the seam kernel.  A tile without a start, or of a block that is not served, is left as it is. */
struct FindAnchorArgs {
    FindArgs f;
    const uint32_t *bound;                  /* [nblocks][wpb] */
};
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_anchor_kernel(FindAnchorArgs aa)
{
    const FindArgs &a = aa.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK || a.tcnt[i] == 0u) return;
    const uint64_t g = t * 64u + lane;
    const bool inside = g * DSUB_SPL < blen;
    const uint32_t w = inside ? aa.bound[b * a.wpb + g] : 0u;
    uint32_t c0;                                                    /* may the byte in front of the tile stand there (the wave's) */
    if (i == 0) {
        c0 = 1u;
    } else if (t != 0) {
        c0 = aa.bound[b * a.wpb + t * 64u - 1u] >> 31;              /* (the tile in front is a full one) */
    } else if (a.errs[b - 1] != HUFE_OK) {
        c0 = 0u;
    } else {
        const uint64_t last = a.s.bsize - 1u;                       /* (a block with a block behind it is a full one) */
        c0 = (aa.bound[(b - 1) * a.wpb + (last >> 5)] >> ((uint32_t)last & 31u)) & 1u;
    }
    const uint32_t below = wave_up1_u32(w);                         /* (by every lane: a lane that sits out of a DPP move is not read) */
    const uint32_t carry = lane == 0 ? c0 : below >> 31;
    uint32_t *word = a.bitmap + b * a.wpb + g;
    const uint32_t m = inside ? *word & ((w << 1) | carry) : 0u;
    if (inside) *word = m;
    const uint32_t cnt = wave_total_u32((uint32_t)__popc(m));
    if (lane == 0) a.tcnt[i] = cnt;
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
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
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

/* ---- hufgpu_find_any_spans: where the longest form at every reported start ends ------------------------------------- */

/* Behind the expr call's whole chain.  The walk's automaton runs over the REVERSED pattern and sees a match at its start, so
 * no end is in its state; this one runs FORWARD from a start.  qa holds the forward table: find_alt_table and find_opt_masks
 * over every alternative's positions in REVERSE order, so that find_cls_step's shift moves from a position to the NEXT one
 * and find_opt_close leaves out the optional positions that FOLLOW.  Its t.first are then the positions that may hold a
 * form's FIRST byte - the seed, used once -, its `starts` the bit of every alternative's last position: set behind the
 * closure, a form ends with this byte.  The table has no boundary position: with `behind` bit 0 of an entry's low half says
 * "this byte may stand behind a form" (with EOL / WORD the positions sum to at most 63, so bit 63 ... 1 hold them), and a form
 * that ends with the data has nothing behind it.  qa.a.r.p is the call's own: f as scan and finish left it (the final
 * mask, the tile counts, the scan), the edges, and plen - the longest form's bytes, + 1 with `behind`: no start reads more. */
struct FindSpanArgs {
    FindOptArgs qa;
    uint32_t behind;                        /* is the byte behind a form tested (EOL / WORD) */
    uint32_t *len;                          /* [pos_cap] */
    uint8_t *open;                          /* [pos_cap], optional */
};
static_assert(sizeof(FindSpanArgs) <= 4096, "a kernel's arguments end at 4 KiB");

#define FIND_SPAN_END 256u                  /* find_span_next: the data ends here */
#define FIND_SPAN_OPEN 257u                 /* ... or a block that is not served begins */

/* the bytes behind a tile's end, one at a time: the head slots of the tiles behind it, by find_seam_candidate's walk over
 * the layout's tile lengths.  A start reads at most plen - 1 of them, so never more than a head slot holds. */
struct FindSpanTail {
    uint64_t cb, ct, cblen;
    const uint8_t *e;
    uint32_t off, csym;                     /* the next byte is e[off]; csym bytes there belong to tile (cb, ct) */
};
__device__ __forceinline__ uint32_t find_span_next(const FindPatArgs &pa, FindSpanTail &w)
{
    const FindArgs &a = pa.f;
    while (w.off == w.csym) {
        if ((w.ct + 1) * HUF_SUB_TILE < w.cblen) {
            w.ct++;
        } else {
            w.cb++;
            w.ct = 0;
            if (w.cb >= a.s.nblocks) return FIND_SPAN_END;
            if (a.errs[w.cb] != HUFE_OK) return FIND_SPAN_OPEN;
            w.cblen = find_block_len(a, w.cb);
        }
        w.e = pa.edges + (w.cb * a.tpb + w.ct) * FIND_EDGE_SLOT;
        w.off = 0;
        w.csym = find_tile_syms(w.cblen, w.ct);
    }
    return w.e[w.off++];
}

/* The longest qualifying form at start s of the wave's decoded tile (tsym bytes in `bytes`, tile t of block b), and whether a
 * longer one could not be ruled out.  Seeded once; a step clears the last positions' bits first, so that no bit leaves its
 * alternative for the one above (the walk's automaton sets that bit anyway, this one must not).  `pending`: a form ended
 * with the byte before and waits for the byte behind it.  The loop ends when nothing is alive and nothing waits, at the end
 * of the data - which qualifies what waits -, at a block that is not served - which leaves the span open when anything is
 * alive or waits -, and after plen bytes at the latest. */
__device__ __forceinline__ uint32_t find_span_one(const FindSpanArgs &sa, const uint32_t *s_m, const uint8_t *bytes, uint32_t tsym, uint64_t b,
                                                  uint64_t t, uint64_t blen, uint32_t s, bool &open)
{
    const FindAltArgs &aa = sa.qa.a;
    const FindPatArgs &pa = aa.r.p;
    const uint32_t slo = aa.starts[0], shi = aa.starts[1];
    FindSpanTail w = {b, t, blen, nullptr, 0u, 0u};
    uint32_t lo = 0, hi = 0, flo = aa.t.first[0], fhi = aa.t.first[1], len = 0;
    bool pending = false;
    open = false;
    for (uint32_t k = 0; k < pa.plen; k++) {
        const uint32_t x = s + k < tsym ? (uint32_t)bytes[s + k] : find_span_next(pa, w);
        if (x >= FIND_SPAN_END) {
            if (x == FIND_SPAN_END) len = pending ? k : len;
            else open = pending || ((lo & ~slo) | (hi & ~shi)) != 0u;
            break;
        }
        if (pending && (s_m[2u * x] & 1u) != 0u) len = k;
        lo &= ~slo;
        hi &= ~shi;
        find_opt_step(lo, hi, s_m, flo, fhi, x, sa.qa.q);
        flo = fhi = 0u;
        const bool acc = ((lo & slo) | (hi & shi)) != 0u;
        if (acc && sa.behind == 0u) len = k + 1u;
        pending = acc && sa.behind != 0u;
        if (!pending && ((lo & ~slo) | (hi & ~shi)) == 0u) break;
    }
    return len;
}

/* The walk's geometry - a workgroup = one (block, chunk), a wave takes tiles - for the tiles that hold a start below pos_cap
 * only: a chunk of a block that is not served, without a start or behind the cap leaves before it builds tables.  Such a tile
 * is decoded once more into the wave's LDS slice with the checked item of sub_tile.hpp (the walk of this same call has passed
 * it already; no bound of an access here rests on that), a block of one byte value is copies of its leaf.  Then a lane takes the set bits
 * of its word of the FINAL start mask - behind the seam and anchor kernels -, one automaton run each: up to 32 starts of up to
 * plen steps a lane ('a{1,64}' over a run of 'a').  Length and flag go to the tile's rank + the rank inside the tile, as
 * find_emit_kernel numbers the starts; the open spans are counted into d_totals[3], one atomic a wave. */
__global__ __launch_bounds__(FIND_THREADS) void find_span_kernel(FindSpanArgs sa)
{
    typedef DsubShared<FIND_THREADS> SH;
    __shared__ SH sh;
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[FIND_WAVES][HUF_SUB_TILE / 4];
    __shared__ alignas(8) uint32_t s_m[FIND_CLS_WORDS];
    const FindPatArgs &pa = sa.qa.a.r.p;
    const FindArgs &a = pa.f;
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    const uint64_t b = blockIdx.x / a.cpb;
    const uint32_t c = blockIdx.x % a.cpb;
    const uint64_t blen = find_block_len(a, b);
    const uint64_t sym0 = (uint64_t)c * DSUB_CHUNK_SYMS;
    if (sym0 >= blen || a.errs[b] != HUFE_OK) return;
    const uint64_t sym1 = dmin<uint64_t>(blen, sym0 + DSUB_CHUNK_SYMS);
    const uint64_t t0 = sym0 / HUF_SUB_TILE;
    const uint32_t nt = (uint32_t)((sym1 - sym0 + HUF_SUB_TILE - 1) / HUF_SUB_TILE);
    static_assert(DSUB_CHUNK_SYMS / HUF_SUB_TILE <= 64, "a lane a tile of the chunk");
    /* (every wave asks for the whole chunk, so the answer is the workgroup's) */
    if (__ballot(lane < nt && a.tcnt[b * a.tpb + t0 + lane] != 0u) == 0ull) return;
    if (two_level_prefix(a.scan, b * a.tpb + t0) >= a.pos_cap) return;
    static_assert(FIND_THREADS == FIND_CLS_WORDS, "a thread a word of the table");
    s_m[threadIdx.x] = sa.qa.a.t.m[threadIdx.x >> 1][threadIdx.x & 1u];
    __syncthreads();
    BlockHeader h;
    if (parse_block_header(a.s.stream, a.s.stream_len, a.s.offsets[b], a.s.offsets[b + 1], a.s.max_tree, h) != HUFE_OK || h.block_len != blen)
        return;                                                     /* (the walk has seen it parse) */
    const SubBlockView v = sub_block_view(h, a.s.sub, b);
    const int leaf = h.tree_len == 5 ? single_leaf_symbol(h.tree) : -1;
    uint32_t *tile_words = s_tile[wave];
    uint32_t *top = nullptr;
    if (leaf >= 0) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) tile_words[8u * lane + j] = 0x01010101u * (uint32_t)leaf;
    } else {
        const DsubTreeWords tw = dsub_tree_request<FIND_THREADS>(h.tree, h.tree_len, a.s.sub.lens + b * HUF_NSYM);
        if (!dsub_fast_tables<FIND_THREADS>(sh, h.tree_len, tw)) return;    /* (workgroup-uniform) */
        top = DsubLds<FIND_THREADS>::slice(sh, (int)wave) + (SH::SLICE_WORDS - 1u);
    }
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(tile_words);
    uint32_t nopen = 0;
    for (uint64_t t = t0 + wave; t * HUF_SUB_TILE < sym1; t += FIND_WAVES) {
        const uint64_t i = b * a.tpb + t;
        if (a.tcnt[i] == 0u) continue;                              /* (the wave's) */
        const uint64_t rank0 = two_level_prefix(a.scan, i);
        if (rank0 >= a.pos_cap) continue;
        if (leaf < 0) {
            uint32_t nsym;
            /* (a tile that fails here has failed in the walk of this call, which read the same words: its block is not
             * served and the exit above has taken it.  Memory safety rests on the checks; that every rank below
             * d_totals[1] gets its length rests on the walk's verdict being this one) */
            if (!sub_tile_checked<FIND_THREADS>(sh, top, v, t, reinterpret_cast<uint8_t *>(tile_words), nsym)) continue;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       /* the lanes' bytes are in LDS before other lanes read them */
        __builtin_amdgcn_wave_barrier();
        const uint32_t tsym = find_tile_syms(blen, t);
        const uint64_t g = t * 64u + lane;
        uint32_t m = g * DSUB_SPL < blen ? a.bitmap[b * a.wpb + g] : 0u;
        uint64_t r = rank0 + (wave_incl_scan_u32((uint32_t)__popc(m)) - (uint32_t)__popc(m));
        while (m != 0u && r < a.pos_cap) {
            bool open;
            const uint32_t len = find_span_one(sa, s_m, bytes, tsym, b, t, blen, 32u * lane + (uint32_t)__builtin_ctz(m), open);
            sa.len[r] = len;
            if (sa.open) sa.open[r] = (uint8_t)open;
            nopen += (uint32_t)open;
            r++;
            m &= m - 1u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       /* ... and read before the next tile overwrites them */
        __builtin_amdgcn_wave_barrier();
    }
    nopen = wave_total_u32(nopen);
    if (lane == 0 && nopen != 0u) atomicAdd((unsigned long long *)&a.totals[3], (unsigned long long)nopen);
}

/* No optional position and one length for all alternatives: nothing is decoded twice.  find_emit_kernel with that length
 * for every start it writes; no span is open. */
struct FindEmitLenArgs {
    FindArgs f;
    uint32_t *len;
    uint8_t *open;                          /* optional */
    uint32_t value;
};
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_emit_len_kernel(FindEmitLenArgs ea)
{
    const FindArgs &a = ea.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK) return;
    const uint64_t rank0 = two_level_prefix(a.scan, i);
    if (rank0 >= a.pos_cap) return;
    const uint64_t g = t * 64u + lane;
    uint32_t m = g * DSUB_SPL < blen ? a.bitmap[b * a.wpb + g] : 0u;
    uint64_t r = rank0 + (wave_incl_scan_u32((uint32_t)__popc(m)) - (uint32_t)__popc(m));
    const uint64_t base = b * a.s.bsize + g * DSUB_SPL;
    while (m != 0u && r < a.pos_cap) {
        a.pos[r] = base + (uint32_t)__builtin_ctz(m);
        ea.len[r] = ea.value;
        if (ea.open) ea.open[r] = 0;
        r++;
        m &= m - 1u;
    }
}

/* ---- hufgpu_find_records: from the match mask and the delimiter mask of one walk to records -------------------------- */

#define FIND_REC_OPEN (~0ull)               /* a record whose start or end lies in or behind a block that is not served */

/* a workgroup = one SCAN_GROUP of tiles: the tiles' delimiter counts summed as find_scan_kernel sums the matches.  A tile
 * of a block that is not served counts ONE delimiter that is nowhere: a look-up that lands on it learns that its record
 * is open.  (The statuses are final: find_rec_sub_kernel has ended.) */
__global__ __launch_bounds__(SCAN_GROUP) void find_rec_dscan_kernel(FindRecArgs ra)
{
    __shared__ uint64_t s_part[SCAN_GROUP / 64];
    const FindArgs &a = ra.p.f;
    const uint64_t i = (uint64_t)blockIdx.x * SCAN_GROUP + threadIdx.x;
    uint64_t c = 0;
    if (i < a.ntiles) {
        const uint64_t b = i / a.tpb, t = i % a.tpb;
        if (t * HUF_SUB_TILE < find_block_len(a, b)) c = a.errs[b] == HUFE_OK ? ra.dcnt[i] : 1u;
    }
    scan_group_publish<SCAN_GROUP>(ra.dscan, i, a.ntiles, c, s_part);
}

/* hufgpu_find_records_context: find_rec_dscan_kernel with a HEAVY virtual delimiter.  A tile of a block that is not served
 * counts max(before, after) + 1 delimiters that are nowhere, so two records with such a block between them are farther
 * apart, in numbers, than either distance: no context is measured across it.  The look-ups of the record kernels only need
 * the count to be non-zero, and a record's number is known in front of the first such block only, where nothing changes.
 * (At most 2^31 - 1 tiles of at most 2^32 each: the sums fit in the scan's 64 bits.) */
struct FindCtxArgs {
    FindRecArgs r;                          /* r.rbits / r.rcnt: the SELECTED records, as mark (and invert) leave them */
    uint32_t *cbits;                        /* [nblocks][wpb] the starts of the records to report: selected or context */
    uint32_t *ccnt;                         /* [nblocks][tpb] ... and how many of them a tile holds */
    TwoLevel rscan;                         /* of the tiles' selected records (find_scan_kernel on rcnt); rscan.total: how many there are */
    uint32_t before, after;
};

/* a workgroup = ONE wave = one SCAN_GROUP of tiles, a lane four of them, as two_level_arrive's last wave scans its group: no
 * LDS.  (Tile numbers fit in 32 bits, so the lanes divide 32-bit values.) */
__global__ __launch_bounds__(64) void find_ctx_dscan_kernel(FindCtxArgs ca)
{
    static_assert(SCAN_GROUP == 256, "a lane scans four tiles of its group");
    const FindRecArgs &ra = ca.r;
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id(), ntiles = (uint32_t)a.ntiles, tpb = (uint32_t)a.tpb;
    const uint32_t i0 = blockIdx.x * SCAN_GROUP + lane * 4u;
    const uint64_t heavy = (uint64_t)dmax(ca.before, ca.after) + 1u;
    uint64_t v[4], own = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t i = i0 + j;
        v[j] = 0;
        if (i < ntiles) {
            const uint32_t b = i / tpb, t = i % tpb;
            if ((uint64_t)t * HUF_SUB_TILE < find_block_len(a, b)) v[j] = a.errs[b] == HUFE_OK ? (uint64_t)ra.dcnt[i] : heavy;
        }
        own += v[j];
    }
    const uint64_t incl = wave_incl_scan_u64(own);
    uint64_t run = incl - own;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (i0 + j < ntiles) ra.dscan.local[i0 + j] = run;
        run += v[j];
    }
    if (lane == 63) handover_store(ra.dscan.gsum + blockIdx.x, incl);
    two_level_finish(ra.dscan, gridDim.x);
}

/* the delimiters, real and virtual, of the tiles in front of tile k; k = ntiles: of all tiles */
__device__ __forceinline__ uint64_t find_rec_before(const FindRecArgs &ra, uint64_t k)
{
    return k < ra.p.f.ntiles ? two_level_prefix(ra.dscan, k) : *ra.dscan.total;
}

/* the lane's delimiter word of tile (b, t); 0 behind the block's end */
__device__ __forceinline__ uint32_t find_rec_dword(const FindRecArgs &ra, uint64_t b, uint64_t t, uint32_t lane)
{
    const uint64_t g = t * 64u + lane;
    return g * DSUB_SPL < find_block_len(ra.p.f, b) ? ra.dbits[b * ra.p.f.wpb + g] : 0u;
}

/* Called by a full wave, every lane with the same i: where the record starts that is open at the start of tile i - behind
 * the last delimiter of the tiles in front, which a binary search in the scanned counts finds (the nearest tile j < i
 * whose count is not 0: O(log ntiles) reads whatever lies between, then one bit scan of its 64 words); byte 0 when there
 * is none.  The start comes back as its word of a [nblocks][wpb] mask, its bit there and its tile; false when that
 * tile's block is not served: the start is not known. */
__device__ __forceinline__ bool find_rec_start_before(const FindRecArgs &ra, uint64_t i, uint32_t lane, uint64_t &word, uint32_t &bit,
                                                      uint64_t &tile)
{
    const FindArgs &a = ra.p.f;
    const uint64_t c = find_rec_before(ra, i);
    word = tile = 0;
    bit = 1u;
    if (c == 0) return true;
    uint64_t lo = 0, hi = i;                                        /* the first k with before(k) >= c: before(0) = 0 < c = before(i) */
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (find_rec_before(ra, mid) >= c) hi = mid;
        else lo = mid + 1;
    }
    /* tile j has a delimiter, the tiles between j and i have none (32-bit and wave-uniform: there are at most 2^31 - 1 tiles) */
    const uint32_t j = uni32((uint32_t)lo - 1u);
    const uint64_t b = j / (uint32_t)a.tpb, t = j % (uint32_t)a.tpb;
    if (a.errs[b] != HUFE_OK) return false;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const uint64_t nz = __ballot(d != 0u);
    if (nz == 0) return false;                                      /* (cannot be: a served tile's count is that of its words) */
    const int top = 63 - __builtin_clzll(nz);
    const uint32_t w = (uint32_t)__shfl((int)d, top);
    const uint64_t rel = t * HUF_SUB_TILE + 32u * (uint32_t)top + (32u - (uint32_t)__builtin_clz(w));     /* behind it, in block b */
    const bool next = rel >= find_block_len(a, b);                  /* it was the block's last byte: tile j + 1 opens block b + 1 */
    word = next ? (b + 1) * a.wpb : b * a.wpb + (rel >> 5);
    bit = next ? 1u : 1u << ((uint32_t)rel & 31u);
    tile = next ? (b + 1) * a.tpb : b * a.tpb + rel / HUF_SUB_TILE;
    return true;
}

/* ... and where the record ends that is open at the end of tile i: at the first delimiter of the tiles behind, raw_size
 * when there is none, FIND_REC_OPEN when that tile's block is not served */
__device__ __forceinline__ uint64_t find_rec_end_behind(const FindRecArgs &ra, uint64_t i, uint32_t lane)
{
    const FindArgs &a = ra.p.f;
    const uint64_t c = find_rec_before(ra, i + 1);
    if (c == find_rec_before(ra, a.ntiles)) return a.s.raw_size;
    uint64_t lo = i + 1, hi = a.ntiles - 1;                         /* the first j > i with before(j + 1) > c */
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (find_rec_before(ra, mid + 1) > c) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t j = uni32((uint32_t)lo);
    const uint64_t b = j / (uint32_t)a.tpb, t = j % (uint32_t)a.tpb;
    if (a.errs[b] != HUFE_OK) return FIND_REC_OPEN;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const uint64_t nz = __ballot(d != 0u);
    if (nz == 0) return FIND_REC_OPEN;
    const int first = __builtin_ctzll(nz);
    const uint32_t w = (uint32_t)__shfl((int)d, first);
    return b * a.s.bsize + t * HUF_SUB_TILE + 32u * (uint32_t)first + (uint32_t)__builtin_ctz(w);
}

/* what a lane knows of the delimiters of its tile around its own word d: the position in the tile of the last one in front
 * of the word and of the first one behind it (-1: none in the tile), and the bits of the word below its first and above
 * its last delimiter */
struct FindRecLane {
    int prev, next;
    uint32_t head, tail;
};
__device__ __forceinline__ FindRecLane find_rec_lane(uint32_t d, uint32_t lane)
{
    const uint64_t nz = __ballot(d != 0u);
    /* the lanes below and above this one with a delimiter, in halves of 32 lanes (shifts of 32-bit words only) */
    const uint32_t lo = (uint32_t)nz, hi = (uint32_t)(nz >> 32), l = lane & 31u;
    const uint32_t lt = (1u << l) - 1u, gt = l == 31u ? 0u : 0xffffffffu << (l + 1u);
    const uint32_t below_lo = lane < 32u ? lo & lt : lo, below_hi = lane < 32u ? 0u : hi & lt;
    const uint32_t above_lo = lane < 32u ? lo & gt : 0u, above_hi = lane < 32u ? hi : hi & gt;
    const int pl = below_hi != 0u ? 63 - __builtin_clz(below_hi) : (below_lo != 0u ? 31 - __builtin_clz(below_lo) : -1);
    const int nl = above_lo != 0u ? __builtin_ctz(above_lo) : (above_hi != 0u ? 32 + __builtin_ctz(above_hi) : -1);
    const uint32_t dp = (uint32_t)__shfl((int)d, pl < 0 ? 0 : pl), dn = (uint32_t)__shfl((int)d, nl < 0 ? 0 : nl);
    FindRecLane k;
    k.prev = pl < 0 ? -1 : 32 * pl + 31 - __builtin_clz(dp);
    k.next = nl < 0 ? -1 : 32 * nl + __builtin_ctz(dn);
    k.head = d != 0u ? (d & (0u - d)) - 1u : 0xffffffffu;
    const uint32_t top = d != 0u ? 31u - (uint32_t)__builtin_clz(d) : 0u;
    k.tail = d != 0u ? (top == 31u ? 0u : 0xffffffffu << (top + 1u)) : 0xffffffffu;
    return k;
}

/* a wave = one tile, a lane = one word of match starts and one of delimiters.  Every match sets the bit of its record's
 * start in rbits (atomic OR: a record with many matches is one bit, and whoever sets it counts it for the tile of the
 * start), when the record is known: its start lies behind a
 * delimiter of a served block or at byte 0, its end at one or at raw_size.  Start and end are looked for in the lane's
 * word, then in the tile's (two shuffles a lane), and only for the tile's first and last record beyond it: at most two
 * look-ups a TILE, however many matches it has and however long the record is. */
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_mark_kernel(FindRecArgs ra)
{
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK || a.tcnt[i] == 0u) return;
    const uint64_t g = t * 64u + lane;
    const uint32_t m = g * DSUB_SPL < blen ? a.bitmap[b * a.wpb + g] : 0u;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const FindRecLane k = find_rec_lane(d, lane);
    const bool head = k.prev < 0 && (m & k.head) != 0u, tail = k.next < 0 && (m & k.tail) != 0u;
    uint64_t hw = 0;                                                /* the word and the bit of the start in front of the tile; */
    uint32_t hbit = 0;                                              /* no bit: that start is not known */
    uint64_t htile = 0;
    bool tail_open = false;
    if (__ballot(head) != 0 && !find_rec_start_before(ra, i, lane, hw, hbit, htile)) hbit = 0u;
    if (__ballot(tail) != 0) tail_open = find_rec_end_behind(ra, i, lane) == FIND_REC_OPEN;
    uint32_t *row = ra.rbits + b * a.wpb + t * 64u;
    uint32_t mm = m, last = ~0u, fresh = 0;                         /* last: the start set last, in the tile; 2048 = in front of it */
    while (mm != 0u) {
        const uint32_t bit = (uint32_t)__builtin_ctz(mm);
        mm &= mm - 1u;
        const uint32_t dl = d & ((1u << bit) - 1u);                 /* (the bit itself is no delimiter: the pattern holds none) */
        const uint32_t s = dl != 0u ? 32u * lane + 32u - (uint32_t)__builtin_clz(dl) : (k.prev >= 0 ? (uint32_t)k.prev + 1u : HUF_SUB_TILE);
        if ((d >> bit) == 0u && k.next < 0 && tail_open) continue;
        if (s == last || (s == HUF_SUB_TILE && hbit == 0u)) continue;
        last = s;
        if (s == HUF_SUB_TILE) {
            if ((atomicOr(&ra.rbits[hw], hbit) & hbit) == 0u) atomicAdd(&ra.rcnt[htile], 1u);
        } else {
            fresh += (atomicOr(&row[s >> 5], 1u << (s & 31u)) & (1u << (s & 31u))) == 0u;
        }
    }
    const uint32_t cnt = wave_total_u32(fresh);
    if (lane == 0 && cnt != 0u) atomicAdd(&ra.rcnt[i], cnt);
}

/* ---- hufgpu_find_records_terms: the records that hold ALL of several terms, or all of them in order ---------------------- */

/* Behind find_rec_mark_kernel, which has run once a term into that term's record mask: a wave = one tile, a lane = one word.
 * A record holds every term when its start is set in every term's mask, and mark sets a record's bit in the tile of its
 * START wherever the match lies, so the AND is local to the tile.  Plain stores into r.rbits / r.rcnt, which nobody has
 * written before: afterwards they are what mark alone leaves for the older calls, for every word and count that a later
 * kernel reads.  A tile of a block that is not served reports nothing. */
struct FindAllArgs {
    FindRecArgs r;
    FindTerms t;
};
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_all_kernel(FindAllArgs aa)
{
    const FindRecArgs &ra = aa.r;
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen) return;
    const uint64_t g = t * 64u + lane;
    const bool inside = g * DSUB_SPL < blen;
    bool some = a.errs[b] == HUFE_OK;                               /* does every term have a record that starts in this tile (the wave's) */
    for (uint32_t k = 0; some && k < aa.t.n_terms; k++) some = aa.t.rcnt[k * a.ntiles + i] != 0u;
    uint32_t r = some && inside ? 0xffffffffu : 0u;
    for (uint32_t k = 0; some && k < aa.t.n_terms; k++) r &= inside ? aa.t.rbits[k * aa.t.nwords + b * a.wpb + g] : 0u;
    if (inside) ra.rbits[b * a.wpb + g] = r;
    const uint32_t cnt = wave_total_u32((uint32_t)__popc(r));
    if (lane == 0) ra.rcnt[i] = cnt;
}

/* HUFGPU_TERMS_ORDERED, behind find_rec_all_kernel: of the records that hold every term, those that hold them one behind
 * the other.  All alternatives of a term have one length, so a term's leftmost occurrence is the one that ends first, and
 * the greedy walk is exact: x = the record's start, then for every term in turn p = the first match start of the term in
 * [x, e) - none: the record's bit is cleared - and x = p + the term's length.  A match lies inside one record, so p < e says
 * that all of it does.  tscan[t] is find_scan_kernel's scan of term t's gated tile counts, with totals of its own. */
struct FindSeqArgs {
    FindRecArgs r;
    FindTerms t;
    TwoLevel tscan[FIND_TERMS_MAX];
};

/* Called by a full wave, every lane with the same t, x and e, x < e, both in one record whose extent is known (so every block
 * that [x, e) touches is served, and the term's mask is complete there): the first match start p of term t at or behind x.
 * The 64 words of the tile that holds x; when they have none, ONE look-up in the scanned counts for the first tile behind it
 * that has a match - O(log tiles) reads however far away it is - and a bit scan of that tile.  false: none below e. */
__device__ __forceinline__ bool find_seq_first(const FindSeqArgs &sa, uint32_t t, uint64_t x, uint64_t e, uint32_t lane, uint64_t &p)
{
    const FindArgs &a = sa.r.p.f;
    const uint32_t *mw = sa.t.mbits + t * sa.t.nwords;
    uint64_t jb = x / a.s.bsize;
    const uint64_t rel = x - jb * a.s.bsize;
    uint64_t jt = rel / HUF_SUB_TILE;
    const uint64_t g = jt * 64u + lane;
    uint32_t w = g * DSUB_SPL < find_block_len(a, jb) ? mw[jb * a.wpb + g] : 0u;
    const uint32_t xw = (uint32_t)(rel >> 5) & 63u;                 /* x's word in its tile: nothing below x counts */
    if (lane < xw) w = 0u;
    else if (lane == xw) w &= ~find_low_bits((uint32_t)rel & 31u);
    uint64_t nz = __ballot(w != 0u);
    if (nz == 0) {
        const TwoLevel &sc = sa.tscan[t];
        const uint64_t i = jb * a.tpb + jt;
        const auto pre = [&](uint64_t k) { return k < a.ntiles ? two_level_prefix(sc, k) : *sc.total; };
        const uint64_t c = pre(i + 1);
        if (c == pre(a.ntiles)) return false;
        uint64_t lo = i + 1, hi = a.ntiles - 1;                     /* the first j > i with pre(j + 1) > c */
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pre(mid + 1) > c) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t j = uni32((uint32_t)lo);                     /* (a tile of a served block: the scan counts no other) */
        jb = j / (uint32_t)a.tpb;
        jt = j % (uint32_t)a.tpb;
        const uint64_t gj = jt * 64u + lane;
        w = gj * DSUB_SPL < find_block_len(a, jb) ? mw[jb * a.wpb + gj] : 0u;
        nz = __ballot(w != 0u);
        if (nz == 0) return false;                                  /* (cannot be: the tile's count is that of its words) */
    }
    const uint32_t first = uni32((uint32_t)__builtin_ctzll(nz));
    p = jb * a.s.bsize + jt * HUF_SUB_TILE + 32u * first + (uint32_t)__builtin_ctz(wave_lane_u32(w, first));
    return p < e;
}

/* A wave = one tile, a lane = one word of record starts.  A record that ends inside the tile - every one but the tile's last,
 * when no delimiter lies behind that one's start - is its lane's own: the lane reads the terms' words of the tile, from x's
 * word to e's at most.  The tile's last record is the wave's: its end comes from find_rec_emit_body's look-up, and every
 * term costs find_seq_first, so the cost does not follow the record's length.  Plain stores over find_rec_all_kernel's words
 * (a record's bit lies in the tile of its start: no other wave reads or writes them here), then the tile's count anew. */
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_seq_kernel(FindSeqArgs sa)
{
    const FindRecArgs &ra = sa.r;
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id(), nt = sa.t.n_terms;
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK || ra.rcnt[i] == 0u) return;
    const uint64_t g = t * 64u + lane, wbase = b * a.wpb + t * 64u;
    const uint32_t r = g * DSUB_SPL < blen ? ra.rbits[b * a.wpb + g] : 0u;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const FindRecLane k = find_rec_lane(d, lane);
    /* two starts of a tile have a delimiter between them, so at most one start of the tile has none behind it */
    const uint32_t tail = k.next < 0 ? r & k.tail : 0u;
    uint32_t keep = r, rr = r & ~tail;
    while (rr != 0u) {
        const uint32_t bit = (uint32_t)__builtin_ctz(rr);
        rr &= rr - 1u;
        const uint32_t du = (d >> bit) << bit;
        const uint32_t e = du != 0u ? 32u * lane + (uint32_t)__builtin_ctz(du) : (uint32_t)k.next;      /* in the tile; x < e: the record holds a match */
        uint32_t x = 32u * lane + bit;
        bool ok = true;
        for (uint32_t q = 0; ok && q < nt; q++) {
            const uint32_t *mw = sa.t.mbits + q * sa.t.nwords + wbase;
            const uint32_t last = (e - 1u) >> 5;
            uint32_t wi = x >> 5, w = mw[wi] & ~find_low_bits(x & 31u);
            while (w == 0u && wi < last) w = mw[++wi];
            const uint32_t p = 32u * wi + (w != 0u ? (uint32_t)__builtin_ctz(w) : 32u);
            x = p + sa.t.len[q];
            ok = p < e && (q + 1u == nt || x < e);
        }
        if (!ok) keep &= ~(1u << bit);
    }
    const uint64_t has_tail = __ballot(tail != 0u);
    if (has_tail != 0) {
        const uint32_t at = uni32((uint32_t)__builtin_ctzll(has_tail));
        const uint32_t bit = (uint32_t)__builtin_ctz(wave_lane_u32(tail, at));
        const uint64_t e = find_rec_end_behind(ra, i, lane);        /* (known: mark has dropped the records whose end is not) */
        uint64_t x = b * a.s.bsize + t * HUF_SUB_TILE + 32u * at + bit;
        bool ok = e != FIND_REC_OPEN;
        for (uint32_t q = 0; ok && q < nt; q++) {
            uint64_t p = 0;
            ok = x < e && find_seq_first(sa, q, x, e, lane, p);
            x = p + sa.t.len[q];
        }
        if (!ok && lane == at) keep &= ~(1u << bit);
    }
    if (keep != r) ra.rbits[b * a.wpb + g] = keep;
    const uint32_t cnt = wave_total_u32((uint32_t)__popc(keep));
    if (lane == 0) ra.rcnt[i] = cnt;
}

/* hufgpu_find_records_select: the records' route with two more answers.  r is the any-of call's; no is d_rec_no, or NULL;
 * first_bad is one word of the find workspace: the first block that is not served, ~0 when every block is */
struct FindSelArgs {
    FindRecArgs r;
    uint64_t *no;
    uint64_t *first_bad;
};

#define FIND_REC_NO_UNKNOWN (~0ull)         /* = HUFGPU_REC_NO_UNKNOWN (include/huffman_gpu.h) */

/* one thread per block (the statuses are final: the walk has ended; *first_bad is ~0 when this kernel starts).  The lanes'
 * blocks ascend, so a wave's lowest lane with a block that is not served speaks for it: no atomic while all are served. */
__global__ __launch_bounds__(256) void find_rec_first_bad_kernel(FindSelArgs sa)
{
    const FindArgs &a = sa.r.p.f;
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = b < a.s.nblocks && a.errs[b] != HUFE_OK;
    const uint64_t any = __ballot(bad);
    if (any != 0 && (uint32_t)lane_id() == (uint32_t)__builtin_ctzll(any)) atomicMin((unsigned long long *)sa.first_bad, (unsigned long long)b);
}

/* HUFGPU_SELECT_INVERT, behind find_rec_mark_kernel: a wave = one tile, a lane = one word.  When mark has ended rbits holds
 * the start of every known record with a match - in the START's tile, wherever the match lies - so this kernel is local to
 * its tile: the candidates are the bytes behind a delimiter that are none themselves (byte 0 is one; nothing behind the
 * block's end is), the byte in front of the lane's word coming from the lane below and, for lane 0, from the last word of
 * the tile in front - the last, maybe short tile of block b - 1 for a block's first tile, and no candidate when that block
 * is not served: the start is not known.  Every candidate but the tile's last ends inside the tile, at a real delimiter of
 * a served block; the last one (no delimiter behind it in the tile) costs ONE look-up a tile, as in find_rec_emit_kernel,
 * and is dropped when its end is open.  What is left is the non-empty records whose extent is known; those without a match
 * are candidates & ~rbits.  Plain stores over mark's words and counts: scan, finish and emit then run as they are.  A tile of
 * a block that is not served reports nothing. */
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_invert_kernel(FindRecArgs ra)
{
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen) return;
    const uint64_t g = t * 64u + lane;
    const bool inside = g * DSUB_SPL < blen;
    uint32_t *word = ra.rbits + b * a.wpb + g;
    if (a.errs[b] != HUFE_OK) {
        if (inside) *word = 0u;
        if (lane == 0) ra.rcnt[i] = 0u;
        return;
    }
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const uint32_t r = inside ? *word : 0u;
    uint32_t c0;                                                    /* is the byte in front of the tile a delimiter (the wave's) */
    if (i == 0) {
        c0 = 1u;
    } else if (t != 0) {
        c0 = ra.dbits[b * a.wpb + t * 64u - 1u] >> 31;              /* (the tile in front is a full one) */
    } else if (a.errs[b - 1] != HUFE_OK) {
        c0 = 0u;
    } else {
        const uint64_t last = a.s.bsize - 1u;                       /* (a block with a block behind it is a full one) */
        c0 = (ra.dbits[(b - 1) * a.wpb + (last >> 5)] >> ((uint32_t)last & 31u)) & 1u;
    }
    const uint32_t below = wave_up1_u32(d);                         /* (by every lane: a lane that sits out of a DPP move is not read) */
    const uint32_t carry = lane == 0 ? c0 : below >> 31;
    const uint64_t left = inside ? blen - g * DSUB_SPL : 0u;
    const uint32_t valid = left >= 32u ? 0xffffffffu : (1u << (uint32_t)left) - 1u;
    uint32_t cand = ((d << 1) | carry) & ~d & valid;
    const FindRecLane k = find_rec_lane(d, lane);
    const bool tail = k.next < 0 && (cand & k.tail) != 0u;
    if (__ballot(tail) != 0 && find_rec_end_behind(ra, i, lane) == FIND_REC_OPEN && tail) cand &= ~k.tail;
    const uint32_t n = cand & ~r;
    if (inside) *word = n;
    const uint32_t cnt = wave_total_u32((uint32_t)__popc(n));
    if (lane == 0) ra.rcnt[i] = cnt;
}

/* a wave = one tile, as find_emit_kernel: a set bit of rbits is a record's start s; its end is the first delimiter behind
 * it, looked for as find_rec_mark_kernel does (one look-up a tile at most: for its last record).  pos = s and
 * len = min(e - s, clip) go to the record's rank, the records cut by clip are counted into totals[3].
 * NO (find_rec_emit_no_kernel): the record's number goes to its rank as well - the delimiters in front of the tile, which
 * find_rec_dscan_kernel has scanned, plus those of the tile below s: a wave prefix over the words' popcounts and the bits
 * below s in the lane's own word.  The scan counts a delimiter that is nowhere for every tile of a block that is not served,
 * so the number is known only while no block in front of b is one of those: FIND_REC_NO_UNKNOWN otherwise.
 * SEL (find_ctx_emit_kernel, find_ctx_emit_no_kernel): the record's bit in a second mask, sbits, goes to its rank as well. */
template <bool NO, bool SEL = false>
__device__ __forceinline__ void find_rec_emit_body(const FindRecArgs &ra, [[maybe_unused]] const FindSelArgs *sa = nullptr,
                                                   [[maybe_unused]] const uint32_t *sbits = nullptr, [[maybe_unused]] uint8_t *sel = nullptr)
{
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK || ra.rcnt[i] == 0u) return;
    const uint64_t rank0 = two_level_prefix(a.scan, i);
    if (rank0 >= a.pos_cap) return;
    const uint64_t g = t * 64u + lane;
    uint32_t r = g * DSUB_SPL < blen ? ra.rbits[b * a.wpb + g] : 0u;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const FindRecLane k = find_rec_lane(d, lane);
    uint64_t e_tail = a.s.raw_size;
    if (__ballot(k.next < 0 && (r & k.tail) != 0u) != 0) e_tail = find_rec_end_behind(ra, i, lane);
    uint64_t rank = rank0 + (wave_incl_scan_u32((uint32_t)__popc(r)) - (uint32_t)__popc(r));
    const uint64_t base = b * a.s.bsize + t * HUF_SUB_TILE;
    [[maybe_unused]] uint64_t no0 = 0;                              /* the delimiters in front of the lane's word */
    [[maybe_unused]] bool known = false;
    if constexpr (NO) {
        no0 = find_rec_before(ra, i) + (wave_incl_scan_u32((uint32_t)__popc(d)) - (uint32_t)__popc(d));
        known = *sa->first_bad >= b;
    }
    [[maybe_unused]] uint32_t sw = 0;                               /* SEL: the lane's word of the selected records' mask */
    if constexpr (SEL) sw = g * DSUB_SPL < blen ? sbits[b * a.wpb + g] : 0u;
    uint32_t cut = 0;
    while (r != 0u && rank < a.pos_cap) {
        const uint32_t bit = (uint32_t)__builtin_ctz(r);
        r &= r - 1u;
        const uint32_t du = (d >> bit) << bit;
        const uint64_t s = base + 32u * lane + bit;
        const uint64_t e = du != 0u ? base + 32u * lane + (uint32_t)__builtin_ctz(du) : (k.next >= 0 ? base + (uint32_t)k.next : e_tail);
        const uint64_t n = e - s;
        a.pos[rank] = s;
        ra.len[rank] = n > ra.clip ? ra.clip : (uint32_t)n;
        if constexpr (NO) sa->no[rank] = known ? no0 + (uint32_t)__popc(d & ((1u << bit) - 1u)) : FIND_REC_NO_UNKNOWN;
        if constexpr (SEL) sel[rank] = (uint8_t)((sw >> bit) & 1u);
        cut += n > ra.clip;
        rank++;
    }
    const uint32_t cuts = wave_total_u32(cut);
    if (lane == 0 && cuts != 0u) atomicAdd((unsigned long long *)&a.totals[3], (unsigned long long)cuts);
}

__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_emit_kernel(FindRecArgs ra) { find_rec_emit_body<false>(ra); }
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_emit_no_kernel(FindSelArgs sa) { find_rec_emit_body<true>(sa.r, &sa); }

/* ---- hufgpu_find_records_context: the records around the selected ones (grep -A / -B / -C) ----------------------------- */

/* the selected records of the tiles in front of tile k (of the served blocks); k = ntiles: all of them */
__device__ __forceinline__ uint64_t find_ctx_sel_before(const FindCtxArgs &ca, uint64_t k)
{
    return k < ca.r.p.f.ntiles ? two_level_prefix(ca.rscan, k) : *ca.rscan.total;
}

/* Called by a full wave, every lane with the same served tile j that holds a selected record: the NUMBER of its last
 * (LAST) or first selected record - the delimiters in front of tile j plus those of the tile in front of the start.  One
 * bit scan of the tile's 64 words. */
template <bool LAST>
__device__ __forceinline__ bool find_ctx_sel_number(const FindCtxArgs &ca, uint32_t j, uint32_t lane, uint64_t &no)
{
    const FindArgs &a = ca.r.p.f;
    const uint64_t b = j / (uint32_t)a.tpb, t = j % (uint32_t)a.tpb;
    const uint64_t g = t * 64u + lane;
    const uint32_t r = g * DSUB_SPL < find_block_len(a, b) ? ca.r.rbits[b * a.wpb + g] : 0u;
    const uint32_t d = find_rec_dword(ca.r, b, t, lane);
    const uint64_t nz = __ballot(r != 0u);
    if (nz == 0) return false;                                      /* (cannot be: the tile's count is that of its words) */
    const uint32_t at = uni32(LAST ? 63u - (uint32_t)__builtin_clzll(nz) : (uint32_t)__builtin_ctzll(nz));
    const uint32_t w = wave_lane_u32(r, at);
    const uint32_t bit = LAST ? 31u - (uint32_t)__builtin_clz(w) : (uint32_t)__builtin_ctz(w);
    const uint32_t mine = lane < at ? (uint32_t)__popc(d) : (lane == at ? (uint32_t)__popc(d & ((1u << bit) - 1u)) : 0u);
    no = find_rec_before(ca.r, j) + wave_total_u32(mine);
    return true;
}

/* The look-ups of find_rec_ctx_kernel gallop: what they look for is nearly always in the tile next door - the delimiter that
 * ends a tile's last record, a selected record of a frequent pattern -, and when it is not, a tile far away seldom matters:
 * a record that many delimiters away is out of either distance.  `pre` is a scan over the tiles - pre(k): the sum over the
 * tiles in front of k, k = ntiles: the total -, all values are the wave's.
 * Backward, given c = pre(i) > 0: the nearest tile j < i that counts something.  Probes at i - 1, i - 2, i - 4, ..., each
 * followed by far(k) - "nothing in front of tile k matters", which ends the search with false -, then a binary search
 * between the last two probes: 2 log2(tiles) probes at most, two when the neighbour holds it. */
template <typename P, typename F>
__device__ __forceinline__ bool find_ctx_gallop_back(P pre, F far, uint64_t i, uint64_t c, uint32_t &j)
{
    uint64_t lo, hi = i;                                            /* pre(hi) = c: the tiles [hi, i) count nothing */
    for (uint64_t step = 1;; step <<= 1) {
        lo = i > step ? i - step : 0;
        if (pre(lo) < c) break;                                     /* (pre(0) = 0 < c at the latest) */
        if (far(lo)) return false;
        hi = lo;
    }
    lo++;                                                           /* the first k in (lo, hi] with pre(k) >= c */
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pre(mid) >= c) hi = mid;
        else lo = mid + 1;
    }
    j = uni32((uint32_t)lo - 1u);
    return true;
}
/* Forward, given c = pre(i + 1) < pre(ntiles): the first tile j > i that counts something; far(k): nothing in the tiles
 * from k on matters. */
template <typename P, typename F>
__device__ __forceinline__ bool find_ctx_gallop_on(P pre, F far, uint64_t i, uint64_t ntiles, uint64_t c, uint32_t &j)
{
    uint64_t lo = i + 1, hi;                                        /* pre(lo) = c: the tiles (i, lo) count nothing */
    for (uint64_t step = 1;; step <<= 1) {
        hi = dmin<uint64_t>(i + step, ntiles - 1);
        if (pre(hi + 1) > c) break;                                 /* (pre(ntiles) > c at the latest) */
        if (far(hi + 1)) return false;
        lo = hi + 1;
    }
    while (lo < hi) {                                               /* the first j in [lo, hi] with pre(j + 1) > c */
        const uint64_t mid = (lo + hi) >> 1;
        if (pre(mid + 1) > c) hi = mid;
        else lo = mid + 1;
    }
    j = uni32((uint32_t)lo);
    return true;
}

/* The number of the nearest selected record in the tiles in front of tile i, in the scanned counts of the selected records
 * as find_rec_start_before looks for a delimiter, and of the nearest one in the tiles behind.  false: there is none that
 * matters - none at all, or tile i's candidates, whose numbers lie in [before(i), before(i + 1)], are farther than the
 * distance from every record of the tiles that were not looked at.  (The scan counts the tiles of served blocks only.) */
__device__ __forceinline__ bool find_ctx_prev_tile(const FindCtxArgs &ca, uint64_t i, uint32_t lane, uint64_t &no)
{
    const uint64_t c = find_ctx_sel_before(ca, i);
    if (c == 0) return false;
    const uint64_t base = find_rec_before(ca.r, i);
    uint32_t j;
    if (!find_ctx_gallop_back([&](uint64_t k) { return find_ctx_sel_before(ca, k); },
                              [&](uint64_t k) { return base - find_rec_before(ca.r, k) > (uint64_t)ca.after; }, i, c, j))
        return false;
    return find_ctx_sel_number<true>(ca, j, lane, no);
}
__device__ __forceinline__ bool find_ctx_next_tile(const FindCtxArgs &ca, uint64_t i, uint32_t lane, uint64_t &no)
{
    const uint64_t ntiles = ca.r.p.f.ntiles;
    const uint64_t c = find_ctx_sel_before(ca, i + 1);
    if (c == find_ctx_sel_before(ca, ntiles)) return false;
    const uint64_t top = find_rec_before(ca.r, i + 1);
    uint32_t j;
    if (!find_ctx_gallop_on([&](uint64_t k) { return find_ctx_sel_before(ca, k); },
                            [&](uint64_t k) { return find_rec_before(ca.r, k) - top > (uint64_t)ca.before; }, i, ntiles, c, j))
        return false;
    return find_ctx_sel_number<false>(ca, j, lane, no);
}

/* find_rec_end_behind, galloping: where the record ends that is open at the end of tile i - nearly always in tile i + 1 */
__device__ __forceinline__ uint64_t find_ctx_end_behind(const FindRecArgs &ra, uint64_t i, uint32_t lane)
{
    const FindArgs &a = ra.p.f;
    const uint64_t c = find_rec_before(ra, i + 1);
    if (c == find_rec_before(ra, a.ntiles)) return a.s.raw_size;
    uint32_t j;
    find_ctx_gallop_on([&](uint64_t k) { return find_rec_before(ra, k); }, [](uint64_t) { return false; }, i, a.ntiles, c, j);
    const uint64_t b = j / (uint32_t)a.tpb, t = j % (uint32_t)a.tpb;
    if (a.errs[b] != HUFE_OK) return FIND_REC_OPEN;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const uint64_t nz = __ballot(d != 0u);
    if (nz == 0) return FIND_REC_OPEN;
    const uint32_t first = uni32((uint32_t)__builtin_ctzll(nz));
    return b * a.s.bsize + t * HUF_SUB_TILE + 32u * first + (uint32_t)__builtin_ctz(wave_lane_u32(d, first));
}

/* Behind find_rec_mark_kernel (and find_rec_invert_kernel), with the selected records' counts scanned: a wave = one tile, a
 * lane = one word.  Context is a dilation of rbits in record-NUMBER space.  The candidates are find_rec_invert_kernel's: the
 * starts of the non-empty records whose extent is known.  A candidate's number is the delimiters in front of its tile
 * (find_ctx_dscan_kernel) + the wave's prefix over the words' popcounts + the bits below it in its own word.  The nearest
 * selected record in front of it lies in the lane's own word, else in the lanes below (a wave max-scan of "my highest
 * selected start's number"), else in the tiles in front: ONE look-up a tile, and only for the candidates in front of the
 * tile's first selected record.  The nearest one behind it: the same, mirrored.  A candidate is reported when it is selected
 * itself, when it lies at most `after` behind the one or at most `before` in front of the other.  So a tile costs three
 * look-ups at most - the end of its last candidate, a neighbour in front, one behind -, each 2 log2(tiles) probes of a scan
 * at most and one bit scan, whatever the data and the distances are (and two probes when the neighbouring tile answers),
 * and none when it has no candidate that is not selected.  The answer goes to a SECOND mask and
 * count array (other tiles' waves read rbits); scan, finish and emit then run on those.  A tile of a block that is not
 * served writes nothing: the scan does not look at it. */
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_rec_ctx_kernel(FindCtxArgs ca)
{
    const FindRecArgs &ra = ca.r;
    const FindArgs &a = ra.p.f;
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t i = find_tile_index<FIND_EMIT_THREADS>();
    if (i >= a.ntiles) return;
    const auto [b, t, blen] = find_tile(a, i);
    if (t * HUF_SUB_TILE >= blen || a.errs[b] != HUFE_OK) return;
    const uint64_t g = t * 64u + lane;
    const bool inside = g * DSUB_SPL < blen;
    const uint32_t d = find_rec_dword(ra, b, t, lane);
    const uint32_t r = inside ? ra.rbits[b * a.wpb + g] : 0u;
    uint32_t c0;                                                    /* is the byte in front of the tile a delimiter (the wave's) */
    if (i == 0) {
        c0 = 1u;
    } else if (t != 0) {
        c0 = ra.dbits[b * a.wpb + t * 64u - 1u] >> 31;              /* (the tile in front is a full one) */
    } else if (a.errs[b - 1] != HUFE_OK) {
        c0 = 0u;
    } else {
        const uint64_t last = a.s.bsize - 1u;                       /* (a block with a block behind it is a full one) */
        c0 = (ra.dbits[(b - 1) * a.wpb + (last >> 5)] >> ((uint32_t)last & 31u)) & 1u;
    }
    const uint32_t below = wave_up1_u32(d);                         /* (by every lane) */
    const uint32_t carry = lane == 0 ? c0 : below >> 31;
    const uint64_t left = inside ? blen - g * DSUB_SPL : 0u;
    const uint32_t valid = left >= 32u ? 0xffffffffu : (1u << (uint32_t)left) - 1u;
    uint32_t cand = ((d << 1) | carry) & ~d & valid & ~r;           /* the candidates that are not selected themselves */
    uint32_t out = 0;
    if (__ballot(cand != 0u) != 0) {
        const FindRecLane k = find_rec_lane(d, lane);
        const bool tail = k.next < 0 && (cand & k.tail) != 0u;
        if (__ballot(tail) != 0 && find_ctx_end_behind(ra, i, lane) == FIND_REC_OPEN && tail) cand &= ~k.tail;
        /* numbers inside the tile: the delimiters of the tile in front of a start */
        const uint32_t pd = (uint32_t)__popc(d), rel0 = wave_incl_scan_u32(pd) - pd;
        const uint32_t rtop = r != 0u ? 31u - (uint32_t)__builtin_clz(r) : 0u, rlow = r != 0u ? (uint32_t)__builtin_ctz(r) : 0u;
        const uint32_t hs = r != 0u ? rel0 + (uint32_t)__popc(d & ((1u << rtop) - 1u)) + 1u : 0u;    /* (+ 1: 0 is "none") */
        const uint32_t ls = rel0 + (uint32_t)__popc(d & ((1u << rlow) - 1u));
        const uint32_t pmax = wave_excl_max_u32(hs);                /* the nearest selected record of the lanes below: its number + 1 */
        /* the nearest lane above with a selected record, in halves of 32 lanes (find_rec_lane) */
        const uint64_t nz = __ballot(r != 0u);
        const uint32_t nlo = (uint32_t)nz, nhi = (uint32_t)(nz >> 32), l = lane & 31u;
        const uint32_t gt = l == 31u ? 0u : 0xffffffffu << (l + 1u);
        const uint32_t above_lo = lane < 32u ? nlo & gt : 0u, above_hi = lane < 32u ? nhi : nhi & gt;
        const int nl = above_lo != 0u ? __builtin_ctz(above_lo) : (above_hi != 0u ? 32 + __builtin_ctz(above_hi) : -1);
        const uint32_t nmin = (uint32_t)__shfl((int)ls, nl < 0 ? 0 : nl);
        /* the tiles in front and behind, for the candidates that have no selected record on that side in the tile */
        const bool want_prev = pmax == 0u && (cand & (r != 0u ? (1u << rlow) - 1u : 0xffffffffu)) != 0u;
        const bool want_next = nl < 0 && (cand & (r != 0u ? (rtop == 31u ? 0u : 0xffffffffu << (rtop + 1u)) : 0xffffffffu)) != 0u;
        uint64_t pno = 0, nno = 0;
        bool has_prev = false, has_next = false;
        if (ca.after != 0u && __ballot(want_prev) != 0) has_prev = find_ctx_prev_tile(ca, i, lane, pno);
        if (ca.before != 0u && __ballot(want_next) != 0) has_next = find_ctx_next_tile(ca, i, lane, nno);
        const uint64_t base = find_rec_before(ra, i);
        uint32_t cc = cand;
        while (cc != 0u) {
            const uint32_t bit = (uint32_t)__builtin_ctz(cc);
            cc &= cc - 1u;
            const uint32_t lowm = (1u << bit) - 1u;
            const uint32_t n = rel0 + (uint32_t)__popc(d & lowm);
            const uint32_t rl = r & lowm, ru = r & ~lowm;            /* (the bit itself is not selected) */
            bool near = false;
            if (rl != 0u) near = n - (rel0 + (uint32_t)__popc(d & ((1u << (31u - (uint32_t)__builtin_clz(rl))) - 1u))) <= ca.after;
            else if (pmax != 0u) near = n + 1u - pmax <= ca.after;
            else if (has_prev) near = base + n - pno <= (uint64_t)ca.after;
            if (ru != 0u) near |= rel0 + (uint32_t)__popc(d & ((1u << (uint32_t)__builtin_ctz(ru)) - 1u)) - n <= ca.before;
            else if (nl >= 0) near |= nmin - n <= ca.before;
            else if (has_next) near |= nno - (base + n) <= (uint64_t)ca.before;
            out |= (uint32_t)near << bit;
        }
    }
    out |= r;
    if (inside) ca.cbits[b * a.wpb + g] = out;
    const uint32_t cnt = wave_total_u32((uint32_t)__popc(out));
    if (lane == 0) ca.ccnt[i] = cnt;
}

/* find_rec_emit_kernel and find_rec_emit_no_kernel with d_rec_sel: s.r.rbits / s.r.rcnt are the mask and the counts of the
 * records to report, sbits is the mask of the selected ones - the flag of a reported record is its bit there - and sel goes
 * to the record's rank as its start and its length do.  s.no and s.first_bad are not looked at without the numbers. */
struct FindCtxEmitArgs {
    FindSelArgs s;
    const uint32_t *sbits;
    uint8_t *sel;
};
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_ctx_emit_kernel(FindCtxEmitArgs ea) { find_rec_emit_body<false, true>(ea.s.r, &ea.s, ea.sbits, ea.sel); }
__global__ __launch_bounds__(FIND_EMIT_THREADS) void find_ctx_emit_no_kernel(FindCtxEmitArgs ea) { find_rec_emit_body<true, true>(ea.s.r, &ea.s, ea.sbits, ea.sel); }

}  // namespace hufgpu

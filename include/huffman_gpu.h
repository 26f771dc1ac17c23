/*
 * huffman_gpu.h - device-resident entry points of the MI355X Huffman block codec.
 *
 * The reference has one boundary for the hot path: huf_encode()/huf_decode() over callback
 * streams (include/huffman/encoder.h:25-26, decoder.h:25-26).  Those are served by this
 * library too (include/huffman.h).  The functions below are the same per-block hot path with
 * the callback streams peeled off: plain pointers into HBM and sizes, no host copies.  They
 * are what huf_encode()/huf_decode() call internally after staging a batch, what the Python
 * layer calls when the data already lives on the GPU, and what bench.py times.
 *
 * C ABI only: no C++ or torch types; `stream` arguments are a hipStream_t passed as void*
 * (NULL = the device's default stream).  All functions return a huf_error_t value
 * (include/huffman.h); HIP failures map to HUF_ERROR_FATAL and hufgpu_last_error() carries
 * the text.  Nothing here falls back to the CPU.
 *
 * Replaces, per block (reference file:line):
 *   hufgpu_histogram      src/histogram.c:73-103   huf_histogram_populate (iota = 1)
 *   hufgpu_encode         src/encoder.c:288-374    block loop: histogram, tree.c:292-427 tree,
 *                                                   encoder.c:40-81 codes, tree.c:233-289
 *                                                   serialize, encoder.c:85-131 bit-pack
 *   hufgpu_decode         src/decoder.c:218-276    header parse, tree.c:138-227 deserialize,
 *                                                   decoder.c:34-96 tree walk
 */
#ifndef INCLUDE_huffman_gpu_h__
#define INCLUDE_huffman_gpu_h__

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-device workspace (side tables, ticket counters, profiling events).  Not thread-safe, and
 * its calls share that workspace: enqueue them on ONE stream at a time (or wait for the stream
 * before switching to another); use one context per concurrently used stream. */
typedef struct hufgpu_ctx hufgpu_ctx_t;

/* Decode flags. */
#define HUFGPU_STRICT_TREE  0u  /* tree_len > 1024 -> HUF_ERROR_BTREE_OVERFLOW (reference parity,
                                   src/decoder.c:237-239) */
#define HUFGPU_RELAXED_TREE 1u  /* accept the 1025-entry tree the encoder itself emits for blocks
                                   with all 256 byte values */

#define HUFGPU_RANGES_TILES 4u  /* hufgpu_decode_ranges only (every other entry point ignores it): the caller states that
                                 * d_sub_index is the sub-index of this very stream; cut blocks are then decoded by the
                                 * sub-index tile, not whole - see TILES at hufgpu_decode_ranges */
#define HUFGPU_SEQUENTIAL   2u  /* hufgpu_decode_stream only: skip the parallel block discovery and take the
                                   blocks strictly in order (diagnostics; results are identical) */

/* Largest block the kernels take (bytes).  Larger blocks -> HUF_ERROR_INVALID_ARGUMENT.  (Codes are
 * kept in 56 bits, which any block below F(57) = 3.6e11 bytes satisfies; the limit is what still
 * fits a device together with its stream and its output.)  hufgpu_histogram() returns 32-bit counts
 * and takes blocks below 2^32 bytes only. */
#define HUFGPU_MAX_BLOCK ((uint64_t)1 << 38)

/* Number of usable gfx950 devices; 0 when HIP is unusable (never an error by itself). */
int hufgpu_device_count(void);

/* Create/destroy a context bound to `device`. HUF_ERROR_FATAL when there is no such GPU. */
int hufgpu_ctx_create(hufgpu_ctx_t **ctx, int device);
int hufgpu_ctx_destroy(hufgpu_ctx_t *ctx);
int hufgpu_ctx_device(const hufgpu_ctx_t *ctx);      /* the device ordinal the context was made for (-1: no context) */

/* Text of the last failure on this context (or of the last global failure if ctx == NULL). */
const char *hufgpu_last_error(const hufgpu_ctx_t *ctx);

/* Number of blocks huf_encode produces for n input bytes (src/encoder.c:288-293). */
uint64_t hufgpu_block_count(uint64_t n, uint64_t blocksize);

/* Capacity (bytes) that always holds the encoded stream of n bytes. */
uint64_t hufgpu_encode_bound(uint64_t n, uint64_t blocksize);

/* 256-bin byte histogram of each block: d_hist[block * 256 + byte] (uint32). */
int hufgpu_histogram(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                     uint32_t *d_hist, void *stream);

/*
 * Encode n bytes at d_in into the libhuffman block stream at d_out (both in HBM).
 *   d_block_offsets : optional, nblocks+1 uint64 in HBM; receives the byte offset of every
 *                     block header in d_out, the last entry being the stream length.  This is
 *                     the in-process block index (the wire format itself stores no payload
 *                     length - SURVEY §0 fact 1).
 *   out_len         : optional host pointer; when given the call synchronises and stores the
 *                     stream length.  When NULL the call only enqueues work on the stream.
 */
int hufgpu_encode(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                  void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                  uint64_t *out_len, void *stream);

/*
 * Decode a block stream whose block index is known (d_block_offsets from hufgpu_encode).
 *   raw_len  : optional host pointer; when given the call synchronises, stores the number of
 *              bytes delivered in d_out and returns the first error in stream order
 *              (HUF_ERROR_BTREE_OVERFLOW / _CORRUPTED / _READ_WRITE like src/decoder.c).  After an
 *              error these are the blocks in front of the failing one AND the symbols of the failing
 *              block that src/decoder.c:69-91 delivers before it stops (the block is decoded once
 *              more, in order, with its record as the whole input).
 *              When NULL the call only enqueues; fetch the result with hufgpu_decode_result().
 */
int hufgpu_decode(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                  const uint64_t *d_block_offsets, uint64_t nblocks,
                  void *d_out, uint64_t out_cap, uint32_t flags,
                  uint64_t *raw_len, void *stream);

/*
 * The same pair with the encoder's SUB-INDEX: besides the block index the encoder can hand over
 * where, inside every block's payload, each group of 32 symbols starts (2 bytes per 32 symbols +
 * 8 bytes per 2 048 symbols + the 256 code lengths of every block; hufgpu_sub_index_bytes() bytes, 8-byte aligned, in HBM).  Like the
 * block index it is in-process side information - the stream is the reference's, byte for byte.
 * With it hufgpu_decode_sub() decodes every symbol once instead of finding the codeword starts by
 * decoding speculatively (src/decoder.c:34-96 has the same information implicitly: it walks the
 * bits in order).  The sub-index is VERIFIED while it is used: a group must decode to exactly its
 * recorded bit count with every walk inside the tree and inside the payload; a block for which
 * that fails (stale or foreign sub-index, damaged stream) is decoded again without it, so results
 * and error codes are those of hufgpu_decode() for ANY content of d_sub_index.
 *   raw_size, blocksize : the n and blocksize of the encode that produced stream and sub-index
 *                         (they fix the block count and the layout of d_sub_index).
 */
uint64_t hufgpu_sub_index_bytes(uint64_t n, uint64_t blocksize);
int hufgpu_encode_sub(hufgpu_ctx_t *ctx, const void *d_in, uint64_t n, uint64_t blocksize,
                      void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                      void *d_sub_index, uint64_t *out_len, void *stream);
int hufgpu_decode_sub(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                      const uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                      const void *d_sub_index, void *d_out, uint64_t out_cap, uint32_t flags,
                      uint64_t *raw_len, void *stream);

/*
 * BATCHES: many independent inputs in one launch sequence.  A call per input costs tens of microseconds of host API
 * whatever the input holds; a batch encodes (decodes) every block of every input with the launches of one call.
 * The inputs lie back to back in one device buffer: item i starts at the sum of the lengths in front of it, at any
 * byte alignment.  Item lengths are a HOST array (the grid sizes depend on them); an item of length 0 has no blocks
 * and an empty stream (src/encoder.c:288).  Blocks are independent and every header stores its own block_len, so
 * the items' streams back to back are ONE valid stream: hufgpu_decode() of the whole of it gives the inputs back to
 * back.  Host arrays may be reused as soon as a call returns.  There is no CPU path: the two batch calls need a
 * context; hufgpu_batch_geometry() is plain arithmetic and works without a GPU.
 *
 *   hufgpu_batch_geometry : for nitems lengths and a blocksize as in hufgpu_encode() (0 = every item is one block):
 *                           *nblocks = the sum of hufgpu_block_count(len_i, blocksize), *row_blocksize = the longest
 *                           block, min(blocksize or infinity, max len_i), *out_bound = the sum of
 *                           hufgpu_encode_bound(len_i, blocksize), *sub_index_bytes = the size of a batch sub-index:
 *                           nblocks rows laid out like hufgpu_sub_index_bytes(), each sized for row_blocksize symbols.
 *                           Outputs may be NULL; item_lens may be NULL only for nitems = 0.
 *   hufgpu_encode_batch   : item i's stream d_out[o[i], o[i+1]) is byte for byte what hufgpu_encode() writes for that
 *                           item alone with the same blocksize.  d_block_offsets (optional, nblocks + 1 words): the
 *                           concatenation of the items' own block indexes, each shifted to its absolute place in d_out
 *                           (the last word = the batch's length).  d_item_offsets (optional, nitems + 1 words) and
 *                           item_offsets (optional HOST array, nitems + 1): o[].  With item_offsets the call
 *                           synchronises; without it, it only enqueues (two such calls back to back on one context are
 *                           safe: the tables are staged per call).  d_sub_index (optional, 8-byte aligned,
 *                           sub_index_bytes): block b's row holds the entries hufgpu_encode_sub() writes for that block
 *                           when its item is encoded alone - the rows are laid out by (nblocks, row_blocksize) instead
 *                           of (n, blocksize).  Blocks of HUFGPU_BATCH_CHUNKED_FROM (2 MiB) and more (row_blocksize >= it)
 *                           are encoded item by item, one synchronisation per item, with the same output; such a
 *                           batch takes no sub-index: a non-NULL d_sub_index returns HUF_ERROR_INVALID_ARGUMENT.
 *   hufgpu_decode_batch   : item i = blocks [item_blocks[i], item_blocks[i+1]) of the stream (item_blocks[0] = 0, host,
 *                           non-decreasing), its slot = d_out[out_offsets[i], out_offsets[i+1]) (host, non-decreasing).
 *                           item_errs[i], item_raw_lens[i] and the bytes of the slot are what
 *                             hufgpu_decode(ctx, d_stream, stream_len, d_block_offsets + item_blocks[i],
 *                                           item_blocks[i+1] - item_blocks[i], d_out + out_offsets[i],
 *                                           out_offsets[i+1] - out_offsets[i], flags, &raw, ...)
 *                           returns: the reference's partial delivery from a failing block, HUF_ERROR_MEMORY_ALLOCATION
 *                           for a slot that is too small.  A damaged or oversized item never moves, shortens or corrupts
 *                           another item's output, and bytes of d_out outside the decoded bytes of every slot are never
 *                           written.  d_sub_index / row_blocksize (optional): from the batch encode; the results are
 *                           those of the same call without them for ANY content of the buffer (as hufgpu_decode_sub()).
 *                           Synchronous.  Returns HUF_ERROR_SUCCESS when every item decoded, else the error of the
 *                           first failing item in item order.  Argument errors return before anything is enqueued.
 */
#define HUFGPU_BATCH_CHUNKED_FROM ((uint64_t)1 << 21)   /* = HUF_CHUNKED_FROM: row_blocksize from here on goes item by item, no sub-index */
int hufgpu_batch_geometry(uint64_t nitems, const uint64_t *item_lens, uint64_t blocksize, uint64_t *nblocks,
                          uint64_t *row_blocksize, uint64_t *out_bound, uint64_t *sub_index_bytes);
int hufgpu_encode_batch(hufgpu_ctx_t *ctx, const void *d_in, uint64_t nitems, const uint64_t *item_lens,
                        uint64_t blocksize, void *d_out, uint64_t out_cap, uint64_t *d_block_offsets,
                        uint64_t *d_item_offsets, void *d_sub_index, uint64_t *item_offsets, void *stream);
int hufgpu_decode_batch(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len, const uint64_t *d_block_offsets,
                        uint64_t nitems, const uint64_t *item_blocks, const uint64_t *out_offsets,
                        const void *d_sub_index, uint64_t row_blocksize, void *d_out, uint32_t flags,
                        int32_t *item_errs, uint64_t *item_raw_lens, void *stream);

/*
 * RANGES: bytes [lo, hi) of the original data out of one indexed stream, many ranges in one launch sequence.  A call costs
 * tens of microseconds whatever it carries; fetching ten thousand records out of a compressed column is one call.
 * Raw positions are positions in what hufgpu_decode() of the whole stream delivers: block b covers [P[b], P[b+1]), P = the
 * exclusive sums of the block_len header fields.  No blocksize is assumed, so an index from hufgpu_block_index(), the
 * stream of a batch (short last blocks per item) and a hand-made stream all work; a range's first and last block are
 * found on the device by binary search in P.  Blocks are independent, positions inside a block are not: the blocks at
 * a range's edges are decoded WHOLE (a start inside a block cannot be verified without decoding what lies in front of
 * it), so with the reference's blocksize = 0 - one block - a range costs a full decode.  There is no CPU path.
 *
 *   range i         : [range_lo[i], range_hi[i]), lo <= hi (host arrays).  Ranges may overlap, repeat and come in any
 *                     order.  Its slot is d_out[out_offsets[i], out_offsets[i+1]) (host, nranges + 1, non-decreasing).
 *                     A range that reaches past the end of the data is cut there: range_raw_lens[i] says so, with
 *                     HUF_ERROR_SUCCESS (a read at the end of a file).  A slot shorter than the cut range gives that
 *                     range HUF_ERROR_MEMORY_ALLOCATION and nothing is written into it.
 *   what is decoded : only blocks that a range touches.  Damage in the PAYLOAD of an untouched block is never seen.  A
 *                     HEADER that does not parse (what hufgpu_decode() reports for the block before it looks at the
 *                     payload) hides the positions of everything behind it: a range that ends in front of the first
 *                     such block is served, every other range fails with that header's error and delivers the bytes
 *                     it has in front of that block.
 *   per range       : range_errs[i] = the error of the first failing touched block in stream order, range_raw_lens[i]
 *                     = the range's bytes in front of that block plus, for HUF_ERROR_READ_WRITE / _BTREE_CORRUPTED,
 *                     the part of what src/decoder.c:69-91 delivers of the failing block (decoded once more, in
 *                     order, its record as the whole input) that lies inside the range.  A failing range never moves,
 *                     shortens or corrupts another range's slot.  Nothing outside the first (cut length) bytes of
 *                     the slots is ever written; inside a FAILING range's slot, what lies behind the delivered bytes
 *                     is unspecified (as behind *raw_len of hufgpu_decode()).
 *   routing         : a block that lies wholly inside exactly one range and is touched by no other is decoded straight
 *                     into that slot.  Every other touched block - a cut edge, a block several ranges share - is
 *                     decoded once into a scratch area of the context (staged blocks x the longest of them; when it
 *                     cannot grow the call returns HUF_ERROR_MEMORY_ALLOCATION) and its pieces are copied to the slots.
 *   d_sub_index     : optional, with (raw_size, blocksize) as in hufgpu_decode_sub() (they must give nblocks blocks):
 *                     the touched blocks are decoded with the encoder's sub-index, verified as ever - the results are
 *                     those of the same call without it for ANY content of the buffer.  NULL: raw_size and blocksize
 *                     are not looked at.
 *
 * TILES (flags & HUFGPU_RANGES_TILES, with d_sub_index; without a sub-index the flag does nothing): the sub-index holds
 * the payload bit every tile of 2 048 symbols starts at, so a range can be decoded from the first tile that holds one of
 * its bytes - the cost of a range follows the range, not the block, and a stream of ONE block (blocksize = 0) has random
 * access.  That a tile's recorded start is where the in-order decoder arrives cannot be verified without decoding what
 * lies in front of it (Huffman codes resynchronise: a false start can pass every later check), so the promise "for ANY
 * content of the buffer" above cannot hold for a partial decode.  It stays as it is for every call without the flag.  By
 * setting the flag the caller states that d_sub_index is the sub-index of THIS stream: from hufgpu_encode_sub(), a batch
 * encode, hufgpu_update_ranges(), hufgpu_append() / hufgpu_truncate(), or one of the three builders below.  Then:
 *   1. With the stream's own sub-index, every range's bytes, error and delivered count are those of the same call
 *      without the flag, as long as the payload in front of the range's first touched tile, inside that tile's block,
 *      is as the encoder wrote it.
 *   2. Damage in the payload of UNTOUCHED tiles of a touched block goes unnoticed, just as damage in untouched blocks
 *      does without the flag; the touched tiles' bytes are delivered with success.
 *   3. Damage inside a touched tile, or in the header or tree of a touched block, gives what the call without the flag
 *      gives: every group of 32 symbols of a touched tile is decoded from its true start - to what the in-order decoder
 *      sees there - and must take exactly its recorded bits; the claimed code lengths are checked against the stream's
 *      tree.  When a check fails, the call is served again by the whole-block route, which produces the reference's
 *      error and partial delivery.
 *   4. With any OTHER content of d_sub_index: no memory fault, no byte outside the first (cut length) bytes of the slots
 *      is written, every walk stays inside the tree and the payload, the call returns.  Bytes inside a slot MAY BE WRONG
 *      WITH HUF_ERROR_SUCCESS - but only if every check happens to hold: the tile start inside the payload, the start
 *      plus the sum of the tile's 64 bit counts equal to the next tile's recorded start, every group of the tile
 *      exactly its bits, the code lengths those of the tree.
 *   5. Without the flag, or without d_sub_index, nothing changes.
 * Which blocks go by tiles: a touched block that is not decoded straight into a slot, whose block_len is the layout's
 * min(blocksize, raw_size - b * blocksize), whose tree has more than one leaf and over which all ranges together make no
 * more (range, tile) pairs than the block has tiles - the tile route never decodes more symbols than the whole block
 * holds.  Every other block is routed as without the flag.  Tile-routed blocks use no scratch area.  A call in which no
 * check fails waits as often as the call without the flag; one in which a check fails is run a second time without it.
 * hufgpu_ranges_counters() says which way the blocks went.
 *
 * Synchronous.  Returns HUF_ERROR_SUCCESS or the error of the first failing range in range order.  Argument errors
 * (lo > hi, decreasing out_offsets, NULL host arrays, a misaligned or mis-sized sub-index, no context) return
 * HUF_ERROR_INVALID_ARGUMENT before anything is enqueued; nranges = 0 is success.  hufgpu_decode_counters() after the
 * call counts the blocks of this call that went to the exact decoder.
 */
int hufgpu_decode_ranges(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                         const uint64_t *d_block_offsets, uint64_t nblocks,
                         uint64_t nranges, const uint64_t *range_lo, const uint64_t *range_hi,
                         const uint64_t *out_offsets,
                         const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                         void *d_out, uint32_t flags,
                         int32_t *range_errs, uint64_t *range_raw_lens, void *stream);

/*
 * GATHER: records whose positions are on the device - an index lookup, a sampler or a join produced them one kernel
 * earlier.  hufgpu_decode_ranges() takes host arrays and waits for the device twice; this call reads nothing of the
 * records on the host, never waits, writes no host memory and only enqueues on `stream` (NULL = the context's): the
 * host knows nrecords and max_len - the sizes of the caller's arrays - and nothing else.  On the device the records are
 * grouped by block, so a block's tables are built once however many records fall into it.  There is no CPU path.
 *
 *   record i      : bytes [d_pos[i], d_pos[i] + len_i) of the original data, len_i = d_len[i] or, with d_len = NULL,
 *                   max_len for every record.  Its slot is d_out + i * out_stride (out_stride >= max_len; any alignment
 *                   of d_out, any stride).  Records may overlap, repeat and come in any order.  A record that reaches
 *                   past raw_size is cut there: d_raw_lens[i] (optional) says so, with status 0.
 *   positions     : are the layout's: block b holds [b * blocksize, b * blocksize + min(blocksize, raw_size - b *
 *                   blocksize)) - for a stream of hufgpu_encode_sub() the positions of the original data.  No header is
 *                   read to find a record's blocks; a touched block whose header gives another length is not served.
 *                   (A batch's stream with (nblocks * row_blocksize, row_blocksize): block b's bytes are addressed from
 *                   b * row_blocksize, records that touch an item's short last block are not served.)
 *   d_sub_index   : required, with (raw_size, blocksize) as in hufgpu_decode_sub().  The call carries the statement of
 *                   HUFGPU_RANGES_TILES: the sub-index is THIS stream's own.  Points 1-4 of the TILES paragraph above
 *                   hold word for word, with "slot" = the first len_i bytes of slot i; no other byte is ever written.
 *   d_errs[i]     : 0 - the record's bytes are delivered and are those of hufgpu_decode_ranges() with the flag.
 *                   HUF_ERROR_INVALID_ARGUMENT - len_i > max_len; nothing is written for it.
 *                   HUF_ERROR_READ_WRITE - a check of the tile route failed in a block the record touches (the tile
 *                   start outside the payload, the bit sums, a group not taking its bits, the claimed lengths not the
 *                   tree's), or such a block cannot be served by tiles (its header does not parse under `flags`, its
 *                   block_len is not the layout's, tree_len reaches past the block's record).
 *                   Any non-zero status means "not served here": hufgpu_decode_ranges() without the flag gives the
 *                   authoritative bytes and error; bytes inside that record's cut length are unspecified.  There is no
 *                   fail-over inside the call (it would need a host decision).  A record over several blocks gets the
 *                   worst status of its parts; the statuses are zeroed by the call's first launch.
 *   one-symbol blocks (a tree of one leaf; the encoder writes no sub-index rows for them) ARE served: once the header
 *                   is checked and the record's own payload bits are seen to be 0, the slot part is a fill.
 *   flags         : HUFGPU_RELAXED_TREE as for hufgpu_decode().
 *
 * Argument errors - no context, a NULL d_stream / d_block_offsets / d_pos / d_out / d_errs, out_stride < max_len, a
 * missing or misaligned sub-index, (raw_size, blocksize) that do not give nblocks, more than 2^32 - 1 (record, block)
 * parts by the bound nrecords * ((max_len + blocksize - 2) / blocksize + 1) - return HUF_ERROR_INVALID_ARGUMENT before
 * anything is enqueued.  nrecords = 0 and max_len = 0 are success with nothing enqueued.  The workspaces are the
 * context's, sized by those bounds and doubled when they grow (only then does the call wait); two calls back to back on
 * one stream are safe, calls on different streams of one context are not.
 */
int hufgpu_gather(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                  const uint64_t *d_block_offsets, uint64_t nblocks,
                  const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                  uint64_t nrecords, const uint64_t *d_pos, const uint32_t *d_len, uint32_t max_len,
                  void *d_out, uint64_t out_stride,
                  int32_t *d_errs, uint32_t *d_raw_lens, uint32_t flags, void *stream);

/*
 * FIND BYTES: the calls above take positions; this one produces them.  For a set of byte values it reports how many bytes of
 * each block are in the set and at which positions of the original data they lie - the newlines of a compressed log, the
 * separators of a table - straight from stream, block index and sub-index: every block is decoded once, no decoded byte
 * is written to device memory (a match mask of one bit per byte, an eighth of the data, lives in a context workspace),
 * and like hufgpu_gather() the call never waits, writes no host memory and only enqueues on `stream` (NULL = the
 * context's): find_bytes -> a device op -> gather is a pipeline without a host wait.  There is no CPU path.
 *
 *   set           : a HOST array of 32 bytes, a 256-bit set: byte value v is looked for when bit v & 7 of set[v >> 3] is 1.
 *                   It is read before the call returns.  The empty set and the full set are valid.
 *   positions     : are the layout's, as in hufgpu_gather(): block b holds [b * blocksize, b * blocksize + min(blocksize,
 *                   raw_size - b * blocksize)), blocksize = 0 means one block; (raw_size, blocksize) must give nblocks.  A
 *                   block whose header gives another block_len is not served.  (A batch's stream with (nblocks *
 *                   row_blocksize, row_blocksize): full blocks are served and addressed from b * row_blocksize, the items'
 *                   short last blocks are reported not served.)
 *   d_sub_index   : required, with (raw_size, blocksize) as in hufgpu_decode_sub().  The caller vouches for NOTHING: every
 *                   block is walked from payload bit 0 through every tile, so checks (a), (b), (c) of hufgpu_decode_sub()
 *                   close their induction, and for ANY content of the buffer a block is either served exactly or
 *                   reported as not served.
 *   d_block_errs  : required, nblocks words.  0 - served.  HUF_ERROR_READ_WRITE - "not served here": the header does not
 *                   parse under `flags`, block_len is not the layout's, the claimed code lengths are not the tree's, one
 *                   of (a) / (b) / (c) fails, a walk leaves the tree or the payload.  hufgpu_decode_sub() gives the
 *                   authoritative bytes and error for such a block; there is no fail-over inside the call (it would
 *                   need a host decision).  The statuses are zeroed by the call's first enqueued operation.
 *   d_block_counts: optional, nblocks words: the matches in block b; 0 for a block that is not served.
 *   d_pos         : may be NULL when pos_cap = 0.  The positions of the matches of all SERVED blocks in ascending order:
 *                   the first min(total, pos_cap) of them are written and nothing else - words from d_totals[1] on are
 *                   untouched.
 *   d_totals      : required, 4 words: [0] matches in served blocks (exact whatever pos_cap is), [1] positions written,
 *                   [2] blocks not served, [3] 0.  One read says whether the answer is complete.
 *   one-symbol blocks (a tree of one leaf; the encoder writes no sub-index rows for them) ARE served: the header is
 *                   checked, the block's block_len payload bits are seen to be 0, the count is block_len or 0.
 *   flags         : HUFGPU_RELAXED_TREE as for hufgpu_decode().
 *
 * Argument errors - no context, a NULL d_stream / d_block_offsets / set / d_totals / d_block_errs, pos_cap > 0 with a NULL
 * d_pos, a missing or misaligned sub-index, (raw_size, blocksize) that do not give nblocks (or more than 2^31 - 1 tiles of
 * 2 048 bytes) - return HUF_ERROR_INVALID_ARGUMENT before anything is enqueued.  nblocks = 0 (with raw_size = 0) is
 * success: d_totals is zeroed and nothing else is enqueued.  The workspaces are the context's, sized by the layout and
 * doubled when they grow (only then does the call wait); two calls back to back on one stream are safe, calls on different
 * streams of one context are not.  The enqueue-only calls - this one and the rest of the search family, hufgpu_gather(),
 * hufgpu_histogram(), and hufgpu_encode() / hufgpu_encode_sub() / hufgpu_decode() / hufgpu_decode_sub() without their host
 * result pointer - may be captured into a graph on a non-default stream once a call of the same sizes has made the
 * workspaces: the graph carries the whole call and may be replayed on other contents of the same buffers.  "Never waits"
 * is the call's own promise: the first launch of one of its kernels on a stream that has not run it may wait inside the
 * runtime (seen: 1.5 ms, once more than 20 ms, for the decoders that use scratch memory).
 */
int hufgpu_find_bytes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                      const uint64_t *d_block_offsets, uint64_t nblocks,
                      const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                      const uint8_t set[32],
                      uint64_t *d_pos, uint64_t pos_cap,
                      uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                      uint32_t flags, void *stream);

/*
 * FIND PATTERN: grep for one string.  Where hufgpu_find_bytes() reports single bytes of a set, this call reports where a
 * PATTERN of 1 to HUFGPU_FIND_PATTERN_MAX bytes starts in the original data - the lines of a compressed log that hold
 * "ERROR" or a request id - again straight from stream, block index and sub-index, decoding every block once, only
 * enqueueing on `stream` and never waiting.  Besides the match mask the context keeps at most 126 bytes of every tile of
 * 2 048 (its first and last pattern_len - 1 bytes, 6 % of the data) in a workspace that hufgpu_find_bytes() never
 * allocates; no other decoded byte reaches device memory.  There is no CPU path.
 *
 * Everything is hufgpu_find_bytes()' word for word - positions, d_sub_index (the caller vouches for NOTHING), d_block_errs,
 * d_totals, d_pos untouched from d_totals[1] on, one-symbol blocks served, batch geometry, flags, nblocks = 0, workspaces
 * doubled only when they grow, the argument errors (worded "find_pattern: ...") - but for this:
 *
 *   pattern       : a HOST array of pattern_len bytes, 1 <= pattern_len <= HUFGPU_FIND_PATTERN_MAX, read before the call
 *                   returns.  A NULL pattern, a length of 0 or one above the maximum is HUF_ERROR_INVALID_ARGUMENT before
 *                   anything is enqueued and before the context is looked at.
 *   a match       : a position p of the original data with data[p .. p + pattern_len) == pattern.  ALL occurrences are
 *                   reported, overlapping ones included ("aa" in "aaaa" matches at 0, 1 and 2), in ascending order, each
 *                   at its START; it counts for the block that holds its start: d_block_counts[b] = matches that start
 *                   in block b, wherever they end.  Nothing matches past raw_size.
 *   blocks that are not served: a match is reported only when EVERY block it touches is served.  A start in a served
 *                   block whose bytes run on into a block that is not served is no match and is counted nowhere;
 *                   d_totals[2] and d_block_errs say which seams are open.  This is the ONE place where this call's
 *                   answer for a served block depends on its neighbour: with d_totals[2] = 0 the answer is complete,
 *                   otherwise up to pattern_len - 1 starts in front of every block that is not served are missing
 *                   besides that block's own.
 *   pattern_len 1 : gives exactly what hufgpu_find_bytes() gives for the set of that one value.
 */
#define HUFGPU_FIND_PATTERN_MAX 64
int hufgpu_find_pattern(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                        const uint64_t *d_block_offsets, uint64_t nblocks,
                        const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                        const uint8_t *pattern, uint32_t pattern_len,
                        uint64_t *d_pos, uint64_t pos_cap,
                        uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                        uint32_t flags, void *stream);

/*
 * FIND RECORDS: grep for lines.  Where hufgpu_find_pattern() reports where a string starts, this call reports the whole
 * RECORDS that hold it - the lines of a compressed log that say "ERROR" - as a start and a length each, every record once
 * however many matches it has, in exactly the form hufgpu_gather() takes: find_records -> gather is a pipeline with no
 * device op of the caller's in between and no host wait.  The stream is walked ONCE: the match mask of
 * hufgpu_find_pattern() and a mask of the delimiters come from the same decoded tile, and the records are made from the two
 * masks on the device (kernels/find.hpp).  Two more masks of one bit per byte and a count per tile live in workspaces that
 * the two other find calls never allocate; no decoded byte but the pattern call's edges reaches device memory.  There is
 * no CPU path.
 *
 * Everything is hufgpu_find_pattern()'s word for word - positions, d_sub_index (the caller vouches for NOTHING),
 * d_block_errs zeroed by the first enqueued operation, one-symbol blocks served, batch geometry, flags, nblocks = 0,
 * workspaces doubled only when they grow, enqueue-only without a host write or a wait, the argument errors (worded
 * "find_records: ...") - but for this:
 *
 *   delim_set     : a HOST array of 32 bytes in hufgpu_find_bytes()' encoding, read before the call returns.  The bytes
 *                   whose value is in it cut the original data into records.  A record is [s, e): s = 0 or byte s - 1 is a
 *                   delimiter; e is the first delimiter at or behind s, or raw_size.  The delimiter is not part of the
 *                   record.  Empty records exist and never match.  The empty set is valid: the data is one record.  NULL
 *                   is HUF_ERROR_INVALID_ARGUMENT.
 *   pattern       : as hufgpu_find_pattern()'s, 1 to HUFGPU_FIND_PATTERN_MAX bytes.  A pattern that holds a byte of
 *                   delim_set is HUF_ERROR_INVALID_ARGUMENT, found on the host before the context is looked at: grep cannot
 *                   match a newline either, and so every match lies inside one record.
 *   d_rec_pos, d_rec_len, rec_cap, max_len: the records that hold at least one match, each ONCE, ascending by start:
 *                   d_rec_pos[i] = s and d_rec_len[i] = min(e - s, clip), clip = max_len, or 2^32 - 1 when max_len = 0.
 *                   The first min(total, rec_cap) entries are written and nothing behind them.  Both may be NULL when
 *                   rec_cap = 0 and both are required otherwise.  (d_rec_pos, d_rec_len, max_len) go into hufgpu_gather()
 *                   as (d_pos, d_len, max_len) unchanged.
 *   d_totals      : [0] matching records (exact whatever rec_cap is), [1] records written, [2] blocks not served,
 *                   [3] WRITTEN records longer than clip.
 *   d_block_counts: optional; the reported records that START in block b, wherever they end.
 *   blocks that are not served: a record is reported only when its extent is KNOWN: every block that holds a byte of
 *                   [max(s - 1, 0), min(e, raw_size - 1)] - the record, the delimiter in front of it and the one that ends
 *                   it - is served.  Any other record is reported and counted nowhere.  With d_totals[2] = 0 the answer is
 *                   complete; otherwise the records that touch a block with a non-zero status are missing, and nothing
 *                   else is.  This replaces hufgpu_find_pattern()'s seam rule: a match inside a known record touches served
 *                   blocks only.
 */
int hufgpu_find_records(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                        const uint64_t *d_block_offsets, uint64_t nblocks,
                        const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                        const uint8_t delim_set[32], const uint8_t *pattern, uint32_t pattern_len,
                        uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                        uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                        uint32_t flags, void *stream);

/*
 * FIND CLASSES: grep -i, a hex digit, a don't-care byte.  The two calls above look for ONE string; in these two every
 * position of the pattern is a SET of byte values - "error" in any case is five classes of two values, a request id is
 * "req-" and eight classes of the sixteen hex digits, a byte that may be anything is the full class - and one call, one
 * walk of the stream, answers what took a call per spelling before (and what hufgpu_find_records() could not answer at
 * all without reporting a line once per spelling).  The tile walk, its checks, the seams, the scans, the records and the
 * workspaces are those of the literal calls; the class table (2 KiB) travels with the launches' own arguments, so no
 * workspace is added and calls back to back need no care.  There is no CPU path.
 *
 *   classes       : a HOST array classes[pattern_len][32], read before the call returns: class k is the 32 bytes at
 *                   classes + 32 * k, a 256-bit set in hufgpu_find_bytes()' encoding - byte value v is in class k when bit
 *                   v & 7 of classes[32 * k + (v >> 3)] is 1.  1 <= pattern_len <= HUFGPU_FIND_PATTERN_MAX.
 *   a match       : a position p of the original data with data[p + k] in class k for every k < pattern_len.  ALL
 *                   occurrences are reported, overlapping ones included, in ascending order, each at its START; a match
 *                   counts for the block that holds its start.  Nothing matches past raw_size.
 *
 * hufgpu_find_classes() is hufgpu_find_pattern()'s contract word for word, with `classes` in the place of `pattern` -
 * positions, d_sub_index (the caller vouches for NOTHING), d_block_errs zeroed by the first enqueued operation, d_pos
 * untouched from d_totals[1] on, d_totals, d_block_counts, one-symbol blocks served (they match iff their one value is in
 * every class), the seam rule (a match is reported only when EVERY block it touches is served), batch geometry, flags,
 * nblocks = 0, workspaces doubled only when they grow, enqueue-only without a host write or a wait - and
 * hufgpu_find_records_classes() is hufgpu_find_records()' in the same way: delim_set, d_rec_pos / d_rec_len / rec_cap /
 * max_len, d_totals[3], the known-extent rule.  The argument errors are worded "find_classes: ..." and
 * "find_records_classes: ...".  Found on the host, before anything is enqueued and before the context is looked at, and
 * HUF_ERROR_INVALID_ARGUMENT are besides the literal calls' errors:
 *
 *   - a NULL `classes`, a pattern_len of 0 or above the maximum;
 *   - an EMPTY class: it matches nothing and is a caller's mistake.  The message names the position;
 *   - for the records call, a class that holds a byte of delim_set (the message names the position and the value): grep's
 *     `.` does not match a newline either.  The caller subtracts the delimiters from a wide class - the full class with a
 *     non-empty delim_set is this error, with the empty delim_set it is valid - and so every match lies inside one
 *     record, which the record kernels rely on.
 *
 * Two identities:
 *   classes of one value each give exactly what hufgpu_find_pattern() / hufgpu_find_records() give for that string;
 *   pattern_len = 1 gives exactly what hufgpu_find_bytes() gives for that set.
 *
 * By construction the cost of a class call depends on pattern_len alone, not on the data and not on how wide the classes
 * are (kernels/find.hpp: one table look-up per byte and start, 32 + pattern_len - 1 a lane of 32 bytes): a first class of
 * [a-z], which would make nearly every start a candidate of a verify-by-candidate matcher, costs what any other class
 * pattern of that length costs.  What a class call costs next to hufgpu_find_pattern() is measured in DESIGN.md 5.16.
 */
int hufgpu_find_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                        const uint64_t *d_block_offsets, uint64_t nblocks,
                        const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                        const uint8_t *classes, uint32_t pattern_len,
                        uint64_t *d_pos, uint64_t pos_cap,
                        uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                        uint32_t flags, void *stream);
int hufgpu_find_records_classes(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                const uint64_t *d_block_offsets, uint64_t nblocks,
                                const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                const uint8_t delim_set[32], const uint8_t *classes, uint32_t pattern_len,
                                uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                                uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                uint32_t flags, void *stream);

/*
 * FIND ANY: grep -e ERROR -e FATAL -e panic, grep -F -f words.txt, grep -E 'timeout|refused|reset'.  The two calls above
 * look for ONE class pattern; these two look for ANY of several - ALTERNATIVES - in one walk of the stream.  With a call per
 * alternative the positions cost a walk each and a merge of the position lists, and the records cannot be had at all
 * without a line that holds two alternatives coming back twice.  The tile walk, its checks, the seams, the scans, the
 * records and the workspaces are those of the class calls - an any-of call grows what a class call of the LONGEST
 * alternative's length grows, no workspace is added -, and the table travels with the launches' own arguments.  There is no
 * CPU path.
 *
 *   an alternative: what hufgpu_find_classes() calls a pattern: 1 to HUFGPU_FIND_PATTERN_MAX positions, each a set of byte
 *                   values.  A literal is classes of one value each, `-i` classes of two.
 *   n_alts        : how many there are, n_alts >= 1.  Their lengths sum to at most HUFGPU_FIND_PATTERN_MAX (so n_alts is
 *                   at most that as well): the alternatives share the 64 bits of one matcher state.
 *   alt_lens      : a HOST array of n_alts lengths, read before the call returns.
 *   classes       : a HOST array classes[alt_lens[0] + alt_lens[1] + ...][32], read before the call returns: the classes
 *                   of alternative 0 in hufgpu_find_classes()' encoding, then those of alternative 1, and so on.
 *   a match       : a position p of the original data at which AT LEAST ONE alternative j lies: data[p + k] is in class k
 *                   of j for every k < len_j, p + len_j <= raw_size, and every block that [p, p + len_j) touches is
 *                   served.  A start is reported ONCE however many alternatives lie there ("ab" and "abc"), in ascending
 *                   order; it counts for the block that holds p.  Each alternative has its own seam rule: when the longer
 *                   of two reaches into a block that is not served and the shorter does not, the start is reported.
 *   WHICH alternative lies at a reported start is NOT reported: the kernels behind the matcher see one bit a start.  A
 *                   caller who needs it reads the bytes with hufgpu_gather() and looks.
 *
 * hufgpu_find_any() is hufgpu_find_pattern()'s contract word for word with this meaning of a match - d_sub_index (the
 * caller vouches for NOTHING), d_block_errs zeroed by the first enqueued operation, d_pos untouched from d_totals[1] on,
 * d_totals[0..3], d_block_counts, pos_cap, one-symbol blocks served (an alternative lies there iff the one value is in each
 * of its classes), batch geometry, flags, nblocks = 0, enqueue-only without a host write or a wait - and
 * hufgpu_find_records_any() is hufgpu_find_records()' with "holds a match" meaning "holds a match of any alternative":
 * each record is reported once, delim_set, d_rec_pos / d_rec_len / rec_cap / max_len, d_totals[3] and the known-extent
 * rule are the same.  The argument errors are worded "find_any: ..." and "find_records_any: ...".  Found on the host, before
 * anything is enqueued and before the context is looked at, and HUF_ERROR_INVALID_ARGUMENT are besides the older calls'
 * errors:
 *
 *   - a NULL `classes` or `alt_lens`; an n_alts of 0 or above HUFGPU_FIND_PATTERN_MAX;
 *   - an alternative of length 0 (the message names the alternative): it would lie everywhere;
 *   - lengths that sum to more than HUFGPU_FIND_PATTERN_MAX (the message names the total); `classes` is not read then;
 *   - an EMPTY class (the message names the alternative and the position in it);
 *   - for the records call, a class that holds a byte of delim_set (alternative, position and value are named): every
 *     match lies inside one record, which the record kernels rely on.
 *
 * Identities: ONE alternative gives exactly what hufgpu_find_classes() / hufgpu_find_records_classes() give for it; n
 * alternatives of one position give what hufgpu_find_bytes() gives for the union of their sets; K alternatives give the
 * sorted union, without duplicates, of what K class calls give.
 *
 * The cost follows the LONGEST alternative's length as a class call's follows pattern_len, plus a few vector operations a
 * byte for the test of the start bits; it does not depend on the data, on how wide the classes are or - but for the seam
 * kernel's few starts a tile - on how many alternatives there are.  Measured in DESIGN.md 5.17.
 */
int hufgpu_find_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                    const uint64_t *d_block_offsets, uint64_t nblocks,
                    const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                    const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                    uint64_t *d_pos, uint64_t pos_cap,
                    uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                    uint32_t flags, void *stream);
int hufgpu_find_records_any(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                            const uint64_t *d_block_offsets, uint64_t nblocks,
                            const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                            const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                            uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t rec_cap, uint32_t max_len,
                            uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                            uint32_t flags, void *stream);

/*
 * FIND RECORDS, SELECTED: grep -v and grep -n.  hufgpu_find_records_any() reports the records that hold a match; this call
 * can report the records that hold NONE (grep -v DEBUG, grep -v -e heartbeat -e healthz) and, for either answer, WHICH
 * record each one is: the number of delimiters in front of it (grep -n prints that plus 1).  Both come from the two masks
 * that the one walk writes anyway - match starts and delimiters -; there is no second walk and no other matcher, and what
 * comes back goes into hufgpu_gather() unchanged.  The pattern arguments are the any-of form: one alternative of one-value
 * classes is a literal, one alternative is a class pattern.  There is no CPU path.
 *
 * The contract is hufgpu_find_records_any()'s word for word - delim_set, classes / alt_lens / n_alts, d_sub_index (the
 * caller vouches for NOTHING), d_block_errs, d_rec_pos / d_rec_len / rec_cap / max_len, d_totals[0..3], d_block_counts,
 * the known-extent rule, batch geometry, flags, nblocks = 0, enqueue-only without a host write or a wait, every argument
 * error (worded "find_records_select: ...") - but for this:
 *
 *   select        : 0 or HUFGPU_SELECT_INVERT.  Any other bit is HUF_ERROR_INVALID_ARGUMENT, found on the host before the
 *                   context is looked at; the message names the value.
 *   HUFGPU_SELECT_INVERT: the call reports the NON-EMPTY records [s, e), e > s, that hold no match of any alternative, each
 *                   once, ascending.  A record is reported only when its extent is KNOWN by hufgpu_find_records()' own rule:
 *                   every block that holds a byte of [max(s - 1, 0), min(e, raw_size - 1)] is served.  Inside a known record
 *                   every match is known, so a record whose extent is known lies in exactly ONE of the two answers, the
 *                   plain one or the inverted one, and a record whose extent is not known lies in neither.  EMPTY records
 *                   are never reported - grep -v prints empty lines, this call does not: an empty record has no byte of
 *                   its own, a final delimiter starts no record, and hufgpu_gather() has nothing to fetch for it.
 *                   (hufgpu_find_records_context(): the distances COUNT empty records, as grep counts empty lines; they are
 *                   still never reported, and as they are not in the inverted S they get no context of their own.)
 *                   d_totals[0..3], d_block_counts, rec_cap and max_len mean for the selected records what they mean for
 *                   the matching ones.
 *   d_rec_no      : optional, NULL or rec_cap entries (it may be NULL with rec_cap > 0, and is not looked at with
 *                   rec_cap = 0); written as d_rec_pos is: the first d_totals[1] entries and nothing behind them.
 *                   d_rec_no[i] is the number of delimiter bytes in [0, d_rec_pos[i]) - empty records count -, exact when
 *                   every block in front of the block that holds d_rec_pos[i] is served, and HUFGPU_REC_NO_UNKNOWN
 *                   otherwise: a block that is not served hides its delimiters.  The record itself is still reported.
 *                   With and without HUFGPU_SELECT_INVERT.
 *
 * The identity: select = 0 and d_rec_no = NULL give exactly what hufgpu_find_records_any() gives, by the same launches.
 * HUFGPU_SELECT_INVERT adds one kernel over the record masks (at most one look-up of O(log tiles) a tile, whatever the
 * data), d_rec_no one word of workspace, a kernel of a thread a block and a second instance of the last kernel; the seven
 * older calls launch what they always did.  Measured in DESIGN.md 5.18.
 */
#define HUFGPU_SELECT_INVERT   1u
#define HUFGPU_REC_NO_UNKNOWN  (~(uint64_t)0)
int hufgpu_find_records_select(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                               const uint64_t *d_block_offsets, uint64_t nblocks,
                               const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                               const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                               uint32_t select,
                               uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint64_t rec_cap, uint32_t max_len,
                               uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                               uint32_t flags, void *stream);

/*
 * FIND RECORDS, WITH CONTEXT: grep -A / -B / -C.  hufgpu_find_records_select() reports the selected records; this call
 * reports the records AROUND them as well (grep -C 3 ERROR, grep -B 5 panic, grep -A 20 'stack trace'), from the masks
 * that the one walk has written anyway: the delimiters, the selected records' starts, and the scanned delimiter counts
 * that give every start its number.  Context is a dilation of the selected records' mask in record-NUMBER space: one more
 * kernel over the masks, no second walk, no other matcher, and what comes back goes into hufgpu_gather() unchanged.  There
 * is no CPU path.
 *
 * The contract is hufgpu_find_records_select()'s word for word - the pattern forms, delim_set, `select` and its check first
 * of all, d_rec_no, rec_cap, max_len, d_totals[0..3], d_block_counts, d_block_errs, the known-extent rule, flags,
 * nblocks = 0, enqueue-only without a host write or a wait, every argument error (worded "find_records_context: ...") -
 * but for this:
 *
 *   S             : the records that hufgpu_find_records_select() reports for the same arguments: non-empty, extent known,
 *                   holding a match - or holding none under HUFGPU_SELECT_INVERT.  A record's NUMBER no(r) is the count of
 *                   delimiter bytes in front of its start; empty records count.
 *   before, after : any uint32_t.  The call reports, each once and ascending, every record of S and every non-empty record
 *                   c whose extent is known for which S holds an m with no(m) - before <= no(c) < no(m) or
 *                   no(m) < no(c) <= no(m) + after - and that only when every block that holds a byte from the start of the
 *                   earlier of the two records to the end of the later one is served.  A block that is not served hides its
 *                   delimiters, so no distance is measured across it: a record is left out on doubt, never reported wrongly.
 *                   S itself is always reported in full: the answer contains the select call's for any before, after.
 *                   0xffffffff in both reports every non-empty record of known extent, whenever S is not empty and every
 *                   block is served.
 *   EMPTY records : distances count them, as grep counts empty lines, but they are never reported (hufgpu_gather() has
 *                   nothing to fetch for them), and under HUFGPU_SELECT_INVERT they are not in S either, so they get no
 *                   context of their own: the records around an empty line are not reported for its sake.
 *   d_rec_sel     : optional, NULL or rec_cap bytes (not looked at with rec_cap = 0), written as d_rec_pos is: 1 when record
 *                   i is in S, 0 when it is context only - grep's ':' and '-'.  grep's "--" between two groups follows from a
 *                   gap in d_rec_no.
 *   d_totals[0..3], d_block_counts, rec_cap and max_len mean for the REPORTED records what they mean for the selected ones.
 *
 * The identity: before = after = 0 and d_rec_sel = NULL enqueue exactly what hufgpu_find_records_select() enqueues, and the
 * eight older calls launch what they always did.  The cost does not follow before or after: a tile of 2048 bytes costs at
 * most three look-ups of O(log tiles) and a bit scan each - the end of its last record, the nearest selected record in
 * front of it and the nearest one behind it - whatever the data and the distances are (kernels/find.hpp,
 * find_rec_ctx_kernel).  A distance that is not 0 grows one workspace more: a second record mask, its tile counts and a
 * scan.  Measured in DESIGN.md 5.20.
 */
int hufgpu_find_records_context(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                const uint64_t *d_block_offsets, uint64_t nblocks,
                                const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                uint32_t select, uint32_t before, uint32_t after,
                                uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                                uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                uint32_t flags, void *stream);

/*
 * FIND, ANCHORED: grep -w, grep -x, '^' and '$'.  The forms of a search that look at the byte NEXT TO a match:
 * grep -w error (not "errors", not "stderror"), grep -x OK, grep '^2026-10-19', grep 'refused$'.  hufgpu_find_any_anchored()
 * is hufgpu_find_any() and hufgpu_find_records_anchored() is hufgpu_find_records_context() - the contracts hold word for
 * word: the pattern forms, d_sub_index (the caller vouches for NOTHING), every output, cap and total, `select`, d_rec_no,
 * before / after, d_rec_sel, the known-extent rule, flags, nblocks = 0, enqueue-only without a host write or a wait, every
 * argument error (worded "find_any_anchored: ..." and "find_records_anchored: ...") in the older calls' order - but for
 * which occurrences count.  One walk of the stream (two for the records call with HUFGPU_ANCHOR_WORD): the byte behind a
 * match is one more position an alternative in the matcher's table, the byte in front of it one AND of two masks that the
 * walk writes.  There is no CPU path.
 *
 *   delim_set     : D, the bytes that end a record; the positions call takes it behind n_alts and looks at it only with
 *                   HUFGPU_ANCHOR_BOL or HUFGPU_ANCHOR_EOL (NULL otherwise is fine).  The records call has its own, in the
 *                   place where hufgpu_find_records_context() has it, and there the caller's classes still may not hold a
 *                   delimiter.
 *   word_set      : W, the word bytes, 32 bytes in hufgpu_find_bytes()' encoding ([A-Za-z0-9_] for grep's); looked at only
 *                   with HUFGPU_ANCHOR_WORD.
 *   anchors       : 0 or an OR of the three bits below; grep -x is HUFGPU_ANCHOR_BOL | HUFGPU_ANCHOR_EOL.
 *   an occurrence : a pair (p, j) as hufgpu_find_any() defines a match of alternative j at p.  Its left neighbour is
 *                   L = data[p - 1], ABSENT when p = 0; its right neighbour is R = data[p + len_j], absent when
 *                   p + len_j = raw_size.  It QUALIFIES when every anchor that is asked for holds:
 *                     HUFGPU_ANCHOR_BOL   L is absent or L is in D
 *                     HUFGPU_ANCHOR_EOL   R is absent or R is in D
 *                     HUFGPU_ANCHOR_WORD  (L is absent or L is not in W) and (R is absent or R is not in W)
 *   what is reported: a start p once, ascending, when at least one alternative that lies there qualifies AND every block
 *                   that holds a byte of that alternative's tested span is served: [p, p + len_j), widened by one byte on
 *                   each side where a neighbour exists and an anchor tests it.  A start is left out on doubt, never reported
 *                   wrongly; each alternative has its own span (hufgpu_find_any()'s own seam rule).  The records call selects
 *                   on "holds a qualifying occurrence"; HUFGPU_SELECT_INVERT, d_rec_no, before / after, d_rec_sel, max_len,
 *                   the caps, d_totals[0..3], d_block_counts and the known-extent rule then apply unchanged.  EVERY
 *                   overlapping occurrence is tested, so a record qualifies when any occurrence in it does - what GNU grep
 *                   gives for patterns of fixed length: grep -w foo selects "foofoo foo".
 *   one-symbol blocks: served; an alternative lies inside one only if the one value is in each of its classes AND may stand
 *                   behind it.
 *
 * Found on the host, before anything is enqueued and before the context is looked at, behind the `select` check and
 * otherwise in the older calls' order, and HUF_ERROR_INVALID_ARGUMENT are besides the older calls' errors:
 *
 *   - an `anchors` bit beyond the three (the message names the value);
 *   - HUFGPU_ANCHOR_BOL or HUFGPU_ANCHOR_EOL without delim_set, for the positions call (the records call always needs one);
 *   - HUFGPU_ANCHOR_WORD without word_set;
 *   - with HUFGPU_ANCHOR_EOL or HUFGPU_ANCHOR_WORD: sum(alt_lens) + n_alts > HUFGPU_FIND_PATTERN_MAX - each alternative
 *     takes one more bit of the matcher's state (the message names the total).  HUFGPU_ANCHOR_BOL alone costs nothing.
 *
 * The identity: anchors = 0 enqueues exactly what hufgpu_find_any() / hufgpu_find_records_context() enqueue, and the sets
 * are not looked at; the nine older calls launch what they always did.  With EOL or WORD the cost is that of a longest
 * alternative one position longer; with BOL or WORD one kernel over the masks is added.  The records call with WORD needs a
 * third mask next to the matches' and the delimiters': hufgpu_find_bytes()' kernel walks the stream a SECOND time for it,
 * which grows two workspaces more; every other form stays at one walk.  Measured in DESIGN.md 5.21.
 *
 * OUT OF SCOPE: anchors per alternative ('^foo|bar$': make two calls, or one without anchors and look), patterns of
 * variable length (hufgpu_find_any_quant() has them, without anchors), and \b INSIDE a pattern.
 */
#define HUFGPU_ANCHOR_BOL   1u   /* '^' : the match starts where a record starts */
#define HUFGPU_ANCHOR_EOL   2u   /* '$' : the match ends where a record ends     */
#define HUFGPU_ANCHOR_WORD  4u   /* -w  : no word byte on either side            */
/* -x is BOL | EOL */
int hufgpu_find_any_anchored(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                             const uint64_t *d_block_offsets, uint64_t nblocks,
                             const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                             const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                             const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors,
                             uint64_t *d_pos, uint64_t pos_cap,
                             uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                             uint32_t flags, void *stream);
int hufgpu_find_records_anchored(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                                 const uint64_t *d_block_offsets, uint64_t nblocks,
                                 const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                                 const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                                 const uint8_t word_set[32], uint32_t anchors,
                                 uint32_t select, uint32_t before, uint32_t after,
                                 uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                                 uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                                 uint32_t flags, void *stream);

/*
 * FIND, ALL OF SEVERAL TERMS: grep A | grep B and grep 'A.*B'.  The records that hold EVERY one of up to
 * HUFGPU_FIND_TERMS_MAX terms - "ERROR" and "timeout" in one line -, or that hold them one behind the other, in ONE walk of
 * the stream: no call a term, no intersection of start lists on the host, and one not-served rule for the whole answer.
 * hufgpu_find_records_terms() is hufgpu_find_records_context() - the contract holds word for word: d_sub_index (the caller
 * vouches for NOTHING), every output, cap and total, `select`, d_rec_no, before / after, d_rec_sel, the known-extent rule,
 * one-symbol blocks served, flags, batch geometry, nblocks = 0, enqueue-only without a host write or a wait, every argument
 * error (worded "find_records_terms: ...") in the older call's order - but for which records are SELECTED.  There is no CPU
 * path.
 *
 *   a term        : what hufgpu_find_records_any() calls the whole pattern: one or more alternatives, each a pattern of
 *                   classes.  The terms' alternatives stand one behind the other in `classes` / `alt_lens` and share the 64
 *                   bits of the matcher's state: the lengths of ALL alternatives of ALL terms sum to at most
 *                   HUFGPU_FIND_PATTERN_MAX.  No class may hold a delimiter, so every occurrence lies inside one record.
 *   term_alts     : a HOST array of n_terms counts, read before the call returns.  Term 0 is the first term_alts[0]
 *                   alternatives, term 1 the next term_alts[1], and so on; the counts sum to n_alts.
 *   n_terms       : 1 to HUFGPU_FIND_TERMS_MAX.  The maximum rests on the walk kernel's registers - a mask word a term next
 *                   to the matcher's state - and on the workspace: a match mask and a record mask of raw_size / 8 bytes each
 *                   for every term.
 *   an occurrence : a pair (p, j) as hufgpu_find_any() defines a match of alternative j at p.
 *   terms_mode    : how a record [s, e) of known extent SATISFIES the call.
 *                     HUFGPU_TERMS_ALL      for every term t the record holds an occurrence of one of t's alternatives.
 *                                           Occurrences of different terms may overlap or be the same bytes: the terms
 *                                           ("ab", "abc") are satisfied by one "abc", as grep ab | grep abc is.
 *                     HUFGPU_TERMS_ORDERED  the record holds occurrences (p_1, j_1) ... (p_T, j_T), j_t an alternative of
 *                                           term t, with p_t + len_{j_t} <= p_{t+1}: T1.*T2.* ... .*TT with '.' any byte that
 *                                           is no delimiter.  "abc" does not satisfy ("ab", "bc"), "abbc" does; "aaa" does
 *                                           not satisfy ("aa", "aa"), "aaaa" does.  In this mode all alternatives of ONE term
 *                                           must have one length (terms may differ): then the leftmost occurrence of a term is
 *                                           also the one that ends first, and taking each term's first occurrence at or
 *                                           behind the end of the one before is exact.  With unequal lengths a later, shorter
 *                                           occurrence may end earlier - the terms ("abcd" or "bc", "d") in "abcd" -, and
 *                                           the walk would have to try every occurrence of every term.
 *   what is reported: S is the satisfying records; with HUFGPU_SELECT_INVERT the non-empty records of known extent that do
 *                   NOT satisfy - a record of known extent lies in exactly one of the two answers.  From S on everything is
 *                   hufgpu_find_records_context()'s: d_rec_no, before / after, d_rec_sel, rec_cap, max_len, d_totals[0..3],
 *                   d_block_counts, d_block_errs.
 *
 * Found on the host, before anything is enqueued and before the context is looked at, behind the `select` check and in front
 * of the older call's checks, and HUF_ERROR_INVALID_ARGUMENT are besides the older call's errors:
 *
 *   - a terms_mode above HUFGPU_TERMS_ORDERED (the message names the value);
 *   - a NULL term_alts;
 *   - an n_terms of 0 or above HUFGPU_FIND_TERMS_MAX (the message names it);
 *   - a term of 0 alternatives (the message names the term);
 *   - counts that do not sum to n_alts (the message names both);
 *   - HUFGPU_TERMS_ORDERED and a term whose alternatives differ in length (the message names the term and two lengths).
 *
 * The identity: n_terms = 1, in either mode, enqueues exactly what hufgpu_find_records_context() enqueues for the same
 * arguments, and the eleven older calls launch what they always did.  With more terms the walk keeps a mask word and a count
 * a term, the records' marking kernel runs once a term, one kernel ANDs the terms' record masks and - ordered - one more
 * walks the terms' match masks a candidate record; then the context call's kernels run as they are.  Measured in DESIGN.md 5.22.
 *
 * OUT OF SCOPE: anchors together with terms (hufgpu_find_records_anchored() has one term); unequal lengths inside a term of
 * an ordered call; a positions call - a conjunction has no natural "start" -; and which occurrences satisfied a record.
 */
#define HUFGPU_FIND_TERMS_MAX 4
#define HUFGPU_TERMS_ALL      0u
#define HUFGPU_TERMS_ORDERED  1u
int hufgpu_find_records_terms(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                              const uint64_t *d_block_offsets, uint64_t nblocks,
                              const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                              const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                              const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode,
                              uint32_t select, uint32_t before, uint32_t after,
                              uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                              uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                              uint32_t flags, void *stream);

/*
 * FIND, OPTIONAL AND REPEATED POSITIONS: grep -E 'colou?r', 'https?://', 'took [0-9]{1,5}ms',
 * '[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}'.  hufgpu_find_any_quant() is hufgpu_find_any() and
 * hufgpu_find_records_quant() is hufgpu_find_records_context() - their contracts hold word for word: d_sub_index (the caller
 * vouches for NOTHING), every output, cap and total, `select`, d_rec_no, before / after, d_rec_sel, the known-extent rule,
 * one-symbol blocks served, flags, batch geometry, nblocks = 0, enqueue-only without a host write or a wait, every argument
 * error (worded "find_any_quant: ..." / "find_records_quant: ...") in the older call's order - but for what a pattern is.
 * There is no CPU path.
 *
 *   optional      : a HOST array of one byte a position, in the order of `classes` (alt_lens sums to its length), read
 *                   before the call returns: 0 - the position is required -, or 1 - it may be left out.  NULL: all 0.
 *   a form        : an alternative with some - none, all - of its optional positions dropped.  An alternative stands for
 *                   ALL its forms: "colo" "u"? "r" for "color" and "colour".  x{m,n} is m required positions and n - m
 *                   optional ones of one class.
 *   a match       : a start p at which at least one form of at least one alternative lies as hufgpu_find_any() defines
 *                   that for an alternative of the form's classes: p + len <= raw_size, data[p + k] in the form's class k,
 *                   and every block that [p, p + len) touches is served.  Each form has its own span, hufgpu_find_any()'s
 *                   "own seam rule" stated for forms: a longer form that reaches into a block which is not served does
 *                   not take a shorter form's start away.  As a shorter span touches no more blocks, the SHORTEST form that
 *                   lies at p decides.  A start is reported once, ascending, however many forms lie there.
 *   alt_lens      : still sums to at most HUFGPU_FIND_PATTERN_MAX: a position takes one bit of the matcher's state
 *                   whether it is optional or not.  So no match is longer than 64 bytes.
 *   records       : no class may hold a delimiter, so every form lies inside one record; a record is selected when it
 *                   holds a match, and from there on everything is hufgpu_find_records_context()'s.
 *
 * Found on the host, before anything is enqueued and before the context is looked at, behind the older call's checks of
 * `select`, n_alts, the lengths and the classes and in front of its other checks, and HUF_ERROR_INVALID_ARGUMENT:
 *
 *   - an `optional` byte above 1 (the message names the alternative, the position and the value);
 *   - an alternative whose positions are all optional: it would match everywhere (the message names the alternative).
 *
 * The identity: with optional == NULL or all zeros the calls enqueue exactly what hufgpu_find_any() /
 * hufgpu_find_records_context() enqueue for the same arguments, and the twelve older calls launch what they always did.
 * With an optional position the walk and the seam kernel are two of their own - the same Shift-And automaton with one 64-bit
 * subtraction and four logic operations a byte more (Navarro and Raffinot's extended patterns) - and everything behind them
 * runs as it is; the workspace is that of an any-of call whose longest alternative has as many positions.  DESIGN.md 5.23.
 *
 * OUT OF SCOPE: anchors together with optional positions; optional positions inside hufgpu_find_records_terms();
 * unbounded repeats ('*', '+', '{m,}': they need state carried from tile to tile) and groups ('(ab)?'); and which form
 * matched, so where a match ends (hufgpu_find_any_spans() reports the longest form's end).
 */
int hufgpu_find_any_quant(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_block_offsets, uint64_t nblocks,
                          const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                          const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                          uint64_t *d_pos, uint64_t pos_cap,
                          uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                          uint32_t flags, void *stream);
int hufgpu_find_records_quant(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                              const uint64_t *d_block_offsets, uint64_t nblocks,
                              const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                              const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                              const uint8_t *optional,
                              uint32_t select, uint32_t before, uint32_t after,
                              uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                              uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                              uint32_t flags, void *stream);

/*
 * FIND, ONE grep -E LINE: anchors, terms and optional positions TOGETHER.  '^[0-9]{1,3}\.[0-9]{1,3}', grep -w 'colou?r',
 * 'refused [0-9]{1,5} times$', '^2026-10-19.*ERROR', 'ERROR.*took [0-9]{1,5}ms'.  hufgpu_find_any_expr() is
 * hufgpu_find_any_anchored() with `optional` behind n_alts; hufgpu_find_records_expr() is hufgpu_find_records_context()
 * with `optional`, the three term arguments of hufgpu_find_records_terms() and the two anchor arguments of
 * hufgpu_find_records_anchored().  Their contracts hold word for word: d_sub_index (the caller vouches for NOTHING), every
 * output, cap and total, `select`, d_rec_no, before / after, d_rec_sel, the known-extent rule, one-symbol blocks served,
 * flags, batch geometry, nblocks = 0, enqueue-only without a host write or a wait, every argument error (worded
 * "find_any_expr: ..." / "find_records_expr: ...") - but for what a pattern is and which occurrences count.  There is no CPU
 * path.
 *
 *   an occurrence : a start p, an alternative j and a FORM of j (hufgpu_find_any_quant(): some of its optional positions
 *                   dropped) of length len that lies at p.  Its left neighbour is L = data[p - 1], ABSENT when p = 0; its
 *                   right neighbour is R = data[p + len], absent when p + len = raw_size: R depends on the form.  It
 *                   QUALIFIES by hufgpu_find_any_anchored()'s rule, form by form:
 *                     HUFGPU_ANCHOR_BOL   L is absent or L is in D
 *                     HUFGPU_ANCHOR_EOL   R is absent or R is in D
 *                     HUFGPU_ANCHOR_WORD  (L is absent or L is not in W) and (R is absent or R is not in W)
 *   positions call: p is reported once, ascending, when some form of some alternative lies there, qualifies, and has its
 *                   tested span in served blocks only: [p, p + len), widened by one byte on each side where a neighbour
 *                   exists and an anchor tests it.  Each form has its own span; as a shorter span touches no more blocks,
 *                   the SHORTEST QUALIFYING form decides the right side ('ab?$' on "ab\n": "a" lies at p and does not
 *                   qualify, "ab" does).  A start is left out on doubt, never reported wrongly.
 *   records call  : n_terms = 1: a record is selected when it holds a qualifying occurrence.
 *                   HUFGPU_TERMS_ALL, more terms: every term may hold optional positions; anchors must be 0.
 *                   HUFGPU_TERMS_ORDERED, more terms: p_t + len_t <= p_{t+1} as in hufgpu_find_records_terms(), and the
 *                   anchors bind the OUTER edges - grep '^A.*B$', grep -w 'A.*B' -: BOL and the left half of WORD test L of
 *                   term 0's occurrence, EOL and the right half of WORD test R of the last term's.  Optional positions -
 *                   and alternatives of several lengths - are allowed in the LAST term only: the walk over a record takes
 *                   each term's first occurrence behind the end of the one before, which needs the end of every term but
 *                   the last.  That is exact: term 0's starts are filtered to those whose L qualifies, the last term's to
 *                   those with a form whose R qualifies, and as the lengths in front of the last term are fixed, taking the
 *                   first of each finds a witness if and only if there is one.
 *                   From the selected records on everything is hufgpu_find_records_context()'s.
 *   the budget    : with EOL or WORD every alternative whose right neighbour is tested takes one more bit of the matcher's
 *                   state: all alternatives of the positions call and of a one-term call, the last term's otherwise.  The
 *                   lengths plus one for each of those sum to at most HUFGPU_FIND_PATTERN_MAX.
 *   one-symbol blocks: served; an alternative lies inside one only if the one value is in the classes of one of its forms
 *                   AND may stand behind it.
 *
 * Found on the host, before anything is enqueued and before the context is looked at, HUF_ERROR_INVALID_ARGUMENT, in this
 * order (the older calls', each group where its call has it):
 *
 *   1. `select` with a bit other than HUFGPU_SELECT_INVERT (records call);
 *   2. the anchored calls': an unknown `anchors` bit; BOL or EOL without delim_set (positions call); WORD without word_set;
 *   3. the terms call's: terms_mode, a NULL term_alts, n_terms, a term without alternatives, counts that do not sum to n_alts;
 *      then HUFGPU_TERMS_ORDERED with unequal lengths in a term OTHER than the last;
 *   4. HUFGPU_TERMS_ALL with n_terms > 1 and anchors != 0;
 *   5. the any-of calls': n_alts, a length of 0, the sum of the lengths; then the budget above; then the classes;
 *   6. the quant calls': an `optional` byte above 1, an alternative whose positions are all optional;
 *   7. HUFGPU_TERMS_ORDERED with an optional position in a term other than the last (the message names the term, the
 *      alternative and the position);
 *   8. the older calls' remaining checks (required pointers, caps, geometry, the context).
 *
 * The identities.  With optional NULL or all zeros and one term the calls enqueue exactly what hufgpu_find_any_anchored() /
 * hufgpu_find_records_anchored() enqueue; with anchors = 0 and one term what hufgpu_find_any_quant() /
 * hufgpu_find_records_quant() enqueue; with anchors = 0 and no optional position what hufgpu_find_records_terms() enqueues
 * (which, unlike that call, also serves an ordered last term of several lengths).  The fourteen older calls launch what
 * they always did.  Where the dimensions cross, the walk is the quant calls' (several terms: the terms' walk with the
 * closure), the seam kernel is the quant calls' window with the end of the data as a boundary, and the kernel for the byte
 * in front runs over the one mask, or term 0's.  DESIGN.md 5.24.
 *
 * OUT OF SCOPE: anchors with HUFGPU_TERMS_ALL of several terms (which term would they bind?); optional positions in a term
 * in front of another in an ordered call (its earliest end is not to be had from a mask of starts); anchors per alternative;
 * \b INSIDE a pattern; unbounded repeats; groups; and which form matched (hufgpu_find_any_spans() reports the longest
 * form's length for the positions call).
 */
int hufgpu_find_any_expr(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                         const uint64_t *d_block_offsets, uint64_t nblocks,
                         const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                         const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                         const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors,
                         uint64_t *d_pos, uint64_t pos_cap,
                         uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                         uint32_t flags, void *stream);
int hufgpu_find_records_expr(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                             const uint64_t *d_block_offsets, uint64_t nblocks,
                             const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                             const uint8_t delim_set[32], const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts,
                             const uint8_t *optional,
                             const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode,
                             const uint8_t word_set[32], uint32_t anchors,
                             uint32_t select, uint32_t before, uint32_t after,
                             uint64_t *d_rec_pos, uint32_t *d_rec_len, uint64_t *d_rec_no, uint8_t *d_rec_sel, uint64_t rec_cap, uint32_t max_len,
                             uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                             uint32_t flags, void *stream);

/*
 * FIND, MATCH SPANS: where each occurrence ENDS.  grep -o and redaction of exactly what matched need, next to every start,
 * the length of what lies there: an IP address, 'took [0-9]{1,5}ms', 'req-[0-9a-f]{1,8}', 'colou?r'.
 * hufgpu_find_any_spans() is hufgpu_find_any_expr() with d_len and d_open directly behind d_pos, and that call's contract
 * holds word for word: d_sub_index (the caller vouches for NOTHING), the same starts in the same order, d_totals[0..2],
 * d_block_counts and d_block_errs, one-symbol blocks served, flags, batch geometry, nblocks = 0, enqueue-only without a host
 * write or a wait, capturable - with every buffer of the caller's made outside the capture - once a call of the same sizes has
 * made the workspaces.  A span call and an expr call with the
 * same arguments write bit-identical d_pos, d_totals[0..2], d_block_counts and d_block_errs.  There is no CPU path.
 *
 *   d_len         : for every rank r < d_totals[1] - nothing else is written - the length in bytes of the LONGEST form of any
 *                   alternative that lies at d_pos[r], QUALIFIES under `anchors` form by form as hufgpu_find_any_expr()
 *                   defines it, and has its tested span in served blocks and inside raw_size: [p, p + len), widened by the
 *                   right neighbour where HUFGPU_ANCHOR_EOL or HUFGPU_ANCHOR_WORD tests it.  A boundary byte is not part of
 *                   the length.  1 <= d_len[r] <= HUFGPU_FIND_PATTERN_MAX always: a start is reported only if a qualifying
 *                   form lies there in served blocks.  A plain number: hufgpu_gather() and hufgpu_scatter() take the array
 *                   as it is, with max_len = HUFGPU_FIND_PATTERN_MAX.  Required when pos_cap > 0.
 *   d_open        : optional (NULL is fine), a byte a rank: 1 when a LONGER form could not be ruled out because a byte it
 *                   needs - one of its own or its tested right neighbour - lies in a block that is not served, else 0.
 *   d_totals[3]   : how many of the written spans are open, whether or not d_open is given; 0 when d_totals[2] is 0.
 *
 * Found on the host as hufgpu_find_any_expr()'s errors are, worded "find_any_spans: ...", in that call's order; new, with
 * the required pointers (its group 8): pos_cap > 0 with a NULL d_len, HUF_ERROR_INVALID_ARGUMENT.
 *
 * What runs: the expr call's chain as it is, then ONE kernel over the walk's grid that decodes the tiles holding a start
 * below pos_cap a second time - into LDS, no decoded byte reaches memory - and runs a forward automaton from every start,
 * reading on into the edge bytes that the walk kept of the following tiles.  Without an optional position and with one
 * length for all alternatives nothing is decoded twice: the kernel that writes d_pos writes the constant.  The seventeen
 * older calls launch what they always did.  The worst case - every byte a start of 64 steps - and the measurements are in
 * DESIGN.md 5.26.
 *
 * OUT OF SCOPE: the non-overlapping leftmost-longest selection that grep -o prints (EVERY start is reported, overlapping
 * ones included, as the family always has: hufgpu_select_spans() selects from them); spans for the records calls; the ends of a quantified middle term of an ordered
 * call; unbounded repeats; groups.
 */
int hufgpu_find_any_spans(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_block_offsets, uint64_t nblocks,
                          const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                          const uint8_t *classes, const uint32_t *alt_lens, uint32_t n_alts, const uint8_t *optional,
                          const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors,
                          uint64_t *d_pos, uint32_t *d_len, uint8_t *d_open, uint64_t pos_cap,
                          uint64_t *d_block_counts, uint64_t *d_totals, int32_t *d_block_errs,
                          uint32_t flags, void *stream);

/*
 * SELECT SPANS: grep -o's non-overlapping leftmost-longest matches, chosen on the device from the spans that
 * hufgpu_find_any_spans() reports.  That call reports EVERY start: '[0-9]{1,3}' on "1234" gives 0:3, 1:3, 2:2, 3:1, and
 * grep -o prints 0:3 and 3:1.  The selection is a chain - the next match is the first start at or behind the end of the match
 * just taken - whose lengths are known only on the device; hufgpu_select_spans() walks it there, enqueue-only, so that
 * find_any_spans -> select_spans -> gather | scatter runs with no operation of the caller's in between and no host wait.
 *
 *   d_pos, d_len  : spans by rank, exactly as hufgpu_find_any_spans() leaves them: positions strictly ascending,
 *                   1 <= len <= HUFGPU_FIND_PATTERN_MAX.  Required.
 *   d_n, n_cap    : the number of spans is n = min(*d_n, n_cap).  d_n is a DEVICE word - &d_totals[1] of the span call can
 *                   be passed as it is -; NULL means n = n_cap.  Nothing at or behind rank n is read for its value.  n_cap
 *                   sizes the grids - rows beyond n do nothing - and is at most HUFGPU_SELECT_MAX.
 *
 * The selection: rank 0 is selected; after a selected rank s the next selected rank is the least r > s with
 * pos[r] >= pos[s] + len[s].  When the span call served every block (d_totals[2] == 0) and was not cut
 * (d_totals[0] == d_totals[1]), this is the set that grep -o -E prints.  Otherwise it is the greedy selection over what was
 * reported.
 *
 *   d_sel_pos, d_sel_len : the selected spans, compacted and in ascending order: the first min(selected, sel_cap) are written
 *                   and nothing behind them (but the pad rows).  Required when sel_cap > 0.
 *   d_sel_rank    : optional (NULL is fine): the input rank of every written row, so that the caller can read d_open[rank].
 *                   A pad row's rank is not written.
 *   pad_pos, HUFGPU_SELECT_PAD : with the flag the rows from the written count to sel_cap get (pad_pos, 0).  A record of
 *                   length 0 at raw_size reads and writes nothing in hufgpu_gather() / hufgpu_scatter(): with
 *                   pad_pos = raw_size those calls take the arrays as they are, with nrecords = sel_cap.
 *   d_sel_totals  : four words.  [0] the number selected, [1] the number written, [2] the status, [3] the lowest offending
 *                   rank (0 with status 0).  Required.
 *
 * The status is HUF_ERROR_INVALID_ARGUMENT when, among the n spans, a rank r > 0 has pos[r] <= pos[r - 1] or a rank has a
 * length outside 1 ... HUFGPU_FIND_PATTERN_MAX; r is the offending rank.  This is found on the device, as hufgpu_scatter()
 * finds its errors: then [0] = [1] = 0 and no span row is written; pad rows are still written, all sel_cap of them.
 *
 * Found on the host, HUF_ERROR_INVALID_ARGUMENT, worded "select_spans: ...", in this order: a NULL d_pos, d_len or
 * d_sel_totals; sel_cap > 0 with a NULL d_sel_pos or d_sel_len; n_cap above HUFGPU_SELECT_MAX; a flag bit other than
 * HUFGPU_SELECT_PAD; an output array (d_sel_pos, d_sel_len, d_sel_rank, d_sel_totals) that starts at the address of an input
 * array (d_pos, d_len, d_n); a NULL ctx (there is no CPU path).  n_cap == 0 is not an error: the totals are written as
 * zeros, and the pads are written.
 *
 * Enqueue-only on `stream`: no host read of device memory, no wait.  Capturable - with every buffer of the caller's made
 * outside the capture - once a call of the same n_cap and sel_cap has made the workspaces.  What runs (kernels/select.hpp,
 * DESIGN.md 5.27): no length is above 64 and positions rise by at least 1 a rank, so the successor of rank i lies in
 * (i, i + 64]; a tile of ranks is reduced to a map of 64 entry offsets to 64 exit offsets, the maps are composed in groups
 * level by level, every tile then walks from its true entry, and a scan of the tiles' counts places the compacted rows.  The
 * work is O(n_cap); the number of launches does not depend on n_cap up to 2^28.  hufgpu_select_geometry() reports the two
 * constants: out[0] ranks a tile, out[1] tiles a composition group.
 *
 * OUT OF SCOPE: selection for the records calls (records never overlap); lengths above HUFGPU_FIND_PATTERN_MAX;
 * leftmost-FIRST (Perl) semantics; replacement with text of another length; a fused search + select kernel.
 */
#define HUFGPU_SELECT_PAD 1u
#define HUFGPU_SELECT_MAX (1ull << 30)
int hufgpu_select_spans(hufgpu_ctx_t *ctx,
                        const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_n, uint64_t n_cap,
                        uint64_t *d_sel_pos, uint32_t *d_sel_len, uint64_t *d_sel_rank, uint64_t sel_cap,
                        uint64_t pad_pos, uint64_t *d_sel_totals, uint32_t flags, void *stream);
void hufgpu_select_geometry(uint32_t out[2]);   /* ranks a tile, tiles a composition group */

/*
 * The sub-index of a stream that came without one: read from a file, written by the reference on a CPU, received from
 * another rank, or encoded here by a caller that did not keep the 7 % of side data.  hufgpu_encode_sub() writes the
 * sub-index as a by-product of packing; these three rebuild exactly that - the same entries, entry for entry
 * (kernels/sub_build.hpp) - from the stream, its block index and the decoded bytes, so that hufgpu_decode_sub() and
 * hufgpu_decode_ranges(..., d_sub_index, ...) decode the stream at their fast rate from then on.
 *
 * (raw_size, blocksize) are those of the encode that wrote the stream, exactly as hufgpu_decode_sub() takes them: they
 * fix the block count and the layout.  d_sub_index: hufgpu_sub_index_bytes(raw_size, blocksize) bytes of device memory,
 * 8-byte aligned; what the encoder never writes there (one-symbol blocks, padding, entries behind a short last block)
 * these calls never write either.  flags: HUFGPU_RELAXED_TREE as for hufgpu_decode().
 *
 * A block is UNBUILT when its header or tree does not parse under `flags`, its header's length is not the layout's, a
 * byte of its data has no code in its tree, or its code lengths do not add up to the payload the index gives it (and,
 * for the two calls that decode, when it did not decode).  *unbuilt counts such blocks; their rows hold whatever they
 * held, or stale entries.  That costs time, never correctness: the decoders verify every entry they use and decode an
 * unverifiable block the slow way.  Trees of any shape are taken - every byte value on at most one leaf, codes of 1 to
 * 255 bits; a block with codes over 32 bits gets its entries like any other (hufgpu_decode_sub sends it to the exact
 * decoder by design).
 *
 * Argument errors - no context, a NULL stream or index, a missing or misaligned sub-index - return
 * HUF_ERROR_INVALID_ARGUMENT before anything is enqueued; raw_size = 0 is success.
 *
 * hufgpu_sub_index_from_raw: the caller holds the decoded data (raw_size bytes at d_raw, any alignment; nothing behind
 *   them is read).  One launch sequence; with unbuilt = NULL it only enqueues.
 * hufgpu_decode_build_sub: hufgpu_decode() - its results, errors and delivered bytes, unchanged, raw_len = NULL enqueues
 *   and hufgpu_decode_result() reports as usual - and the sub-index from the output it has just written.  After a
 *   decode error the rows of the blocks that did not decode are unbuilt and counted.
 * hufgpu_build_sub_index: no output buffer is wanted - the blocks are decoded into a scratch area of the context (128 MiB
 *   of whole blocks at a time, at least one block; HUF_ERROR_MEMORY_ALLOCATION when it cannot be had) and indexed from
 *   there.  Synchronous.  A pending hufgpu_decode() of the context is forgotten.
 */
int hufgpu_sub_index_from_raw(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                              const uint64_t *d_block_offsets, const void *d_raw, uint64_t raw_size,
                              uint64_t blocksize, void *d_sub_index, uint32_t flags, uint64_t *unbuilt, void *stream);
int hufgpu_decode_build_sub(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                            const uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                            void *d_out, uint64_t out_cap, void *d_sub_index, uint32_t flags,
                            uint64_t *raw_len, uint64_t *unbuilt, void *stream);
int hufgpu_build_sub_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                           const uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                           void *d_sub_index, uint32_t flags, uint64_t *unbuilt, void *stream);

/*
 * OVERWRITE: byte ranges of the original data replaced in one indexed stream, out of place, many ranges in one launch
 * sequence - the write side of hufgpu_decode_ranges().  Only the blocks a range touches are encoded again; every other
 * record moves to its new place byte for byte.  Changing 4 KiB of a gigabyte costs a copy of the stream plus a fixed
 * 0.2 ms (measured: 0.57 ms, 1.6 device copies of the stream, a third of decode + patch + encode).
 *
 * Raw positions are those of hufgpu_decode_ranges(): block b covers [P[b], P[b+1]), P = the exclusive sums of the
 * block_len header fields; no blocksize is assumed for the stream, so the stream of a batch and a reference-written
 * stream with an index from hufgpu_block_index() work.  Let D be the data the stream decodes to and D' be D with
 * [range_lo[i], range_hi[i]) replaced by the range_hi[i] - range_lo[i] bytes at d_src + src_offsets[i] (src_offsets = NULL:
 * the ranges' bytes lie back to back at d_src, in range order).  An overwrite changes no length: every block keeps its
 * block_len.  The new stream at d_out is the records of all blocks back to back: an untouched block's record is the old
 * one, a touched block's record is what hufgpu_encode() writes for the block's bytes of D' alone.  For a stream written
 * by hufgpu_encode(D, blocksize) the result is hufgpu_encode(D', blocksize) byte for byte, d_out_block_offsets
 * (nblocks + 1 entries, optional) its block index.
 *
 *   ranges          : host arrays, lo <= hi, in any order; empty ranges are allowed and ignored.  Ranges that overlap
 *                     return HUF_ERROR_INVALID_ARGUMENT (ranges that touch do not overlap).  A range that reaches past the
 *                     end of the data returns HUF_ERROR_INVALID_ARGUMENT, one that reaches the first block whose header
 *                     does not parse returns that header's error; both are found on the device.
 *   out of place    : d_out (out_cap bytes, 4-byte aligned: the packer writes whole words of the destination),
 *                     d_out_block_offsets and d_out_sub_index must not overlap the stream, its index, its sub-index,
 *                     the new bytes or one another: HUF_ERROR_INVALID_ARGUMENT.  The old stream is
 *                     never written.  A new stream longer than out_cap returns HUF_ERROR_MEMORY_ALLOCATION; old length +
 *                     touched blocks x hufgpu_encode_bound(longest block, 0) always suffices.
 *   routing         : a block wholly inside one range is encoded straight from the new bytes; its old record is not
 *                     looked at beyond its header, so damage in its old payload does not matter.  A block that a range
 *                     edge cuts or that several ranges touch is decoded once into the context's scratch area (the one
 *                     hufgpu_decode_ranges() uses; HUF_ERROR_MEMORY_ALLOCATION when it cannot grow) by the indexed
 *                     decoders, overwritten there and encoded from there; when it does not decode the call returns what
 *                     hufgpu_decode() says of it, the first such block in stream order.  Untouched blocks are not decoded:
 *                     payload damage in them is carried over unseen, as in hufgpu_decode_ranges().  A block behind a
 *                     header that does not parse is untouched by definition; an index entry that names no bytes of the
 *                     stream (offsets that decrease or pass stream_len) gets no bytes in the new stream.
 *   d_sub_index     : optional, the OLD stream's, with (raw_size, blocksize) as in hufgpu_decode_ranges(): speeds up the
 *                     decode of the cut blocks, verified as ever - any content gives the same result.
 *   d_out_sub_index : optional, hufgpu_sub_index_bytes(raw_size, blocksize) bytes, 8-byte aligned, needs (raw_size,
 *                     blocksize) that give nblocks blocks and blocksize below HUFGPU_BATCH_CHUNKED_FROM (for a batch's
 *                     stream: nblocks x row_blocksize, row_blocksize); a touched block longer than blocksize returns
 *                     HUF_ERROR_INVALID_ARGUMENT.  The rows of the touched blocks receive every entry hufgpu_encode_sub()
 *                     writes for them.  With d_sub_index as well, the rows of the untouched blocks are copied from it
 *                     (the entries the encoder writes, nothing else), so the buffer then holds the whole sub-index of
 *                     the new stream; WITHOUT d_sub_index only the touched rows are written.
 *   *blocks_reencoded: the number of touched blocks (optional).
 * Blocks of HUFGPU_BATCH_CHUNKED_FROM bytes and more: when a touched block is that long, the touched blocks are encoded
 * one at a time through the chunked path (same output, one wait per block).
 * Synchronous: waits once for the plan and once for the result.  Argument errors (lo > hi, overlapping ranges, NULL host
 * arrays with nranges > 0, no context, a misaligned d_out, a misaligned or mis-sized sub-index, overlapping buffers) return
 * HUF_ERROR_INVALID_ARGUMENT before anything is enqueued.  nranges = 0 (or only empty ranges) is a plain copy of the
 * stream, its index and - when both are given - its sub-index, and succeeds.  On any error *out_len = 0 and the content
 * of d_out and the output indexes is unspecified; nothing outside them is ever written.  A pending hufgpu_decode() of
 * the context is forgotten.  There is no CPU path.
 */
int hufgpu_update_ranges(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                         const uint64_t *d_block_offsets, uint64_t nblocks,
                         uint64_t nranges, const uint64_t *range_lo, const uint64_t *range_hi,
                         const uint64_t *src_offsets, const void *d_src,
                         const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                         void *d_out, uint64_t out_cap, uint64_t *d_out_block_offsets, void *d_out_sub_index,
                         uint32_t flags, uint64_t *out_len, uint64_t *blocks_reencoded, void *stream);

/*
 * SCATTER: records overwritten at positions that are on the device - the write side of hufgpu_gather(), as
 * hufgpu_update_ranges() is the write side of hufgpu_decode_ranges().  The starts and (start, length) records that the
 * hufgpu_find_* calls leave in device memory go in as they are: find -> scatter blanks what grep found with no host wait in
 * between, and both can sit in one captured graph.  Nothing about the records is read on the host, no host memory is
 * written, and the call only enqueues on `stream` (NULL = the context's); it waits only when a workspace of the context
 * grows.  Two calls back to back on one stream are safe, calls on different streams of one context are not.  It works on
 * a non-default stream and inside a stream capture (a replay reads d_pos, d_len and d_src anew).  There is no CPU path.
 *
 *   record i      : bytes [d_pos[i], d_pos[i] + len_i) of the original data, exactly as hufgpu_gather() defines it: len_i =
 *                   d_len[i] or, with d_len = NULL, max_len for every record.  Positions are the layout's: fixed blocksize,
 *                   blocksize = 0 means one block.  A record that reaches past raw_size is cut there; one that starts at
 *                   or behind raw_size, or has len_i = 0, writes nothing.  An overwrite changes no length.
 *   new bytes     : without HUFGPU_SCATTER_FILL the first len_i bytes of slot d_src + i * src_stride (src_stride >= max_len,
 *                   any alignment) - the layout hufgpu_gather() writes, so gather -> the caller's kernel -> scatter needs
 *                   no repacking.  With the flag every covered byte becomes `fill` and d_src is not read.
 *   overlap       : records may repeat, overlap and come in any order (the overlapping starts of hufgpu_find_pattern() are
 *                   the normal input).  With FILL the result is defined.  Without, a byte that several records cover
 *                   receives the byte that ONE of those records carries for it, which one is unspecified; every other byte
 *                   is exact.
 *   result        : hufgpu_update_ranges()' contract word for word.  With D' = D with the records applied, d_out receives
 *                   the records of all blocks back to back: an untouched block's record is the old one, moved byte for
 *                   byte, a touched block's record is what hufgpu_encode() writes for the block's bytes of D' alone.  For a
 *                   stream of hufgpu_encode(D, blocksize) the output is hufgpu_encode(D', blocksize) byte for byte.
 *                   d_out_block_offsets (nblocks + 1 entries) is REQUIRED here and receives the new index.
 *                   d_out_sub_index is optional and follows hufgpu_update_ranges()' rules: the touched rows receive every
 *                   entry hufgpu_encode_sub() writes; with d_sub_index given as well the untouched rows are copied from it.
 *                   d_sub_index is optional, verified as ever - any content gives the same result - and only speeds up
 *                   the decode of the touched blocks.
 *   routing       : EVERY touched block is staged: decoded whole into the context's scratch area (the one
 *                   hufgpu_decode_ranges() uses) by the indexed decoders, overlaid there, encoded from there.  There is no
 *                   "direct" kind - whether a block lies wholly inside one record would need the records sorted.  So a
 *                   touched block MUST DECODE, even when the records cover all of it (hufgpu_update_ranges() does not ask
 *                   that of a block wholly inside one range).  Untouched blocks are not decoded: damage in them is carried
 *                   over unseen.
 *   touched_cap   : the largest number of distinct blocks the records may touch, 1 .. nblocks.  It sizes the scratch area
 *                   (touched_cap x blocksize rounded up to 16; HUF_ERROR_MEMORY_ALLOCATION from the call itself when it
 *                   cannot grow), the row workspaces and every row grid.  hufgpu_scatter_touched_bound() returns
 *                   min(nblocks, nrecords * ((max_len + blocksize - 2) / blocksize + 1)), which always suffices (1 for
 *                   blocksize = 0).  If more blocks are touched the call reports failure in d_result; it never writes
 *                   outside its buffers.
 *   d_result      : four words of device memory, required, zeroed by the call's first kernel, written by its last launch:
 *                     [0] status: 0 or a huf_error_t value        [2] the number of touched blocks, even when above the cap
 *                     [1] the length of the new stream, 0 when    [3] the record or block that caused the status, ~0 when
 *                         the status is not 0                         none
 *                   The status is the first condition that holds, in this order:
 *                     1. HUF_ERROR_INVALID_ARGUMENT: some len_i > max_len; [3] is the lowest such i (such records write
 *                        nothing and touch nothing).
 *                     2. HUF_ERROR_MEMORY_ALLOCATION: touched > touched_cap.
 *                     3. a touched block cannot be served: its header does not parse under `flags`, its block_len is not
 *                        the layout's, or it does not decode.  The status is what hufgpu_decode() says of it, or
 *                        HUF_ERROR_READ_WRITE for a block_len that is not the layout's; [3] is the first such block in
 *                        stream order.
 *                     4. HUF_ERROR_MEMORY_ALLOCATION: the new stream is longer than out_cap.  Old length + touched_cap x
 *                        hufgpu_encode_bound(blocksize, 0) always suffices.
 *                   With a non-zero status the contents of d_out and the two output indexes are unspecified; nothing else
 *                   has been written.  The input stream is never written.
 *   flags         : HUFGPU_RELAXED_TREE as for hufgpu_decode(), HUFGPU_SCATTER_FILL.
 *
 * Argument errors return HUF_ERROR_INVALID_ARGUMENT, worded "scatter: ...", before anything is enqueued and before the
 * context is looked at, the first that holds in this order: a NULL d_stream / d_block_offsets / d_pos / d_out /
 * d_out_block_offsets / d_result; a NULL d_src without FILL; src_stride < max_len without FILL; (raw_size, blocksize) that
 * do not give nblocks; blocksize >= HUFGPU_BATCH_CHUNKED_FROM (the chunked encoder waits once per block, so this call does
 * not serve it); touched_cap = 0 or above nblocks; more than 2^32 - 1 (record, block) parts by hufgpu_gather()'s bound;
 * a d_out that is not 4-byte aligned, a sub-index that is not 8-byte aligned; a d_out_sub_index with a layout it cannot
 * hold (more than 2^31 - 1 rows of chunks); hufgpu_update_ranges()' out-of-place overlap checks with the d_src extent
 * nrecords * src_stride, and d_result against the three outputs; no context.  nrecords = 0 or max_len = 0 is
 * hufgpu_update_ranges()' "no ranges" case, enqueued: a plain copy of the stream, its index and - when both are given -
 * its sub-index, with d_result = {0, stream_len, 0, ~0} (or {HUF_ERROR_MEMORY_ALLOCATION, 0, 0, ~0} and nothing copied
 * when stream_len > out_cap).  A pending hufgpu_decode() of the context is forgotten.
 */
#define HUFGPU_SCATTER_FILL 0x100u   /* flags: every record's new bytes are `fill`, d_src is not read */
int hufgpu_scatter(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t stream_len,
                   const uint64_t *d_block_offsets, uint64_t nblocks,
                   const void *d_sub_index, uint64_t raw_size, uint64_t blocksize,
                   uint64_t nrecords, const uint64_t *d_pos, const uint32_t *d_len, uint32_t max_len,
                   const void *d_src, uint64_t src_stride, uint8_t fill,
                   uint64_t touched_cap,
                   void *d_out, uint64_t out_cap, uint64_t *d_out_block_offsets, void *d_out_sub_index,
                   uint64_t *d_result, uint32_t flags, void *stream);
uint64_t hufgpu_scatter_touched_bound(uint64_t nblocks, uint64_t blocksize, uint64_t nrecords, uint32_t max_len);

/*
 * APPEND and TRUNCATE: an indexed stream made longer or shorter IN PLACE.  Every record in front of the last block
 * stays where it is, so the cost follows the appended bytes, not the stream.
 *
 * hufgpu_append: let D be the raw_size bytes the stream decodes to; the stream was written by hufgpu_encode(D, blocksize)
 * (blocksize as passed there, not 0).  Let A be the src_len bytes at d_src, at any alignment.  After the call
 * d_stream[0, *out_len) is hufgpu_encode(D ++ A, blocksize) byte for byte, and d_block_offsets[0 .. nb_new] its block
 * index, nb_new = hufgpu_block_count(raw_size + src_len, blocksize) - the caller's index buffer has room for nb_new + 1
 * entries.
 *
 *   what is touched : with t = raw_size % blocksize and nb_keep = nb_old - (t > 0), the records of blocks [0, nb_keep)
 *                     and the index entries [0, nb_keep] are not written, and apart from the last block's header, which
 *                     is always read, not read either: payload damage in them is carried over unseen, as in
 *                     hufgpu_update_ranges().  With t > 0 the last block is decoded once into the context's scratch area
 *                     (the one hufgpu_decode_ranges() uses; HUF_ERROR_MEMORY_ALLOCATION when it cannot grow) by the
 *                     indexed decoders, the first min(src_len, blocksize - t) bytes of A are placed behind it and the
 *                     joined block is encoded from there; every further block is encoded straight from A.  The new
 *                     records land at old_index[nb_keep] onwards.  With t = 0 or raw_size = 0 nothing is decoded.
 *   canonical check : the last block's header must parse (else: what hufgpu_decode() reports for it) and show a
 *                     block_len of t (blocksize when t = 0), else HUF_ERROR_INVALID_ARGUMENT: a batch's stream, a wrong
 *                     raw_size, a stream that already has a short block in the middle.  A tail that does not decode
 *                     returns hufgpu_decode()'s error for it.
 *   all or nothing  : on any error - a new length over stream_cap (HUF_ERROR_MEMORY_ALLOCATION), a tail that does not
 *                     decode, a bad header, an argument error - d_stream[0, stream_len) and d_block_offsets[0 .. nb_old]
 *                     are unchanged byte for byte and *out_len = 0.  Nothing behind stream_cap or behind index entry
 *                     nb_new is ever written, and on success nothing in [*out_len, stream_cap) either.
 *                     stream_len + hufgpu_encode_bound(t + src_len, blocksize) always suffices as stream_cap.
 *   d_sub_index     : optional, the OLD stream's (hufgpu_sub_index_bytes(raw_size, blocksize) bytes): speeds up the decode
 *                     of the tail, verified as ever - any content gives the same result.
 *   d_out_sub_index : optional, hufgpu_sub_index_bytes(raw_size + src_len, blocksize) bytes, 8-byte aligned, blocksize
 *                     below HUFGPU_BATCH_CHUNKED_FROM.  The three arrays of a sub-index are each sized by the block count,
 *                     so a longer stream has another layout: the sub-index cannot grow in place and is written out of
 *                     place.  It receives the rows of the new blocks; with d_sub_index as well, the rows of blocks
 *                     [0, nb_keep) are copied from the old layout to the new one, so the buffer then holds the sub-index
 *                     of the new stream wherever hufgpu_encode_sub() writes one.  Whole rows are copied, since these
 *                     blocks' headers are not read: the padding of a row and the row of a one-symbol block, which the
 *                     encoder never writes and no decoder reads, carry whatever the old buffer held.  That copy moves 7 % of
 *                     the raw size and is the only part of the call that grows with the stream.  WITHOUT d_sub_index
 *                     only the new rows are written.
 * Synchronous: waits once, for (error, *out_len).  Argument errors - blocksize = 0, stream_len > stream_cap, a NULL
 * stream or index with raw_size > 0 or src_len > 0, a NULL d_src with src_len > 0, a d_stream that is not 4-byte aligned, a
 * misaligned sub-index, d_src, d_sub_index or d_out_sub_index overlapping d_stream[0, stream_cap), the index or one
 * another, no context - return HUF_ERROR_INVALID_ARGUMENT before anything is enqueued.  src_len = 0 is success, writes
 * nothing, needs no context and gives *out_len = stream_len.  Blocks of HUFGPU_BATCH_CHUNKED_FROM bytes and more take a slow route through
 * the chunked encoder (same output, same guarantee, several waits, scratch for the new records as well); a d_out_sub_index
 * returns HUF_ERROR_INVALID_ARGUMENT there.  A pending hufgpu_decode() of the context is forgotten.  There is no CPU path.
 */
int hufgpu_append(hufgpu_ctx_t *ctx, void *d_stream, uint64_t stream_len, uint64_t stream_cap,
                  uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                  const void *d_src, uint64_t src_len,
                  const void *d_sub_index, void *d_out_sub_index,
                  uint32_t flags, uint64_t *out_len, void *stream);

/*
 * hufgpu_truncate: the stream of hufgpu_append() cut to its first new_raw_size bytes: afterwards d_stream[0, *out_len) is
 * hufgpu_encode(D[0, new_raw_size), blocksize) and d_block_offsets[0 .. hufgpu_block_count(new_raw_size, blocksize)] its
 * index, in place, with the guarantees and the argument checks of hufgpu_append() (stream_cap = stream_len: a cut never
 * makes a stream longer).  new_raw_size > raw_size returns HUF_ERROR_INVALID_ARGUMENT; new_raw_size = raw_size changes
 * nothing.  A cut on a block border decodes nothing and writes nothing: *out_len is the device index entry at that border
 * (one wait).  A cut inside block k decodes block k into the scratch area and encodes its first new_raw_size - k * blocksize
 * bytes at old_index[k]; index entry k + 1 is written, the entries behind it are left as they are.  The canonical check
 * applies to the header of block k: its block_len must be blocksize, or raw_size % blocksize for the last block.
 * d_out_sub_index is laid out for (new_raw_size, blocksize): row k is written by the encoder, rows [0, k) are copied when
 * d_sub_index is given.
 */
int hufgpu_truncate(hufgpu_ctx_t *ctx, void *d_stream, uint64_t stream_len,
                    uint64_t *d_block_offsets, uint64_t raw_size, uint64_t blocksize,
                    uint64_t new_raw_size,
                    const void *d_sub_index, void *d_out_sub_index,
                    uint32_t flags, uint64_t *out_len, void *stream);

/*
 * One logical input over the GPUs of a node: RCCL scatter / gather of block buffers.
 * Blocks are independent (src/encoder.c:288-374 resets all state between blocks), so rank r of G owns a contiguous range
 * of ceil(nblocks / G) blocks (hufgpu_shard_range) and the codec needs no collective; the data starts and ends on ONE
 * rank, the root.  Every rank of the communicator makes the same call with the same n_total, blocksize, root and flags;
 * the pointers count on the root only (NULL elsewhere).  Each movement is one group of ncclSend / ncclRecv of exactly-sized
 * buffers to computed offsets (RCCL has no scatterv / gatherv) on the object's own stream, plus all-gathers of one or two
 * words a rank: who is ready, every shard's compressed size (rank order = stream order: shard r starts at the sum of the
 * sizes in front of it), every rank's decode result.  The gathered stream is the reference's, byte for byte - the one a
 * single hufgpu_encode() of the whole input writes.  RCCL is looked up with dlopen at the first call (HUF_GPU_RCCL_LIB,
 * else librccl.so.1): without it these entry points return HUF_ERROR_FATAL and hufgpu_shard_last_error(NULL) says why.
 * Every call has a deadline (HUF_GPU_SHARD_TIMEOUT_MS when the object is made, default 120 000 ms; hufgpu_shard_set_timeout;
 * 0 = none): a rank that never arrives, or a communicator that reports an asynchronous error, makes the call return
 * HUF_ERROR_FATAL on the ranks that did arrive - the object's own communicator is aborted (ncclCommAbort), the object
 * is broken and every later call on it fails at once; hufgpu_shard_destroy() is still to be called.
 *
 *   hufgpu_shard_create   : nccl_comm = an existing ncclComm_t of the ranks (not destroyed with the object; nranks and rank
 *                           are the communicator's), or NULL: then the object makes its own from `id`
 *                           (HUFGPU_SHARD_ID_BYTES from hufgpu_shard_unique_id() on one rank, handed to all by the caller),
 *                           nranks and rank.  ctx = this rank's context: its device is the rank's GPU, and no other work
 *                           may be in flight on it during a sharded call.
 *   hufgpu_encode_sharded : d_in (root: n_total bytes) -> d_stream (root: room for hufgpu_encode_bound(n_total, blocksize)
 *                           bytes); *stream_len and shard_lens[nranks] (host, optional) are filled on EVERY rank.
 *                           HUFGPU_SHARD_INDEX: d_block_offsets (root: hufgpu_block_count(n_total, blocksize) + 1 words)
 *                           receives the block index of the whole stream.
 *   hufgpu_decode_sharded : d_stream + d_block_offsets (root) -> d_out (root: n_total bytes).  The stream is cut into
 *                           nranks shares of about equal compressed BYTES at block borders (hufgpu_shard_plan_decode);
 *                           a rank decodes its blocks from the block index alone.  HUFGPU_SHARD_OWN_LAYOUT: the stream is
 *                           the one this object's last hufgpu_encode_sharded (same root, n_total, blocksize) produced -
 *                           the shards are cut as they were then and every rank uses the block index and the sub-index
 *                           it kept (d_block_offsets is not read).  Errors: the first failing rank's in stream order,
 *                           returned on every rank; *raw_len = bytes in front of it (as hufgpu_decode()).
 *   legs_ms               : optional, 4 doubles: host milliseconds of the call's four legs (scatter, codec, control words,
 *                           gather; decode: plan, scatter, codec + results, gather), each synchronised.
 */
typedef struct hufgpu_shard hufgpu_shard_t;
#define HUFGPU_SHARD_ID_BYTES   128      /* sizeof(ncclUniqueId) */
#define HUFGPU_SHARD_INDEX      0x100u
#define HUFGPU_SHARD_OWN_LAYOUT 0x200u
int hufgpu_shard_unique_id(void *id);
int hufgpu_shard_create(hufgpu_shard_t **sh, hufgpu_ctx_t *ctx, void *nccl_comm, const void *id, int nranks, int rank);
int hufgpu_shard_destroy(hufgpu_shard_t *sh);
int hufgpu_shard_info(const hufgpu_shard_t *sh, int *nranks, int *rank);
const char *hufgpu_shard_last_error(const hufgpu_shard_t *sh);
int hufgpu_shard_set_timeout(hufgpu_shard_t *sh, uint32_t timeout_ms);
int hufgpu_shard_range(uint64_t n_total, uint64_t blocksize, int rank, int nranks, uint64_t *lo, uint64_t *hi);
/* first_block[nranks + 1] from a host copy of the block index (nblocks + 1 offsets, the last = the stream's length) */
int hufgpu_shard_plan_decode(const uint64_t *block_offsets, uint64_t nblocks, int nranks, uint64_t *first_block);
int hufgpu_encode_sharded(hufgpu_shard_t *sh, int root, const void *d_in, uint64_t n_total, uint64_t blocksize,
                          uint32_t flags, void *d_stream, uint64_t stream_cap, uint64_t *d_block_offsets,
                          uint64_t *stream_len, uint64_t *shard_lens, double *legs_ms);
int hufgpu_decode_sharded(hufgpu_shard_t *sh, int root, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_block_offsets, uint64_t n_total, uint64_t blocksize, uint32_t flags,
                          void *d_out, uint64_t out_cap, uint64_t *raw_len, double *legs_ms);

/* A small encode with one synchronisation instead of three: h_in_pinned (n bytes, pinned host memory) -> d_in ->
 * encode -> h_out_pinned: the stream's first hufgpu_encode_bound(n, blocksize) bytes and, 8-byte aligned behind them,
 * its length (h_out_cap >= bound rounded up to 8, + 8).  What huf_encode() uses for memory streams of up to 32 KiB. */
int hufgpu_encode_small(hufgpu_ctx_t *ctx, const void *h_in_pinned, uint64_t n, uint64_t blocksize, void *d_in,
                        void *d_out, uint64_t out_cap, void *h_out_pinned, uint64_t h_out_cap, uint64_t *out_len);

/* The decode's twin of hufgpu_encode_small(): a raw stream of `avail` bytes in PINNED host memory (of which the reference's
 * loop takes blocks while fewer than `length` bytes are consumed, src/decoder.c:218), decoded in order by one workgroup,
 * output and outcome back in pinned host memory, one synchronisation.  d_in: avail bytes of device memory; d_out /
 * out_cap: the device output buffer; h_out_pinned / h_out_cap: min(out_cap, 8 avail + 64) rounded up to 8, + 48 bytes.
 * Returns what hufgpu_decode_stream() returns for the same stream; *raw_len bytes at h_out_pinned are the result. */
int hufgpu_decode_small(hufgpu_ctx_t *ctx, const void *h_in_pinned, uint64_t avail, uint64_t length, uint32_t flags,
                        void *d_in, void *d_out, uint64_t out_cap, void *h_out_pinned, uint64_t h_out_cap,
                        uint64_t *raw_len, uint64_t *consumed);

/* Of the last enqueued hufgpu_decode() / hufgpu_decode_sub(), or the last hufgpu_decode_ranges(): blocks that went through a slower decoder -
 * counters[0] = decoded again by the exact in-order-equivalent decoder (a damaged block, an unusual tree, a stale
 * sub-index), counters[1] = 0 (reserved: it counted the blocks round 4's one-pass decoder handed on).
 * Results never depend on these; they say what a slow decode was slow for.  Synchronises the stream. */
int hufgpu_decode_counters(hufgpu_ctx_t *ctx, uint32_t *counters);

/* How the last hufgpu_decode_ranges() routed its blocks: counters[0] = blocks decoded direct (straight into a slot),
 * [1] = blocks decoded whole into the scratch area, fail-overs of the tile route included, [2] = blocks served by tiles
 * (HUFGPU_RANGES_TILES), [3] = (range, tile) items decoded, [4] = blocks that failed a tile check and were decoded again,
 * [5..7] = 0.  When [4] is not 0 the call was served again by the whole-block route: [0] and [1] are then that run's and
 * [2] is 0.  Results never depend on these.  HUF_ERROR_INVALID_ARGUMENT for a NULL context or array; touches no GPU. */
int hufgpu_ranges_counters(hufgpu_ctx_t *ctx, uint64_t counters[8]);

/* Synchronise and report the outcome of the last enqueued hufgpu_decode() / hufgpu_decode_sub().
 * LIFETIME: d_stream, d_block_offsets and d_out of the enqueued call must stay valid until this returns - when a block
 * failed, this call reads the stream and the index once more and WRITES the failing block's symbols in front of the
 * failure to d_out (what src/decoder.c:69-91 delivers).  After it has returned the library holds none of them. */
int hufgpu_decode_result(hufgpu_ctx_t *ctx, uint64_t *raw_len);

/*
 * Decode a raw stream (no index): `avail` bytes are readable at d_stream, `length` compressed
 * bytes drive the block loop exactly like config->length in src/decoder.c:218.  Block
 * boundaries are discovered on the device: every byte offset is tested for a valid header,
 * every candidate is decoded to find its end (straight into d_out when all candidates together
 * fit it), the chain from offset 0 is followed, blocks that are not in place yet are decoded in
 * parallel and anything else (errors, odd headers, tails) goes to an exact in-order decoder -
 * results, errors and byte counts are those of the reference in every case.  Synchronous.
 * *raw_len bytes of d_out are the result; what lies behind them in d_out is unspecified.
 */
int hufgpu_decode_stream(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length,
                         void *d_out, uint64_t out_cap, uint32_t flags, uint64_t *raw_len,
                         uint64_t *consumed, void *stream);

/*
 * The block index of a raw stream (what hufgpu_decode() wants) without decoding the stream into an output
 * buffer: every candidate header is probed count-only and the chain from offset 0 is walked
 * (kernels/discover.hpp).  *d_index = device array of *nblocks + 1 header offsets owned by the context (valid
 * until its next decode call), the last one = *consumed, the stream offset behind the validated blocks.
 * *nblocks = 0: nothing could be validated (a damaged or tiny stream - hufgpu_decode_stream() reports what is
 * wrong with it).  d_stream must be 16-byte aligned.  For callers that spread the decode of ONE stream over
 * several devices (huf_decode() with HUF_GPU_DEVICES, src/decoder.c:218-276: blocks are independent once found).
 */
int hufgpu_block_index(hufgpu_ctx_t *ctx, const void *d_stream, uint64_t avail, uint64_t length, uint32_t flags,
                       const uint64_t **d_index, uint64_t *nblocks, uint64_t *consumed, void *stream);

/* Of the last hufgpu_decode_stream() call: the stream bytes and output bytes of the blocks that
 * decoded COMPLETELY (on success all of them; after an error the position in front of the failing
 * block - what a caller that feeds a stream piecewise keeps for its next piece). */
int hufgpu_decode_stream_complete(hufgpu_ctx_t *ctx, uint64_t *raw_len, uint64_t *consumed);

/* What the block discovery (kernels/discover.hpp) of the last hufgpu_decode_stream() or hufgpu_block_index() on the
 * context did: counters[0] = 1 if the call went through the discovery at all (0: a stream below the path's threshold, a
 * misaligned one, HUFGPU_SEQUENTIAL, a stream of leading big blocks alone - [1..7] are then 0), [1] = candidate headers
 * found, [2] = candidates the arrays held (= [1] when the call returned without an error), [3] = candidates the lean
 * probe handed to the exact one, [4] = links of the chain that are not "the next candidate" (0: the plain chain, which
 * the walk takes as it stands), [5] = blocks the walk validated, [6] = output bytes the probes left in place for them
 * (~0: none - hufgpu_block_index, an output without room for every candidate, a chain that skips a candidate, no block
 * validated),
 * [7] = passes of the discovery (2: the stream held more candidates than the arrays, and everything ran again with room).
 * Results never depend on these.  HUF_ERROR_INVALID_ARGUMENT for a NULL context or array; touches no GPU. */
int hufgpu_stream_counters(hufgpu_ctx_t *ctx, uint64_t counters[8]);

/* Deterministic synthetic inputs of SURVEY §8d, generated in HBM (kind: 0 const41,
 * 1 uniform256, 2 uniform255, 3 zipf255). `first` = index of the first byte of this shard in
 * the global sequence, so shards of one logical input can be produced on different GPUs. */
int hufgpu_fill(hufgpu_ctx_t *ctx, void *d_out, uint64_t n, int kind, uint64_t seed,
                uint64_t first, void *stream);

/* Plain device memory helpers so that C callers need not link HIP themselves. */
int hufgpu_malloc(hufgpu_ctx_t *ctx, void **d_ptr, uint64_t bytes);
int hufgpu_free(hufgpu_ctx_t *ctx, void *d_ptr);
int hufgpu_memcpy_h2d(hufgpu_ctx_t *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int hufgpu_memcpy_d2h(hufgpu_ctx_t *ctx, void *h_dst, const void *d_src, uint64_t bytes);
int hufgpu_memcpy_d2d(hufgpu_ctx_t *ctx, void *d_dst, const void *d_src, uint64_t bytes);
int hufgpu_synchronize(hufgpu_ctx_t *ctx);

/* Bandwidth calibration: ONE launch of a hand-written kernel that only moves bytes, 16 bytes per lane and access
 * (kernels/fill.hpp) - kind 0: copy d_a -> d_b, 1: read d_a, 2: fill d_b; variant 0 .. HUFGPU_CALIB_VARIANTS - 1 =
 * workgroup shape and cache policy.  bytes: a multiple of 64 KiB; pointers 16-byte aligned.  bench.py times these
 * for the ceilings it prints beside the roofline (what a kernel that reads N and writes N can reach on this part). */
#define HUFGPU_CALIB_VARIANTS 8
int hufgpu_calib_bandwidth(hufgpu_ctx_t *ctx, int kind, int variant, const void *d_a, void *d_b, uint64_t bytes, void *stream);

/* Per-kernel timing. While enabled, every hufgpu_encode/hufgpu_decode call records HIP
 * events around each of its kernels on the stream it launches on (up to 256 calls are kept).
 * enabled: 1 = start a new record, 0 = pause (the record is kept), 2 = resume the record - so a
 * timed loop can sample every n-th call (an event costs ~5 us).  hufgpu_get_profile() returns, for
 * kind 0 = encode or 1 = decode, the per-stage time summed over the recorded calls, in launch order:
 *   encode: [hist256, tree, scan_sizes, pack]     decode: [prepare, decode]
 * (blocks shorter than 4 MiB run hist256 + tree + scan_sizes as ONE kernel: its time is stage 0,
 * stages 1 and 2 are empty).  No host synchronisation happens until hufgpu_get_profile(). */
int hufgpu_set_profiling(hufgpu_ctx_t *ctx, int enabled);
int hufgpu_get_profile(hufgpu_ctx_t *ctx, int kind, float *ms_sum, int max_stages,
                       int *n_stages, int *n_calls);

/* ---- extensions of the host API of include/huffman.h (not in the reference) ----
 * huf_gpu_set_relaxed_tree: 1 = huf_decode() accepts the 1025-entry trees of blocks that use all
 * 256 byte values (the reference's encoder writes them, its decoder returns error 5).
 * huf_gpu_memwrap: a read-only huf_read_writer_t over `length` bytes the caller already holds
 * (no copy into a huf_memopen() buffer); huf_encode()/huf_decode() send such a stream to the
 * device directly.  Close it with huf_memclose(); the bytes are never written or freed. */
struct __huf_read_writer;
struct __huf_encoder_config;
void huf_gpu_set_relaxed_tree(int enabled);
int huf_gpu_memwrap(struct __huf_read_writer **self, const void *data, size_t length);
/* huf_gpu_memwrap_out: a WRITER over `capacity` bytes of memory the caller provides (the buffer that is to hold
 * the result): huf_encode()/huf_decode() write there directly; a write that does not fit fails with
 * HUF_ERROR_MEMORY_ALLOCATION (the memory is never grown, moved or freed).  huf_memlen() = bytes written. */
int huf_gpu_memwrap_out(struct __huf_read_writer **self, void *buffer, size_t capacity);
/* huf_gpu_decode_blocks: huf_decode() for a caller that holds only a PIECE of a stream (a file read
 * in bounded rounds, src/decoder.c:218 has the whole stream behind its reader): the blocks that lie
 * completely inside config->length bytes are decoded and written, *consumed = their stream bytes.
 * A last block that is cut off is not an error here - it is left for the next call (*consumed <
 * config->length; 0 when not even one block is complete); every other error is huf_decode()'s.
 * The reader is never asked for more than config->length bytes. */
int huf_gpu_decode_blocks(const struct __huf_encoder_config *config, uint64_t *consumed);

/* huf_gpu_sessions: huf_encode()/huf_decode() calls hold one SESSION (a device context and its staging
 * buffers) each.  The environment decides how many there are: HUF_GPU_DEVICE=k (default 0) = one
 * session on device k, concurrent calls take turns; HUF_GPU_DEVICES="0,1,2" or "all" = one session per
 * listed device ("0,0" = two on device 0), and concurrent calls - disjoint configs on different
 * threads, parallel in the reference (src/encoder.c:379-392 has no global state) - run side by side
 * on different sessions, so a multi-threaded caller uses every listed GPU.  Returns the sessions that
 * hold a context so far; *configured = the length of the list. */
int huf_gpu_sessions(int *configured);

/* With several sessions configured and free, ONE huf_encode() / huf_decode() between memory streams is spread
 * over them: the encoder deals out rounds of whole blocks, the decoder finds the stream's blocks on one device
 * (hufgpu_block_index) and deals out block ranges balanced by compressed bytes (src/decoder.c:218-276: blocks
 * are independent once found).  Counts of the calls of this process that went that way; returns their sum. */
int huf_gpu_fanouts(int *encodes, int *decodes);

/* huf_gpu_copy_out: memcpy for a binding that must hand a result over as an object of its own (the
 * Python layer's `bytes`): `dst` is fresh memory, where a plain memcpy runs at page-fault speed.
 * Huge-page advice for the destination, then a few threads make their parts present and copy them. */
int huf_gpu_copy_out(void *dst, const void *src, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* INCLUDE_huffman_gpu_h__ */

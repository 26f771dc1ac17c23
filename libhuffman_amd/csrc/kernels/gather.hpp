/* gather.hpp - the kernels of hufgpu_gather (include/huffman_gpu.h): records of the original data out of one indexed
   stream, their positions, lengths, slots and statuses all in device memory; the host knows the sizes of the caller's
   arrays and nothing else, and only enqueues.  Part of hufgpu_kernels.hip (one translation unit, gfx950 only).

   Positions are the layout's: block b holds [b B, b B + min(B, raw_size - b B)), so a record's blocks follow from a
   division and no header has to be read to find them.  A block whose header says another length is not served.

     gather_mark_kernel   one thread a record: its status zeroed, the record cut at raw_size, one count for every block
                          it has bytes in (a part);
     gather_scan_kernel   the counts summed by the two-level / ticket scan of offsets.hpp, the parts in the low half of a
                          word, "the block is touched" in the high half: a block's place in the part list and in the list
                          of touched blocks; the grand total - parts, touched blocks - stays in device memory;
     gather_place_kernel  every touched block into the list, every part into its block's segment;
     gather_serve_kernel  workgroups of eight waves walk the list.  A block's header is parsed and checked and its tables
                          are built ONCE (dsub_fast_tables: the claimed code lengths checked against the stream's tree)
                          however many records fall into it; the waves then take the block's (part, tile) items, one wave
                          an item - the item of sub_tile.hpp, with its checks.  A block of one byte value has no
                          sub-index rows: its parts are fills, once the header and the parts' own payload bits (all
                          zero) have been looked at.

   A block with many items (blocksize = 0: one block holds every record) is the work of `shares` workgroups, each
   with the block's tables of its own: unit u of the walk is share u % shares of touched block u / shares.  The grid is
   fixed by host-known bounds; the number of units is read from device memory.

   Whatever fails - a header that does not parse or is not the layout's, lengths that are not the tree's, a tile check -
   raises the status of the records concerned to HUF_ERROR_READ_WRITE with an atomic max; nothing is decided on the
   host.  Nothing but the first (cut length) bytes of a record's slot is ever written. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "offsets.hpp"
#include "sub_tile.hpp"

namespace hufgpu {

#define GATHER_THREADS 512                  /* as RTILE_THREADS (range_tiles.hpp): decode_sub.hpp's step-by-step functions are instantiated for 512 threads already */
#define GATHER_WAVES (GATHER_THREADS / 64)

/* a record's bytes inside one block */
struct __attribute__((aligned(16))) GatherPart {
    uint64_t start;                         /* first raw position */
    uint64_t dst;                           /* where its first byte goes, from d_out */
    uint32_t n;                             /* bytes */
    uint32_t rec;                           /* the record */
    uint64_t pad_;
};

struct GatherArgs {
    SubStream s;
    uint32_t max_len;
    uint64_t nrecords;
    const uint64_t *pos;
    const uint32_t *len;                    /* NULL: every record has max_len bytes */
    uint8_t *out;
    uint64_t stride;
    int32_t *errs;
    uint32_t *raw_lens;                     /* optional */
    uint32_t *cnt;                          /* [nblocks] parts of the block (zero when the first kernel starts) */
    uint32_t *cur;                          /* [nblocks] parts placed so far (zero when the first kernel starts) */
    TwoLevel scan;                          /* of (touched << 32) + parts; scan.total: the list's length << 32 | all parts */
    uint32_t *list;                         /* the touched blocks */
    GatherPart *parts;
    uint32_t shares;                        /* workgroups a touched block's items are dealt to */
    uint32_t tmax;                          /* tiles a part can have bytes in, at most */
};

/* the record cut at the end of the data: false when nothing of it is to be served */
__device__ __forceinline__ bool gather_record(const GatherArgs &a, uint64_t i, uint64_t &pos, uint32_t &n, bool &too_long)
{
    pos = a.pos[i];
    const uint32_t len = a.len ? a.len[i] : a.max_len;
    too_long = len > a.max_len;
    n = (too_long || pos >= a.s.raw_size) ? 0u : (uint32_t)dmin<uint64_t>(len, a.s.raw_size - pos);
    return n != 0u;
}

__global__ __launch_bounds__(256) void gather_mark_kernel(GatherArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nrecords) return;
    uint64_t pos;
    uint32_t n;
    bool too_long;
    const bool any = gather_record(a, i, pos, n, too_long);
    a.errs[i] = too_long ? HUFE_ARGUMENT : HUFE_OK;
    if (a.raw_lens) a.raw_lens[i] = n;
    if (!any) return;
    const uint64_t fb = pos / a.s.bsize, lb = (pos + n - 1) / a.s.bsize;
    for (uint64_t b = fb; b <= lb; b++) atomicAdd(&a.cnt[b], 1u);
}

/* a workgroup = one SCAN_GROUP of blocks, as decode_prepare_kernel sums the block lengths */
__global__ __launch_bounds__(SCAN_GROUP) void gather_scan_kernel(GatherArgs a)
{
    __shared__ uint64_t s_part[SCAN_GROUP / 64];
    const uint64_t b = (uint64_t)blockIdx.x * SCAN_GROUP + threadIdx.x;
    const uint64_t c = b < a.s.nblocks ? a.cnt[b] : 0u;
    scan_group_publish<SCAN_GROUP>(a.scan, b, a.s.nblocks, c + ((uint64_t)(c != 0) << 32), s_part);
}

/* one thread per block and per record */
__global__ __launch_bounds__(256) void gather_place_kernel(GatherArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.s.nblocks && a.cnt[i] != 0u) a.list[two_level_prefix(a.scan, i) >> 32] = (uint32_t)i;
    if (i >= a.nrecords) return;
    uint64_t pos;
    uint32_t n;
    bool too_long;
    if (!gather_record(a, i, pos, n, too_long)) return;
    const uint64_t fb = pos / a.s.bsize, lb = (pos + n - 1) / a.s.bsize;
    for (uint64_t b = fb; b <= lb; b++) {
        const uint64_t p0 = b * a.s.bsize;
        const uint64_t s = dmax<uint64_t>(pos, p0), e = dmin<uint64_t>(pos + n, p0 + a.s.bsize);
        GatherPart p;
        p.start = s;
        p.dst = i * a.stride + (s - pos);
        p.n = (uint32_t)(e - s);
        p.rec = (uint32_t)i;
        p.pad_ = 0;
        a.parts[(uint32_t)two_level_prefix(a.scan, b) + atomicAdd(&a.cur[b], 1u)] = p;   /* (the order inside a segment is free) */
    }
}

/* n bytes of value v to dst, which has any alignment, by one wave */
__device__ __forceinline__ void gather_fill(uint8_t *__restrict__ dst, uint32_t v, uint32_t n)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t head = dmin<uint32_t>(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint32_t chunks = (n - head) >> 4, tail = (n - head) & 15u;
    if (lane < head) dst[lane] = (uint8_t)v;
    if (lane < tail) dst[head + 16u * chunks + lane] = (uint8_t)v;
    const uint32_t w = v * 0x01010101u;
    v4u x;
    x.x = w; x.y = w; x.z = w; x.w = w;
    v4u *d = reinterpret_cast<v4u *>(dst + head);
    for (uint32_t c = lane; c < chunks; c += 64u) d[c] = x;
}

/* every part of the block is not served here (one workgroup of the block's shares says so) */
__device__ __forceinline__ void gather_fail_block(const GatherArgs &a, uint32_t seg, uint32_t count, uint32_t share)
{
    if (share != 0u) return;
    for (uint32_t p = threadIdx.x; p < count; p += GATHER_THREADS) atomicMax(&a.errs[a.parts[seg + p].rec], (int32_t)HUFE_RW);
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_serve_kernel(GatherArgs a)
{
    typedef DsubShared<GATHER_THREADS> SH;
    __shared__ SH sh;
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[GATHER_WAVES][HUF_SUB_TILE / 4 + 8];
    const uint32_t lane = (uint32_t)lane_id(), wave = uni32(threadIdx.x >> 6);
    uint32_t *tile_words = s_tile[wave];
    uint32_t *top = DsubLds<GATHER_THREADS>::slice(sh, (int)wave) + (SH::SLICE_WORDS - 1u);
    const uint64_t units = (*a.scan.total >> 32) * a.shares;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        __syncthreads();                                            /* the waves are through with the tables of the unit before */
        const uint32_t share = (uint32_t)(u % a.shares);
        const uint64_t b = a.list[u / a.shares];
        const uint32_t count = a.cnt[b], seg = (uint32_t)two_level_prefix(a.scan, b);
        const uint64_t nids = (uint64_t)count * a.tmax;             /* item id = part * tmax + the tile's number inside the part */
        const uint64_t id0 = (uint64_t)share * GATHER_WAVES, idstep = (uint64_t)a.shares * GATHER_WAVES;
        if (id0 >= nids) continue;
        /* ---- the header, as decode_prepare_kernel reads it - and its length must be the layout's ---- */
        const uint64_t p0 = b * a.s.bsize, blen = dmin<uint64_t>(a.s.bsize, a.s.raw_size - p0);
        BlockHeader h;
        if (parse_block_header(a.s.stream, a.s.stream_len, a.s.offsets[b], a.s.offsets[b + 1], a.s.max_tree, h) != HUFE_OK || h.block_len != blen) {
            gather_fail_block(a, seg, count, share);
            continue;
        }
        const SubBlockView v = sub_block_view(h, a.s.sub, b);
        const int leaf = h.tree_len == 5 ? single_leaf_symbol(h.tree) : -1;
        if (leaf >= 0) {
            /* ---- one byte value: every symbol is a 0 bit (decode.hpp), a part is a fill once its own bits are seen to be 0 ---- */
            if (blen > v.pay_bits) {
                gather_fail_block(a, seg, count, share);
                continue;
            }
            for (uint64_t p = id0 + wave; p < count; p += idstep) {
                const GatherPart part = a.parts[seg + p];
                const uint64_t c0 = part.start - p0, c1 = c0 + part.n;
                const uint64_t w0 = c0 >> 5, w1 = (c1 - 1) >> 5;
                bool set = false;
                for (uint64_t w = w0 + lane; w <= w1; w += 64u) {
                    uint32_t x = load_be32(v.pay, 4ull * w, v.pay_bytes);
                    if (w == w0) x &= 0xffffffffu >> (uint32_t)(c0 & 31u);
                    if (w == w1) x &= 0xffffffffu << (31u - (uint32_t)((c1 - 1) & 31u));
                    set |= x != 0u;
                }
                if (__ballot(set) != 0ull) {
                    if (lane == 0) atomicMax(&a.errs[part.rec], (int32_t)HUFE_RW);
                    continue;
                }
                gather_fill(a.out + part.dst, (uint32_t)leaf, part.n);
            }
            continue;
        }
        /* ---- the block's tables, once ---- */
        const DsubTreeWords tw = dsub_tree_request<GATHER_THREADS>(h.tree, h.tree_len, a.s.sub.lens + b * HUF_NSYM);
        if (!dsub_fast_tables<GATHER_THREADS>(sh, h.tree_len, tw)) {  /* (workgroup-uniform) */
            gather_fail_block(a, seg, count, share);
            continue;
        }
        /* ---- the items, one wave each ---- */
        for (uint64_t id = id0 + wave; id < nids; id += idstep) {
            const GatherPart part = a.parts[seg + id / a.tmax];
            const uint64_t c0 = part.start - p0, c1 = c0 + part.n;
            const uint64_t t = c0 / HUF_SUB_TILE + id % a.tmax;
            if (t > (c1 - 1) / HUF_SUB_TILE) continue;
            uint32_t nsym;
            if (!sub_tile_checked<GATHER_THREADS>(sh, top, v, t, reinterpret_cast<uint8_t *>(tile_words), nsym)) {
                if (lane == 0) atomicMax(&a.errs[part.rec], (int32_t)HUFE_RW);
                continue;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   /* the lanes' bytes are in LDS before other lanes read them */
            __builtin_amdgcn_wave_barrier();
            const uint64_t ts = t * HUF_SUB_TILE;
            const uint64_t s0 = dmax<uint64_t>(c0, ts), s1 = dmin<uint64_t>(c1, ts + HUF_SUB_TILE);
            rtile_store(a.out + part.dst + (s0 - c0), tile_words, (uint32_t)(s0 - ts), (uint32_t)(s1 - s0));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   /* ... and read before the next item overwrites them */
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace hufgpu

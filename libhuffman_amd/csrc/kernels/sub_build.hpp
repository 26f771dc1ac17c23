/* sub_build.hpp - the decoder's sub-index (pack.hpp, HufSubIndex) of a stream that came without one, from the stream, its
   block index and the decoded bytes: sub_lens_kernel, sub_groups_kernel, sub_chunk_scan_kernel, sub_tile_add_kernel.
   Part of hufgpu_kernels.hip (one translation unit, gfx950 only). */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../hufgpu_common.h"
#include "util.hpp"
#include "offsets.hpp"
#include "pack.hpp"
#include "hist_chunk.hpp"
#include "decode.hpp"

namespace hufgpu {

/* ======================================================================================
 * What hufgpu_encode_sub writes as a by-product of packing, for a stream nobody packed here: per block the code length of
 * every byte value (`lens`), per group of 32 symbols the payload bits they take (`group_bits`), per tile of 2 048 symbols
 * the payload bit it starts at (`tile_bits`).  The written set is the encoder's (tests/sub_index_ref.py).
 *
 *   sub_lens_kernel        one workgroup a block: header and tree -> the block's 256 code lengths, straight into its row
 *   sub_groups_kernel      one workgroup a block (a chunk of HUF_CHUNK_SYMS from HUF_CHUNKED_FROM on): a lane sums the 32
 *                          code lengths of one group, a wave's 64 groups are a tile; tile starts count from the chunk's start
 *   sub_chunk_scan_kernel  chunked blocks: the chunks' first bits (one workgroup a block) and the block's check
 *   sub_tile_add_kernel    chunked blocks: the chunk's first bit onto its tiles
 *
 * A block is UNBUILT, and counted, when its header or tree does not parse (then nothing of its row is written), when a
 * byte of its data has no code, or when the groups do not add up to the payload the index gives it (then what was written
 * is stale - decode_sub verifies every entry it uses).  A one-symbol block (tree_len == 5) has no entries: skipped.
 * ==================================================================================== */
#define SB_THREADS 256
static_assert(HUF_SUB_GROUP == 32 && HUF_SUB_TILE == 64 * HUF_SUB_GROUP && HUF_CHUNK_SYMS % (SB_THREADS * HUF_SUB_GROUP) == 0,
              "a lane takes a group with two 16-byte loads, a wave a tile, a workgroup's step never straddles chunks");
#define SB_SKIP    0u
#define SB_BUILD   1u
#define SB_UNBUILT 2u
#define SB_MAX_CODE 255u                 /* a length is a byte */
#define SB_CHUNK_BAD (~0ull)             /* a chunk total: a byte of the chunk has no code */

struct SubBuildArgs {
    const uint8_t *stream;
    uint64_t stream_len;
    const uint64_t *offsets;             /* the stream's whole block index */
    const uint8_t *raw;                  /* the decoded bytes of blocks blk0, blk0 + 1 ... back to back */
    uint64_t raw_avail;                  /* bytes of `raw` that may be read */
    uint64_t n, blocksize;               /* of the whole stream: they fix the layout */
    uint64_t blk0;                       /* first block of this launch */
    uint32_t nblk, cpb;                  /* blocks of this launch; chunks a block (1 below HUF_CHUNKED_FROM) */
    int max_tree;
    const int32_t *dec_status;           /* [nblk] of the decode that wrote `raw` (not 0: the block did not decode), or NULL */
    HufSubIndex sub;
    uint32_t *state;                     /* [nblk] SB_* */
    uint64_t *pay_bytes;                 /* [nblk] the payload's size by the index and the header */
    uint64_t *chunk_tot, *chunk_bits;    /* [nblk * cpb], chunked blocks */
    unsigned long long *unbuilt;
};

/* ---- code lengths from the serialised tree ------------------------------------------------------------------------------
 * Entries are in preorder, -1 where a child is missing (src/tree.c:138-227).  With S(i) = open child slots in front of
 * entry i (S(0) = 1, +1 behind a node, -1 behind a marker: decode.hpp), the parent of entry i is the nearest entry in
 * front of it whose S is not larger - entry i - 1 for a left child, the node the left subtree hangs on for a right one.
 * The search skips sixteen entries at a time by their minimum.  A leaf (a node above two markers) then walks to the root
 * and counts: its code length, the wrapped root's bit included.  Taken: any tree that fills its tree_len entries exactly,
 * with leaves 0..255, each at most once, 1 to 255 bits deep. */
__global__ __launch_bounds__(SB_THREADS) void sub_lens_kernel(SubBuildArgs a)
{
    __shared__ int16_t s_ent[1024 + 8];
    __shared__ uint16_t s_S[1024];
    __shared__ uint16_t s_par[1024];
    __shared__ uint16_t s_gmin[64];
    __shared__ uint32_t s_len[HUF_NSYM];
    __shared__ uint32_t s_part[SB_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t lb = blockIdx.x, b = a.blk0 + lb;
    const uint64_t s0 = b * a.blocksize;
    const uint64_t len = dmin<uint64_t>(a.blocksize, a.n - s0);
    BlockHeader h;
    int tl = -1;
    if (!(a.dec_status && a.dec_status[lb] != 0) && lb * a.blocksize + len <= a.raw_avail &&
        parse_block_header(a.stream, a.stream_len, a.offsets[b], a.offsets[b + 1], a.max_tree, h) == HUFE_OK && h.block_len == len)
        tl = h.tree_len;
    tl = (int)uni32((uint32_t)tl);
    if (tl == 5) {                                                   /* one distinct byte: the encoder writes nothing */
        if (tid == 0) a.state[lb] = SB_SKIP;
        return;
    }
    bool bad = tl < 0;
    if (!bad) {
        typedef int16_t __attribute__((aligned(1))) unaligned_i16;
        const unaligned_i16 *ent = reinterpret_cast<const unaligned_i16 *>(h.tree);
        int e[4];
        int x = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = 4 * (int)tid + k;
            e[k] = i < tl ? (int)ent[i] : -1;
            s_ent[i] = (int16_t)e[k];
            if (i < tl) x += e[k] != -1 ? 1 : -1;
        }
        if (tid < 8) s_ent[1024 + tid] = (tid == 0 && tl == 1025) ? ent[1024] : (int16_t)-1;
        uint32_t total;
        int run = 1 + (int)block_excl_scan_u32<SB_THREADS>((uint32_t)x, s_part, total);
        /* every entry fills an open slot and the last one fills the last: S is 1 at least in front of every entry and 0
         * behind the tree (entry 1024, which no thread owns, can only be the marker that closes it) */
        if (tl == 1025) bad = ent[1024] != -1 || 1 + (int)total != 1;
        else bad = 1 + (int)total != 0;
        uint32_t m = 0xffffu;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = 4 * (int)tid + k;
            uint32_t s = 0xffffu;                                    /* behind the tree: never a parent */
            if (i < tl) {
                if (run < 1) bad = true;
                else s = (uint32_t)run;
                run += e[k] != -1 ? 1 : -1;
            }
            s_S[i] = (uint16_t)s;
            m = dmin<uint32_t>(m, s);
        }
        m = dmin<uint32_t>(m, wave_xor_u32<1>(m));
        m = dmin<uint32_t>(m, wave_xor_u32<2>(m));
        if ((tid & 3u) == 0) s_gmin[tid >> 2] = (uint16_t)m;
        if (tid < HUF_NSYM) s_len[tid] = 0;
    }
    bad = __syncthreads_or(bad) != 0;                                /* (s_S, s_gmin and s_ent are written) */
    if (!bad) {
        /* S(0) = 1 is the lowest there is: every search ends at entry 0 at the latest */
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const uint32_t i = 4 * tid + (uint32_t)k;
            if (i == 0 || i >= (uint32_t)tl || s_ent[i] == -1) continue;
            const uint32_t s = s_S[i];
            uint32_t j = i;
            bool found = false;
            while ((j & 15u) != 0) {
                j--;
                if (s_S[j] <= s) { found = true; break; }
            }
            if (!found) {
                uint32_t g = j >> 4;
                do { g--; } while (s_gmin[g] > s);
                j = 16 * g + 16;
                do { j--; } while (s_S[j] > s);
            }
            s_par[i] = (uint16_t)j;
        }
    }
    __syncthreads();
    if (!bad) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const uint32_t i = 4 * tid + (uint32_t)k;
            if (i >= (uint32_t)tl || s_ent[i] == -1 || s_ent[i + 1] != -1 || s_ent[i + 2] != -1) continue;
            const int v = s_ent[i];
            uint32_t d = 0;
            for (uint32_t j = i; j != 0; j = s_par[j]) d++;
            if (v < 0 || v >= HUF_NSYM || d < 1 || d > SB_MAX_CODE) bad = true;
            else if (atomicExch(&s_len[v], d) != 0) bad = true;      /* a byte value on two leaves */
        }
    }
    bad = __syncthreads_or(bad) != 0;
    if (bad) {
        if (tid == 0) {
            a.state[lb] = SB_UNBUILT;
            atomicAdd(a.unbuilt, 1ull);
        }
        return;
    }
    if (tid < 64)
        reinterpret_cast<uint32_t *>(a.sub.lens + b * HUF_NSYM)[tid] =
            s_len[4 * tid] | (s_len[4 * tid + 1] << 8) | (s_len[4 * tid + 2] << 16) | (s_len[4 * tid + 3] << 24);
    if (tid == 0) {
        a.state[lb] = SB_BUILD;
        a.pay_bytes[lb] = h.pay_bytes;
    }
}

/* ---- groups and tiles --------------------------------------------------------------------------------------------------
 * The 256 lengths are the hot structure: one look-up per input byte.  TABLE 0: a byte table, four lengths a dword, read
 * with ds_read_u8 - 64 dwords over the 32 banks a 4-byte read has, so two byte values 128 apart in one half-wave cost a
 * second cycle.  TABLE 1: the same 256 bytes read eight at a time (ds_read_b64 has 64 banks: no two of its 32 pairs
 * share one) and the byte shifted out - no conflicts, two more VALU instructions a byte.  DESIGN.md 5.8 has the
 * measurement that chose. */
template <int TABLE>
__device__ __forceinline__ uint32_t sb_len(const uint8_t *tab, uint32_t v)
{
    if constexpr (TABLE == 0) return tab[v];
    else {
        const uint64_t q = reinterpret_cast<const uint64_t *>(tab)[v >> 3];
        return (uint32_t)(q >> ((v & 7u) * 8u)) & 0xffu;
    }
}

template <int TABLE>
__device__ __forceinline__ void sb_dword(const uint8_t *tab, uint32_t w, uint32_t &sum, uint32_t &least)
{
    const uint32_t l0 = sb_len<TABLE>(tab, w & 0xffu), l1 = sb_len<TABLE>(tab, (w >> 8) & 0xffu),
                   l2 = sb_len<TABLE>(tab, (w >> 16) & 0xffu), l3 = sb_len<TABLE>(tab, w >> 24);
    sum += l0 + l1;
    sum += l2 + l3;
    least = dmin<uint32_t>(least, dmin<uint32_t>(l0, l1));
    least = dmin<uint32_t>(least, dmin<uint32_t>(l2, l3));
}

template <int TABLE>
__global__ __launch_bounds__(SB_THREADS) void sub_groups_kernel(SubBuildArgs a)
{
    typedef uint32_t v4u_any __attribute__((ext_vector_type(4), aligned(1)));      /* the data lies at any byte */
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[HUF_NSYM];
    __shared__ uint32_t s_wave[2][SB_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t lb = blockIdx.x / a.cpb, c = blockIdx.x % a.cpb, b = a.blk0 + lb;
    if (uni32(a.state[lb]) != SB_BUILD) return;
    const uint64_t len = dmin<uint64_t>(a.blocksize, a.n - b * a.blocksize);
    const uint64_t c0 = a.cpb > 1 ? c * (uint64_t)HUF_CHUNK_SYMS : 0;
    if (c0 >= len) {                                                 /* a chunk behind the stream's last, short block */
        if (tid == 0) a.chunk_tot[blockIdx.x] = 0;
        return;
    }
    const uint64_t clen = a.cpb > 1 ? dmin<uint64_t>(HUF_CHUNK_SYMS, len - c0) : len;
    if (tid < 64) reinterpret_cast<uint32_t *>(s_tab)[tid] = reinterpret_cast<const uint32_t *>(a.sub.lens + b * HUF_NSYM)[tid];
    const uint8_t *src = a.raw + lb * a.blocksize + c0;
    uint64_t *tiles = a.sub.tile_bits + b * a.sub.tpb + c0 / HUF_SUB_TILE;
    uint16_t *groups = a.sub.group_bits + b * a.sub.gpb + c0 / HUF_SUB_GROUP;
    const uint64_t ngroups = (clen + HUF_SUB_GROUP - 1) / HUF_SUB_GROUP;
    uint64_t run = 0;                                                /* bits of the chunk in front of this step's four tiles */
    uint32_t least = 255u;
    int buf = 0;
    __syncthreads();
    for (uint64_t g0 = 0; g0 < ngroups; g0 += SB_THREADS, buf ^= 1) {
        const uint64_t g = g0 + tid;
        uint32_t bits = 0;
        if (g < ngroups) {
            const uint8_t *p = src + g * HUF_SUB_GROUP;
            if (clen - g * HUF_SUB_GROUP >= HUF_SUB_GROUP) {
                const v4u_any v0 = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(p));
                const v4u_any v1 = __builtin_nontemporal_load(reinterpret_cast<const v4u_any *>(p + 16));
                sb_dword<TABLE>(s_tab, v0.x, bits, least);
                sb_dword<TABLE>(s_tab, v0.y, bits, least);
                sb_dword<TABLE>(s_tab, v0.z, bits, least);
                sb_dword<TABLE>(s_tab, v0.w, bits, least);
                sb_dword<TABLE>(s_tab, v1.x, bits, least);
                sb_dword<TABLE>(s_tab, v1.y, bits, least);
                sb_dword<TABLE>(s_tab, v1.z, bits, least);
                sb_dword<TABLE>(s_tab, v1.w, bits, least);
            } else {                                                 /* the block's last group: byte by byte, nothing behind the data is read */
                const uint32_t nsym = (uint32_t)(clen - g * HUF_SUB_GROUP);
                for (uint32_t k = 0; k < nsym; k++) {
                    const uint32_t l = s_tab[p[k]];
                    bits += l;
                    least = dmin<uint32_t>(least, l);
                }
            }
        }
        const uint32_t incl = wave_incl_scan_u32(bits);
        if (lane == 63) s_wave[buf][wave] = incl;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (uint32_t i = 0; i < SB_THREADS / 64; i++) {
            const uint32_t x = s_wave[buf][i];
            if (i < wave) pre += x;
            tot += x;
        }
        if (g < ngroups) {
            groups[g] = (uint16_t)bits;
            if (lane == 0) tiles[g / 64] = run + pre;
        }
        run += tot;
    }
    const bool nocode = __syncthreads_or(least == 0u) != 0;
    if (tid != 0) return;
    if (a.cpb > 1) a.chunk_tot[blockIdx.x] = nocode ? SB_CHUNK_BAD : run;
    else if (nocode || ((run + 7u) >> 3) != a.pay_bytes[lb]) atomicAdd(a.unbuilt, 1ull);
}

/* chunked blocks: first payload bit of every chunk, and the block's check against its payload */
template <int THREADS>
__global__ __launch_bounds__(THREADS) void sub_chunk_scan_kernel(SubBuildArgs a)
{
    const uint64_t lb = blockIdx.x;
    if (uni32(a.state[lb]) != SB_BUILD) return;
    const uint64_t *src = a.chunk_tot + lb * a.cpb;
    bool nocode = false;
    const uint64_t total = chunked_excl_scan<THREADS>(a.cpb, a.chunk_bits + lb * a.cpb, [src, &nocode](uint64_t i) {
        const uint64_t v = src[i];
        if (v == SB_CHUNK_BAD) nocode = true;
        return v == SB_CHUNK_BAD ? 0ull : v;
    });
    nocode = __syncthreads_or(nocode) != 0;
    if (threadIdx.x == 0 && (nocode || ((total + 7u) >> 3) != a.pay_bytes[lb])) atomicAdd(a.unbuilt, 1ull);
}

/* chunked blocks: a chunk's tiles count from the block's first payload bit (one thread a tile) */
__global__ __launch_bounds__(HUF_CHUNK_SYMS / HUF_SUB_TILE) void sub_tile_add_kernel(SubBuildArgs a)
{
    const uint64_t lb = blockIdx.x / a.cpb, c = blockIdx.x % a.cpb, b = a.blk0 + lb;
    if (c == 0 || uni32(a.state[lb]) != SB_BUILD) return;
    const uint64_t len = dmin<uint64_t>(a.blocksize, a.n - b * a.blocksize);
    const uint64_t t = c * (HUF_CHUNK_SYMS / HUF_SUB_TILE) + threadIdx.x;
    if (t * HUF_SUB_TILE < len) a.sub.tile_bits[b * a.sub.tpb + t] += a.chunk_bits[blockIdx.x];
}

}  // namespace hufgpu

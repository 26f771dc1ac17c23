"""A CPU reference of the encoder's sub-index (hufgpu_encode_sub, kernels/pack.hpp and pack_chunk.hpp), and the table of
cases test_gpu_sub_index_content.py compares the encoder with.  Test infrastructure (CPU, numpy).

Layout (csrc/host/encode.hpp, sub_index_view / hufgpu_sub_index_bytes).  blocksize 0 means one block of all n symbols.  With
nb blocks, tpb = ceil(blocksize / 2 048) tiles and gpb = ceil(blocksize / 32) groups rounded up to a multiple of 8 a block,
the buffer holds, in this order:
  tile_bits   u64[nb][tpb]    the payload bit where tile t of the block starts (symbol 2 048 t)
  group_bits  u16[nb][gpb]    the payload bits of group g of the block (symbols 32 g .. 32 g + 31, fewer in the last)
  lens        u8 [nb][256]    the code length of every byte value in the block, 0 for a value that does not occur
Because gpb is a multiple of 8, `lens` starts a multiple of 16 bytes behind `group_bits` (8-byte aligned in the buffer:
the tiles may end on an odd word).  Code lengths are those of the block's serialised tree,
the wrapped root's bit included (what the payload holds).

The written set: the entries the encoder defines.  Taken from the writers, not from their output:
  - a block of two or more distinct bytes: every tile and every group that holds at least one of the block's symbols
    (pack.hpp and pack_chunk.hpp store them only when the lane's `nsym` is not 0), and all 256 `lens`;
  - a block of one distinct byte (tree_len == 5): nothing at all - pack_header / pack_segment return before any store,
    and the `lens` loop is skipped;
  - the groups that pad gpb to a multiple of 8, and the tiles and groups behind a short last block, are never written.
Everything outside the written set keeps whatever the caller's buffer held.

Decoding with the encoder's own sub-index (decode_sub.hpp) sends no block to the exact decoder, except - by design - a
block with a code longer than 32 bits: dsub_fast_tables rejects a claimed length d > 32 (`if (d < 2u || d > 32u) ok =
false`), and decode_sub_kernel lists the block for decode_fix_kernel.  `SubCase.fix` pins that count for every case.
"""
from __future__ import annotations

import dataclasses
import zlib

import numpy as np

from decode_edge_cases import block_facts

GROUP = 32                              # HUF_SUB_GROUP (pack.hpp)
TILE = 2048                             # HUF_SUB_TILE
NSYM = 256

# path thresholds of encode_impl (csrc/host/encode.hpp)
HL_MIN_BLOCK = 32768                    # kernels/hist_lanes.hpp: below it the fused hist_tree_kernel
SHORT_MAX = 121392                      # the SHORT pack_kernel: no code longer than 24 bits
CHUNKED_FROM = 1 << 21                  # HUF_CHUNKED_FROM (kernels/hist_chunk.hpp): pack_chunk_kernel
BIG_BLOCK = 1 << 22                     # HUF_BIG_BLOCK: tree_kernel with 64-bit keys
CHUNK_SYMS = 262144                     # HUF_CHUNK_SYMS
DSUB_MAX_CODE = 32                      # decode_sub.hpp, dsub_fast_tables: longer claimed lengths fail the check


# ---- layout ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Layout:
    nb: int
    tpb: int
    gpb: int
    tile_off: int
    group_off: int
    lens_off: int
    size: int


def layout(n: int, blocksize: int) -> Layout:
    if n == 0:
        return Layout(0, 0, 0, 0, 0, 0, 0)
    bs = blocksize or n
    nb = -(-n // bs)
    tpb = -(-bs // TILE)
    gpb = (-(-bs // GROUP) + 7) & ~7
    group_off = nb * tpb * 8
    lens_off = group_off + nb * gpb * 2
    return Layout(nb, tpb, gpb, 0, group_off, lens_off, lens_off + nb * NSYM)


# ---- the expected sub-index -----------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Expected:
    lay: Layout
    tiles: np.ndarray                   # u64[nb * tpb]
    groups: np.ndarray                  # u16[nb * gpb]
    lens: np.ndarray                    # u8 [nb * 256]
    w_tiles: np.ndarray                 # bool: the written set, per array
    w_groups: np.ndarray
    w_lens: np.ndarray
    facts: list                         # block_facts() of every block, in order
    block_syms: list                    # (first symbol, length) of every block


def expected(stream: np.ndarray, offsets: np.ndarray, data: np.ndarray, blocksize: int) -> Expected:
    """The sub-index of `data` encoded in blocks of `blocksize` into `stream` (the oracle's) with block `offsets`."""
    n = data.size
    bs = blocksize or n
    lay = layout(n, blocksize)
    assert offsets.size == lay.nb + 1
    tiles = np.zeros(lay.nb * lay.tpb, np.uint64)
    groups = np.zeros(lay.nb * lay.gpb, np.uint16)
    lens = np.zeros(lay.nb * NSYM, np.uint8)
    w_tiles = np.zeros(tiles.size, bool)
    w_groups = np.zeros(groups.size, bool)
    w_lens = np.zeros(lens.size, bool)
    facts, block_syms = [], []
    for b in range(lay.nb):
        f = block_facts(stream[int(offsets[b]):int(offsets[b + 1])])
        s0, ln = b * bs, min(bs, n - b * bs)
        assert f["len"] == ln, (b, f["len"], ln)
        facts.append(f)
        block_syms.append((s0, ln))
        lut = np.zeros(NSYM, np.int64)
        for v, L in f["code_len"].items():
            lut[v] = L
        bits = lut[data[s0:s0 + ln]]                                   # int64 per symbol
        ng, nt = -(-ln // GROUP), -(-ln // TILE)
        g = np.zeros(ng * GROUP, np.int64)
        g[:ln] = bits
        g = g.reshape(ng, GROUP).sum(axis=1)
        assert g.max() < 1 << 16
        front = np.concatenate([np.zeros(1, np.int64), np.cumsum(bits, dtype=np.int64)])
        groups[b * lay.gpb:b * lay.gpb + ng] = g
        tiles[b * lay.tpb:b * lay.tpb + nt] = front[np.arange(nt, dtype=np.int64) * TILE]
        lens[b * NSYM:(b + 1) * NSYM] = lut
        if f["tree_len"] != 5:
            w_groups[b * lay.gpb:b * lay.gpb + ng] = True
            w_tiles[b * lay.tpb:b * lay.tpb + nt] = True
            w_lens[b * NSYM:(b + 1) * NSYM] = True
    return Expected(lay, tiles, groups, lens, w_tiles, w_groups, w_lens, facts, block_syms)


def views(buf: np.ndarray, lay: Layout):
    """(tiles, groups, lens) of the bytes of a sub-index buffer"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    return (buf[lay.tile_off:lay.group_off].view("<u8"), buf[lay.group_off:lay.lens_off].view("<u2"),
            buf[lay.lens_off:lay.size])


def mismatches(buf: np.ndarray, exp: Expected, limit: int = 8) -> list:
    """[(block, array, index inside the block, found, expected)] of written entries that differ"""
    out = []
    lay = exp.lay
    for name, got, want, w, per in zip(("tile_bits", "group_bits", "lens"), views(buf, lay),
                                       (exp.tiles, exp.groups, exp.lens), (exp.w_tiles, exp.w_groups, exp.w_lens),
                                       (lay.tpb, lay.gpb, NSYM)):
        for i in np.flatnonzero(w & (got != want))[:limit]:
            out.append((int(i) // per, name, int(i) % per, int(got[i]), int(want[i])))
    return out


def unwritten_changed(buf: np.ndarray, fill: np.ndarray, exp: Expected, limit: int = 8) -> list:
    """[(block, array, index inside the block, found, what the buffer held)] of entries outside the written set that
    changed"""
    out = []
    lay = exp.lay
    for name, got, was, w, per in zip(("tile_bits", "group_bits", "lens"), views(buf, lay), views(fill, lay),
                                      (exp.w_tiles, exp.w_groups, exp.w_lens), (lay.tpb, lay.gpb, NSYM)):
        for i in np.flatnonzero(~w & (got != was))[:limit]:
            out.append((int(i) // per, name, int(i) % per, int(got[i]), int(was[i])))
    return out


# ---- paths and writers ----------------------------------------------------------------------------------------------------
def path_of(n: int, blocksize: int) -> str:
    """encode_impl's route for blocks of `blocksize` (0: one block of n)"""
    bs = blocksize or n
    if bs < HL_MIN_BLOCK:
        return "fused"                  # hist_tree_kernel, SHORT pack_kernel
    if bs <= SHORT_MAX:
        return "lanes_short"            # hist_lanes_kernel + tree_wave_kernel, SHORT pack_kernel
    if bs < CHUNKED_FROM:
        return "lanes_full"             # hist_lanes_kernel + tree_wave_kernel, full pack_kernel
    if bs < BIG_BLOCK:
        return "chunked32"              # chunk counts, tree_wave_kernel, pack_chunk_kernel
    return "chunked64"                  # chunk counts, tree_kernel<uint64_t>, pack_chunk_kernel


def writer_of(path: str, max_len: int) -> str:
    """the pack function whose stores write a block's tiles and groups (pack_kernel / pack_chunk_kernel)"""
    if path.startswith("chunked"):
        return "pack_segment<0>" if max_len <= 16 else ("pack_segment<1>" if max_len <= 24 else "pack_segment<2>")
    if max_len <= 10:
        return "pack_block_multi<3>"
    if max_len <= 15:
        return "pack_block_multi<2>"
    if path != "lanes_full" or max_len <= 24:
        return "pack_block<uint32_t>"
    return "pack_block<hufcode_t>"


CLASSES = {"le10": (1, 10), "11_15": (11, 15), "16_24": (16, 24), "gt24": (25, 64),
           "le16": (1, 16), "17_24": (17, 24)}


# ---- data ---------------------------------------------------------------------------------------------------------------
FIB = [1, 1]
while len(FIB) < 60:
    FIB.append(FIB[-1] + FIB[-2])


def deepest(n: int) -> int:
    """the longest code (root bit included) chain() can give a block of n symbols"""
    m = 1
    while sum(FIB[:m + 1]) <= n:
        m += 1
    return m


def chain(rng, n: int, depth: int) -> np.ndarray:
    """n symbols whose longest code is `depth` bits: Fibonacci counts over `depth` byte values (a chain of merges), the
    rest of n on the most frequent one"""
    assert 2 <= depth <= deepest(n), (n, depth)
    cnt = list(FIB[:depth])
    cnt[-1] += n - sum(cnt)
    vals = rng.permutation(NSYM)[:depth]
    out = np.repeat(vals.astype(np.uint8), cnt)
    rng.shuffle(out)
    return out


def all_values(rng, n: int) -> np.ndarray:
    """n symbols in which every byte value occurs (k = 256), otherwise uniform"""
    assert n >= NSYM
    out = np.concatenate([np.arange(NSYM, dtype=np.uint8), rng.integers(0, NSYM, n - NSYM, dtype=np.uint8)])
    rng.shuffle(out)
    return out


def two_values(rng, n: int) -> np.ndarray:
    v = rng.permutation(NSYM)[:2].astype(np.uint8)
    out = np.where(rng.random(n) < 0.3, v[0], v[1]).astype(np.uint8)
    out[0], out[-1] = v[0], v[1]
    return out


CLASS_DEPTH = {"11_15": 13, "17_24": 21}


def class_data(rng, cls: str, n: int) -> np.ndarray:
    if cls in ("le10", "le16"):          # (every byte value, uniform: 9 or 10 bits once a value occurs ~64 times)
        return all_values(rng, n) if n >= 64 * NSYM else rng.integers(0, 64, n, dtype=np.uint8)
    if cls == "16_24":
        return chain(rng, n, min(22, deepest(n)))
    if cls == "gt24":
        return chain(rng, n, deepest(n))
    return chain(rng, n, CLASS_DEPTH[cls])


# ---- the case table -------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class SubCase:
    name: str
    path: str                           # claimed route (path_of)
    cls: str                            # the max_len class of the "cls" blocks (CLASSES)
    blocksize: int
    blocks: list                        # [(kind, length)]: kind in cls, k1, k2, k256; the last one may be short
    dev_offsets: tuple = (0,)           # where the input lies inside a larger device tensor
    fix: int = 0                        # blocks decode_sub hands to the exact decoder (codes over 32 bits only)

    @property
    def n(self) -> int:
        return sum(ln for _, ln in self.blocks)

    def data(self) -> np.ndarray:
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        parts = []
        for kind, ln in self.blocks:
            if kind == "cls":
                parts.append(class_data(rng, self.cls, ln))
            elif kind == "k1":
                parts.append(np.full(ln, rng.integers(0, NSYM), np.uint8))
            elif kind == "k2":
                parts.append(two_values(rng, ln))
            else:
                parts.append(all_values(rng, ln))
        return np.concatenate(parts)


def tail_len(bs: int) -> int:
    """a short last block: not a multiple of 32 (nor, then, of 2 048)"""
    t = bs // 3 + 7
    return t + 1 if t % GROUP == 0 else t


# one blocksize per path takes its input at device offsets 3 and 13 (pack's unaligned loads, every lane)
MATRIX = [
    # path, blocksizes, classes, the blocksize of unaligned inputs
    ("fused", [31, 32, 2047, 2048, 2049, 32767], ["le10", "11_15", "16_24"], 2049),
    ("lanes_short", [32768, 65536, 121392], ["le10", "11_15", "16_24"], 65536),
    ("lanes_full", [121393, 1 << 20, (2 << 20) - 1], ["le10", "11_15", "16_24", "gt24"], 1 << 20),
    ("chunked32", [2 << 20, (2 << 20) + 1, (3 << 20) + 2049], ["le16", "17_24", "gt24"], (2 << 20) + 1),
    ("chunked64", [4 << 20, (5 << 20) + 3, 0], ["le16", "17_24", "gt24"], (5 << 20) + 3),
]
ONE_BLOCK_N = (9 << 20) + 77            # blocksize 0: the whole input is one block


def fits(cls: str, bs: int) -> bool:
    """the class can be reached by a full block of bs symbols"""
    lo, _ = CLASSES[cls]
    if cls in ("le10", "le16"):
        return True
    return deepest(bs) >= max(lo, CLASS_DEPTH.get(cls, lo))


def cases() -> list:
    out = []
    for path, sizes, classes, unaligned in MATRIX:
        for bs in sizes:
            for cls in classes:
                if bs == 0:
                    blocks = [("cls", ONE_BLOCK_N)]
                    full = ONE_BLOCK_N
                else:
                    full = bs
                    if not fits(cls, bs):
                        continue
                    if path.startswith("chunked"):
                        blocks = [("cls", bs), ("k1", bs), ("k2", bs), ("cls", tail_len(bs))]
                    elif bs < NSYM:
                        blocks = [("cls", bs), ("k1", bs), ("cls", bs), ("k2", bs), ("cls", bs), ("cls", tail_len(bs))]
                    else:
                        blocks = [("cls", bs), ("k1", bs), ("k256", bs), ("k2", bs), ("cls", bs), ("cls", tail_len(bs))]
                    if bs == 2049 and cls == "le10":
                        blocks[-1] = ("cls", 1)                     # a block of one symbol
                fix = 1 if cls == "gt24" and deepest(full) > DSUB_MAX_CODE else 0
                out.append(SubCase(f"{path}_{bs}_{cls}", path, cls, bs, blocks,
                                   (3, 13) if bs == unaligned else (0,), fix))
    return out


def check_claims(case: SubCase, stream: np.ndarray, offsets: np.ndarray, data: np.ndarray) -> list:
    """Asserts that the case keeps to its path and classes on the oracle's stream; returns the writers its blocks use."""
    assert path_of(data.size, case.blocksize) == case.path, case.name
    lay = layout(data.size, case.blocksize)
    assert lay.nb == len(case.blocks) and offsets.size == lay.nb + 1, case.name
    bs = case.blocksize or data.size
    lo, hi = CLASSES[case.cls]
    writers, fix = [], 0
    for b, (kind, ln) in enumerate(case.blocks):
        f = block_facts(stream[int(offsets[b]):int(offsets[b + 1])])
        tag = (case.name, b, kind)
        assert f["len"] == ln, tag
        if b < lay.nb - 1:
            assert ln == bs, tag
        if kind == "k1":
            assert f["K"] == 1 and f["tree_len"] == 5, tag
        elif kind == "k2":
            assert f["K"] == 2 and set(f["code_len"].values()) == {2}, tag
        elif kind == "k256":
            assert f["K"] == 256, tag
        elif ln == bs:                                          # a full block of the class
            assert lo <= f["max_code"] <= hi, tag + (f["max_code"],)
        else:                                                   # the short last block
            assert ln % GROUP != 0 and ln % TILE != 0 or ln == 1, tag
        if f["K"] >= 2:
            writers.append(writer_of(case.path, f["max_code"]))
            fix += f["max_code"] > DSUB_MAX_CODE
    assert fix == case.fix, (case.name, fix, case.fix)
    return writers

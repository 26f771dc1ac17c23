"""GPU tests of the tile route of hufgpu_decode_ranges (HUFGPU_RANGES_TILES; GpuCodec.decode_ranges(..., tiles=True)):
of a block at a range's cut edge only the sub-index tiles that hold bytes of the range are decoded.

Bit-exact, no tolerance.  Every successful call with the flag is compared three ways: with slices of the input, with the
same call without the flag (the whole buffer, errs, raws), and with the counters a model of the routing rule expects
(include/huffman_gpu.h: direct / staged whole / served by tiles / (range, tile) items / failed a tile check).  Output
buffers are filled with 0xA5 first; the bytes between and behind the slots must still hold it.
"""
import numpy as np
import pytest

from libhuffman_amd import datagen
from stream_support import GUARD, Enc, dev, make, max_code_len, touched
from stream_support import ranges_route_model as model
from test_gpu_ranges import check_all_good, slots_for

pytestmark = pytest.mark.gpu

TILE, GROUP = 2048, 32
HUFE_OK, HUFE_MEMORY = 0, 1


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    yield c
    c.close()


# ---- inputs ------------------------------------------------------------------------------------------------------------
def encode(torch, codec, kind, n, bs):
    enc = Enc(torch, codec, make(kind, n, bs), bs, sub=True)
    enc.codec, enc.kind = codec, kind
    enc.raw_size, enc.row_bs = enc.n, enc.bs            # the layout the sub-index rows are addressed by
    enc.block_lens = np.diff(enc.P)
    enc.elig = np.full(enc.nb, kind != "const41")      # (the header length is the layout's in all of these)
    return enc


def call(torch, codec, enc, ranges, oo, tiles, relaxed=False, sub_index="own"):
    out = torch.full((oo[-1] + 9,), GUARD, dtype=torch.uint8, device="cuda")
    kw = {}
    if sub_index is not None:
        kw = dict(sub_index=enc.sub if isinstance(sub_index, str) else sub_index, raw_size=enc.raw_size, blocksize=enc.row_bs)
    _, errs, raws = codec.decode_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges, out=out, out_offsets=oo,
                                        relaxed=relaxed, tiles=tiles, **kw)
    return out.cpu().numpy(), errs, raws


def three_ways(torch, codec, enc, ranges, relaxed=False, oo=None):
    """a successful call with the flag: the input's slices, the call without the flag, the counters; returns the counters"""
    oo = slots_for(ranges, enc.n) if oo is None else oo
    ref = call(torch, codec, enc, ranges, oo, False, relaxed)
    d0, s0 = codec.ranges_counters()[:2]
    got = call(torch, codec, enc, ranges, oo, True, relaxed)
    cnt = codec.ranges_counters()
    check_all_good(enc, ranges, got[0], got[1], got[2], oo)
    assert got[1:] == ref[1:] and np.array_equal(got[0], ref[0]), "differs from the call without the flag"
    direct, staged, tiles, items = model(enc, ranges, oo)
    assert cnt == (direct, staged, tiles, items, 0, 0, 0, 0), (cnt, (direct, staged, tiles, items))
    assert (d0, s0) == (direct, staged + tiles), "without the flag the tile blocks are staged"
    return cnt


# ---- shapes and ranges -------------------------------------------------------------------------------------------------
BIG = 3 * (1 << 20) + 77
SHAPES = {"bs4096": (4096, 9 * 4096 + 1500), "bs65536": (65536, 5 * 65536 + 1000), "oneblock": (0, BIG)}
# (which inputs in which shapes: every input in the small blocks, the tables' paths in all three)
CASES = [("zipf255", "bs4096"), ("zipf255", "bs65536"), ("zipf255", "oneblock"), ("two", "bs4096"), ("two", "bs65536"),
         ("l2", "bs4096"), ("l2", "bs65536"), ("l2", "oneblock"), ("long", "bs65536"), ("long", "oneblock"),
         ("uniform256", "bs4096"), ("uniform256", "bs65536"), ("const41", "bs4096"), ("const41", "bs65536")]

_cache = {}


def encoded(torch, codec, kind, shape):
    """one encode per (input, shape) for the whole module; the tests never change it"""
    if (kind, shape) not in _cache:
        bs, n = SHAPES[shape]
        _cache[kind, shape] = encode(torch, codec, kind, n, bs)
    return _cache[kind, shape]


def edge_ranges(bs, n):
    b = bs or n                                         # block length
    last0 = (n - 1) // b * b                            # where the last block starts
    t = b + 3 * TILE if n > b + 4 * TILE else TILE       # a tile start inside a block that has several
    r = [(0, 1), (n - 1, n), (GROUP - 1, GROUP), (t + 31, t + 32),          # one byte: first, last, a group's last
         (t + 3, t + 20), (t + 20, t + 45), (t + TILE - 9, t + TILE + 9),   # inside a group, across groups, across tiles
         (t, t + TILE),                                                      # exactly one tile
         (5, 5), (n, n + 9), (n + 3, n + 8), (n - 10, n + 100),              # empty, past the end
         (t + 100, t + 300), (t + 100, t + 300),                             # the same range twice
         (t + TILE + 5, t + TILE + 10), (t + TILE + 900, t + TILE + 1000)]   # two ranges in one tile
    if bs:
        r += [(bs - 7, bs + 7),                                              # across a block border
              (bs - 100, 3 * bs + 100),                                      # ... two edges by tiles, whole blocks between them direct
              (3 * bs, 4 * bs),                                              # exactly one block: direct
              (last0, n), (last0 - 3, n)]                                    # the whole short last block, and with its neighbour's end
    return r


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_edge_ranges(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    relaxed = kind == "uniform256"
    ranges = edge_ranges(enc.bs, enc.n)
    cnt = three_ways(torch_mod, codec, enc, ranges, relaxed)
    if kind == "const41":
        assert cnt[2] == 0 and cnt[1] > 0               # one-symbol blocks have no sub-index rows: the old route
    else:
        assert cnt[2] > 0 and cnt[3] >= cnt[2]
    if kind == "l2":
        assert 12 < max_code_len(enc) <= 18
    if kind == "long":
        # codes beyond 18 bits go through the step-by-step path's binary search over the leaves inside the tile route:
        # the blocks are SERVED BY TILES and none fails over (cnt[4] == 0 above)
        assert max_code_len(enc) > 18 and cnt[2] > 0
    # each range alone: one range inside an eligible block is that block by tiles, nothing staged
    for lo, hi in ranges[:8]:
        c = three_ways(torch_mod, codec, enc, [(lo, hi)], relaxed)
        fb, lb = touched(enc, lo, hi)
        if kind != "const41" and fb == lb and hi - lo < enc.block_lens[fb]:
            p0 = int(enc.P[fb])
            assert c == (0, 0, 1, (hi - 1 - p0) // TILE - (lo - p0) // TILE + 1, 0, 0, 0, 0)


def test_exactly_one_block_is_direct(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs65536")
    assert three_ways(torch_mod, codec, enc, [(65536, 2 * 65536)]) == (1, 0, 0, 0, 0, 0, 0, 0)
    # both edges by tiles, the two whole blocks between them direct
    assert three_ways(torch_mod, codec, enc, [(65536 - 100, 3 * 65536 + 100)]) == (2, 0, 2, 2, 0, 0, 0, 0)


def test_pairs_decide(torch_mod, codec):
    """a block of 4 KiB has 2 tiles: three ranges over both are 6 pairs - staged whole; two ranges of one tile each are 2"""
    enc = encoded(torch_mod, codec, "zipf255", "bs4096")
    p = 3 * 4096
    assert three_ways(torch_mod, codec, enc, [(p + 10, p + 4000), (p + 2000, p + 2100), (p + 1, p + 4095)]) == (0, 1, 0, 0, 0, 0, 0, 0)
    assert three_ways(torch_mod, codec, enc, [(p + 10, p + 2000), (p + 2048, p + 4096)]) == (0, 0, 1, 2, 0, 0, 0, 0)
    assert three_ways(torch_mod, codec, enc, [(p + 10, p + 2049), (p + 2048, p + 4096)]) == (0, 1, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("kind,shape", [("zipf255", "bs4096"), ("l2", "bs65536"), ("zipf255", "oneblock"), ("long", "oneblock")])
def test_hundreds_of_random_ranges(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    rng = np.random.default_rng(11)
    lo = rng.integers(0, enc.n - 300, 400)
    ranges = [(int(x), int(x) + int(rng.integers(1, 301))) for x in lo]
    oo = slots_for(ranges, enc.n, gaps=(13, 0, 7, 1, 16, 3, 2, 5), lead=3)       # odd slot addresses
    three_ways(torch_mod, codec, enc, ranges, oo=oo)


def test_a_long_range_inside_one_block(torch_mod, codec):
    """hundreds of tiles of one range: several workgroups, the interior tiles' wide stores at every slot alignment"""
    enc = encoded(torch_mod, codec, "zipf255", "oneblock")
    for lead in (0, 1, 7, 16):
        ranges = [(TILE * 3 + 5, TILE * 900 + 1111)]
        oo = slots_for(ranges, enc.n, lead=lead)
        assert three_ways(torch_mod, codec, enc, ranges, oo=oo) == (0, 0, 1, 898, 0, 0, 0, 0)


# ---- sub-index contents with the flag ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["bs4096", "bs65536", "oneblock"])
def test_foreign_sub_index(torch_mod, codec, shape):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", shape)
    rng = np.random.default_rng(13)
    ranges = edge_ranges(enc.bs, enc.n)
    oo = slots_for(ranges, enc.n)
    ref = call(torch, codec, enc, ranges, oo, False)
    _, _, tiles, items = model(enc, ranges, oo)
    # a bit count of 0 or of 65 535 cannot be that of 32 codewords: every tile fails its checks, every block fails over
    for name, sub in (("zeros", torch.zeros_like(enc.sub)), ("ones", torch.full_like(enc.sub, -1))):
        got = call(torch, codec, enc, ranges, oo, True, sub_index=sub)
        cnt = codec.ranges_counters()
        assert got[1:] == ref[1:] and np.array_equal(got[0], ref[0]), name
        assert cnt[2:5] == (0, items, tiles) and tiles > 0, (name, cnt)
    # contents that may pass by chance: no byte outside the cut slots, no more delivered than asked for
    other = encode(torch, codec, "two", enc.n, enc.bs)
    for name, sub in (("random", torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()), ("stale", other.sub)):
        got, errs, raws = call(torch, codec, enc, ranges, oo, True, sub_index=sub)
        want = np.full(got.size, GUARD, np.uint8)
        for i, (lo, hi) in enumerate(ranges):
            cut = min(hi, enc.n) - min(lo, enc.n)
            assert raws[i] <= cut, (name, i)
            got[oo[i]:oo[i] + cut] = GUARD
        assert np.array_equal(got, want), f"{name}: bytes outside the cut slots written"


# ---- damage ------------------------------------------------------------------------------------------------------------
def payload_byte_of(enc, pos):
    """the stream byte that holds the first payload bit of the group of raw position `pos` (from the sub-index)"""
    nbytes = enc.codec.sub_index_bytes(enc.n, enc.bs)
    raw = enc.sub.cpu().numpy().view(np.uint8)[:nbytes]
    b = enc.bs or enc.n
    tpb, gpb = (b + TILE - 1) // TILE, ((b + GROUP - 1) // GROUP + 7) & ~7
    tile_bits = raw[:8 * enc.nb * tpb].view(np.uint64)
    group_bits = raw[8 * enc.nb * tpb:8 * enc.nb * tpb + 2 * enc.nb * gpb].view(np.uint16)
    k, r = pos // b, pos % b
    bit = int(tile_bits[k * tpb + r // TILE]) + int(group_bits[k * gpb + r // TILE * 64:k * gpb + r // GROUP].sum())
    bo = int(enc.h_offs[k])
    tl = int.from_bytes(bytes(enc.stream[bo + 8:bo + 10].cpu().numpy()), "little")
    return bo + 10 + 2 * tl + bit // 8 + 1


def damaged(enc, at, xor):
    st = enc.stream.clone()
    st[at] ^= xor
    other = enc.with_stream(st)
    return other


def same_as_without_flag(torch, codec, bad, ranges, oo):
    ref = call(torch, codec, bad, ranges, oo, False)
    got = call(torch, codec, bad, ranges, oo, True)
    assert got[1:] == ref[1:], (got[1:], ref[1:])
    for i, (lo, hi) in enumerate(ranges):
        assert np.array_equal(got[0][oo[i]:oo[i] + got[2][i]], ref[0][oo[i]:oo[i] + ref[2][i]]), f"range {i}: delivered bytes"
        cut = min(hi, bad.n) - min(lo, bad.n)
        assert np.all(got[0][oo[i] + cut:oo[i + 1]] == GUARD)
    assert np.all(got[0][:oo[0]] == GUARD) and np.all(got[0][oo[-1]:] == GUARD)
    return got


@pytest.mark.parametrize("shape", ["bs65536", "oneblock"])
def test_payload_damage(torch_mod, codec, shape):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", shape)
    b = enc.bs or enc.n
    p = (2 * b if enc.bs else 0) + 5 * TILE             # a tile in the middle of a block
    ranges = [(p + 100, p + 400), (p + TILE + 7, p + TILE + 50), (7, 99)]
    oo = slots_for(ranges, enc.n)
    # inside a touched tile, in a group the range delivers: what the call without the flag gives
    for xor in (0x10, 0x01, 0x80):
        bad = damaged(enc, payload_byte_of(enc, p + 128), xor)
        same_as_without_flag(torch, codec, bad, ranges, oo)
    # in an earlier, untouched tile of the same block: not seen
    bad = damaged(enc, payload_byte_of(enc, p - 3 * TILE + 64), 0x10)
    got = call(torch, codec, bad, ranges[:2], oo[:3], True)
    check_all_good(enc, ranges[:2], got[0], got[1], got[2], oo[:3])
    assert codec.ranges_counters() == (0, 0, 1, 2, 0, 0, 0, 0)


def test_tree_damage(torch_mod, codec):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", "bs65536")
    p = 2 * 65536
    ranges = [(p + 5000, p + 5100), (p - 10, p + 10), (100, 200)]
    oo = slots_for(ranges, enc.n)
    bo = int(enc.h_offs[2])
    for at, xor in ((bo + 10 + 2 * 9, 0x55), (bo + 10 + 2 * 4 + 1, 0x80), (bo + 10 + 2 * 30, 0x01)):
        same_as_without_flag(torch, codec, damaged(enc, at, xor), ranges, oo)


def test_a_slot_one_byte_short(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs4096")
    ranges = [(10, 4096 + 10), (4096 + 20, 4096 + 700), (2 * 4096 + 1, 2 * 4096 + 700), (5 * 4096, 5 * 4096 + 1)]
    for short in (0, 1, 2):
        oo = slots_for(ranges, enc.n, shrink={short: 1})
        ref = call(torch_mod, codec, enc, ranges, oo, False)
        got, errs, raws = call(torch_mod, codec, enc, ranges, oo, True)
        cnt = codec.ranges_counters()
        assert (errs[short], raws[short]) == (HUFE_MEMORY, 0) and (errs, raws) == ref[1:]
        assert np.all(got[oo[short]:oo[short + 1]] == GUARD), "the short slot was written"
        check_all_good(enc, ranges, got, errs, raws, oo, only=[i for i in range(len(ranges)) if i != short])
        assert cnt == model(enc, ranges, oo) + (0, 0, 0, 0)


# ---- further cases -----------------------------------------------------------------------------------------------------
def test_batch_stream(torch_mod, codec):
    """a batch's stream with its sub-index, laid out as (nblocks x row_blocksize, row_blocksize): the items' short last
    blocks do not have the layout's length and stay on the old route"""
    torch = torch_mod
    bs = 4096
    lens = [5000, 0, 70000, 3, 65536 + 17, 12345, 4096]
    items = [datagen.zipf255(x, seed=50 + i) if x else np.zeros(0, np.uint8) for i, x in enumerate(lens)]
    data = np.concatenate(items)
    batch = codec.encode_batch(dev(torch, data), lens, bs, sub_index=True)
    block_lens = [min(bs, x - o) for x in lens for o in range(0, x, bs)]
    enc = Enc(torch, codec, data, bs, stream=batch.stream, offsets=batch.offsets, block_lens=block_lens)
    enc.sub, enc.raw_size, enc.row_bs = batch.sub_index, batch.nblocks * batch.row_blocksize, batch.row_blocksize
    enc.block_lens = np.asarray(block_lens)
    enc.elig = enc.block_lens == batch.row_blocksize
    ranges = [(4990, 5010), (4096, 5000), (100, 300), (5000 + 4096 + 9, 5000 + 3 * 4096 - 9), (enc.n - 1, enc.n + 9),
              (5000 + 70000 + 1, 5000 + 70000 + 3), (5000 + 2 * 4096 + 2047, 5000 + 2 * 4096 + 2049)]
    cnt = three_ways(torch, codec, enc, ranges)
    assert cnt[1] > 0 and cnt[2] > 0


def test_built_sub_index(torch_mod, codec):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", "bs65536")
    built, unbuilt = codec.build_sub_index(enc.stream, enc.length, enc.offsets, enc.n, enc.bs)
    assert unbuilt == 0
    ranges = edge_ranges(enc.bs, enc.n)
    oo = slots_for(ranges, enc.n)
    got = call(torch, codec, enc, ranges, oo, True, sub_index=built)
    check_all_good(enc, ranges, got[0], got[1], got[2], oo)
    assert codec.ranges_counters() == model(enc, ranges, oo) + (0, 0, 0, 0)


def test_interleaved_with_decode(torch_mod, codec):
    torch = torch_mod
    a = encoded(torch, codec, "zipf255", "bs4096")
    b = encoded(torch, codec, "l2", "bs65536")
    ra, rb = edge_ranges(a.bs, a.n), edge_ranges(b.bs, b.n)
    three_ways(torch, codec, a, ra)
    out = torch.full((b.n + 3,), GUARD, dtype=torch.uint8, device="cuda")
    assert codec.decode(b.stream, b.length, b.offsets, b.nb, out, sub_index=b.sub, raw_size=b.n, blocksize=b.bs) == b.n
    assert np.array_equal(out.cpu().numpy()[:b.n], b.data) and np.all(out.cpu().numpy()[b.n:] == GUARD)
    three_ways(torch, codec, b, rb)
    assert codec.decode(a.stream, a.length, a.offsets, a.nb, out[:a.n]) == a.n      # every block again: nothing stays switched off
    assert np.array_equal(out.cpu().numpy()[:a.n], a.data)
    three_ways(torch, codec, a, ra[:6])


def test_flag_without_sub_index(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs65536")
    ranges = edge_ranges(enc.bs, enc.n)
    oo = slots_for(ranges, enc.n)
    ref = call(torch_mod, codec, enc, ranges, oo, False, sub_index=None)
    c0 = codec.ranges_counters()
    got = call(torch_mod, codec, enc, ranges, oo, True, sub_index=None)
    assert got[1:] == ref[1:] and np.array_equal(got[0], ref[0])
    assert codec.ranges_counters() == c0 and c0[2:] == (0, 0, 0, 0, 0, 0)
    one = codec.decode_range(enc.stream, enc.length, enc.offsets, enc.nb, 70000, 70100, tiles=True, **enc.sub_args())
    assert np.array_equal(one.cpu().numpy(), enc.data[70000:70100]) and codec.ranges_counters()[2:4] == (1, 1)

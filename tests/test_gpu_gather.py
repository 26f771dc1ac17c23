"""GPU tests of hufgpu_gather (GpuCodec.gather): records of the original data whose positions, lengths, slots and
statuses live on the device, served by sub-index tile, grouped by block on the device, enqueue-only.

Bit-exact, no tolerance.  A record with status 0 holds a slice of the input and what decode_ranges(..., tiles=True)
delivers for the same range; a record with another status is "not served here" and decode_ranges without the flag has
the last word.  Every output buffer is filled with 0xA5 first: around every slot, and over the whole stride behind a
record's (cut) length, it must still be there.  Positions are made by a torch op on the device right before the call.
"""
import numpy as np
import pytest

from libhuffman_amd import datagen
from test_gpu_ranges import GUARD, Enc, dev, slots_for
from test_gpu_range_tiles import make

pytestmark = pytest.mark.gpu

TILE, GROUP = 2048, 32
OK, ARGUMENT, RW = 0, 2, 3
BIG = 3 * (1 << 20) + 77
SHAPES = {"bs4096": (4096, 9 * 4096 + 1500), "bs65536": (65536, 5 * 65536 + 1000), "oneblock": (0, BIG)}
CASES = [("zipf255", "bs4096"), ("zipf255", "bs65536"), ("zipf255", "oneblock"), ("two", "bs4096"), ("long", "bs65536"),
         ("const41", "bs4096"), ("const41", "bs65536"), ("mix", "bs4096")]
SIZES = (1, 31, 32, 33, 64, 2048, 2049)


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


_cache = {}


def encoded(torch, codec, kind, shape):
    """one encode per (input, shape) for the whole module; the tests never change it"""
    if (kind, shape) not in _cache:
        bs, n = SHAPES[shape]
        if kind == "mix":                               # one-symbol and ordinary blocks alternate
            data = datagen.zipf255(n, seed=4).copy()
            for b in range(0, n, 2 * bs):
                data[b:b + bs] = 41
        else:
            data = make(kind, n, bs)
        enc = Enc(torch, codec, data, bs, sub=True)
        enc.raw_size, enc.row_bs = enc.n, enc.bs
        _cache[kind, shape] = enc
    return _cache[kind, shape]


def gather(torch, codec, enc, pos, lens, max_len=None, spare=5, lead=3, sub=None, raw_size=None, blocksize=None):
    """records at `pos` (a list), `lens` an int or a list (then on the device, with max_len): rows of max_len + spare
    bytes from byte `lead` of a guarded buffer.  Returns (buffer, errs, raw_lens, row stride) on the host."""
    n = len(pos)
    fixed = isinstance(lens, int)
    max_len = lens if fixed else max_len
    stride = max_len + spare
    buf = torch.full((lead + n * stride + 9,), GUARD, dtype=torch.uint8, device="cuda")
    out = buf[lead:lead + n * stride].view(n, stride)
    positions = torch.tensor(pos, dtype=torch.int64).cuda() - 7 + 7        # (an op on the device)
    lengths = lens if fixed else torch.tensor(lens, dtype=torch.int32).cuda()
    _, errs, raws = codec.gather(enc.stream, enc.length, enc.offsets, enc.nb, positions, lengths,
                                 sub_index=enc.sub if sub is None else sub, raw_size=enc.raw_size if raw_size is None else raw_size,
                                 blocksize=enc.row_bs if blocksize is None else blocksize, max_len=None if fixed else max_len, out=out)
    return buf.cpu().numpy(), errs.cpu().numpy(), raws.cpu().numpy(), stride


def cut(enc, p, ln, n=None):
    n = enc.n if n is None else n
    return min(ln, n - p) if p < n else 0


def check_guards(enc, got, pos, lens, stride, lead=3, n=None):
    """nothing outside the first (cut length) bytes of the slots is written"""
    g = got.copy()
    for i, p in enumerate(pos):
        ln = lens if isinstance(lens, int) else lens[i]
        g[lead + i * stride:lead + i * stride + cut(enc, p, ln, n)] = GUARD
    bad = np.flatnonzero(g != GUARD)
    assert bad.size == 0, f"bytes outside the cut slots written at {bad[:8]}"


def check_good(enc, got, errs, raws, pos, lens, stride, lead=3, only=None):
    want = np.full(got.size, GUARD, np.uint8)
    for i, p in enumerate(pos):
        ln = lens if isinstance(lens, int) else lens[i]
        c = cut(enc, p, ln)
        if only is not None and i not in only:
            want[lead + i * stride:lead + i * stride + c] = got[lead + i * stride:lead + i * stride + c]
            continue
        assert (errs[i], raws[i]) == (OK, c), f"record {i} at {p} + {ln}: ({errs[i]}, {raws[i]})"
        want[lead + i * stride:lead + i * stride + c] = enc.data[p:p + c]
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, f"bytes differ at {diff[:8]} (stride {stride})"


def by_ranges(torch, codec, enc, pos, lens, tiles, sub="own"):
    """the same records through decode_ranges: (bytes per record, errs, raws)"""
    ranges = [(p, p + (lens if isinstance(lens, int) else lens[i])) for i, p in enumerate(pos)]
    oo = slots_for(ranges, enc.n)
    out = torch.full((oo[-1] + 9,), GUARD, dtype=torch.uint8, device="cuda")
    kw = dict(sub_index=enc.sub, raw_size=enc.raw_size, blocksize=enc.row_bs) if sub == "own" else {}
    _, errs, raws = codec.decode_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges, out=out, out_offsets=oo, tiles=tiles, **kw)
    h = out.cpu().numpy()
    return [h[oo[i]:oo[i] + raws[i]] for i in range(len(ranges))], errs, raws


def same_as_ranges(torch, codec, enc, got, errs, raws, pos, lens, stride, lead=3):
    ref, rerrs, rraws = by_ranges(torch, codec, enc, pos, lens, True)
    assert list(errs) == rerrs and list(raws) == rraws
    for i in range(len(pos)):
        assert np.array_equal(got[lead + i * stride:lead + i * stride + rraws[i]], ref[i]), f"record {i}: differs from decode_ranges"


def positions_for(enc, ln, seed):
    b = enc.bs or enc.n
    n = enc.n
    t = b + 3 * TILE if n > b + 4 * TILE else TILE
    rng = np.random.default_rng(seed)
    pos = [int(x) for x in rng.integers(0, n, 400)]
    pos += [t + 3, t + GROUP - 1, t + GROUP - ln // 2, t + TILE - 1, t + TILE - ln // 2 - 1,    # inside a group, across groups and tiles
            0, max(0, n - ln), n, n + 5, n - 1, max(0, n - ln // 2 - 1),                         # at 0, ending at / past / cut by raw_size
            t + 100, t + 100, t + 100]                                                           # repeated
    if enc.bs:
        pos += [b - 1, b - ln // 2 - 1, 3 * b - 1, 3 * b, (n - 1) // b * b - 1]                  # across block borders, the short last block
    return pos


# ---- equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_fixed_sizes(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    for k, ln in enumerate(SIZES):
        pos = positions_for(enc, ln, 20 + k)
        got, errs, raws, stride = gather(torch_mod, codec, enc, pos, ln, spare=(5, 0, 7, 1, 16, 3, 2)[k], lead=(3, 0, 1, 16, 7, 5, 9)[k])
        lead = (3, 0, 1, 16, 7, 5, 9)[k]
        check_good(enc, got, errs, raws, pos, ln, stride, lead)
        if ln in (33, 2049):
            same_as_ranges(torch_mod, codec, enc, got, errs, raws, pos, ln, stride, lead)


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_lengths_from_the_device(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    pos = positions_for(enc, 300, 31)
    rng = np.random.default_rng(32)
    lens = [int(x) for x in rng.integers(0, 2501, len(pos))]
    lens[:4] = [2500, 0, 1, 2049]
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, lens, max_len=2500)
    check_good(enc, got, errs, raws, pos, lens, stride)
    same_as_ranges(torch_mod, codec, enc, got, errs, raws, pos, lens, stride)


def test_all_inside_one_block(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs65536")
    rng = np.random.default_rng(33)
    pos = [int(x) for x in rng.integers(2 * 65536, 3 * 65536 - 64, 400)]
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, 64)
    check_good(enc, got, errs, raws, pos, 64, stride)


def test_a_record_over_three_blocks(torch_mod, codec):
    for kind in ("zipf255", "mix"):
        enc = encoded(torch_mod, codec, kind, "bs4096")
        pos = [4096 - 50, 2 * 4096 + 1, 5 * 4096 - 4100, 0, enc.n - 8200]
        got, errs, raws, stride = gather(torch_mod, codec, enc, pos, 8200, spare=3, lead=1)
        check_good(enc, got, errs, raws, pos, 8200, stride, 1)
        same_as_ranges(torch_mod, codec, enc, got, errs, raws, pos, 8200, stride, 1)


def test_long_records_in_a_giant_block(torch_mod, codec):
    """hundreds of tiles of one record: the block's items are the work of several workgroups"""
    enc = encoded(torch_mod, codec, "zipf255", "oneblock")
    pos = [TILE * 3 + 5, 77, enc.n - 100000]
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, 700001, spare=2, lead=7)
    check_good(enc, got, errs, raws, pos, 700001, stride, 7)


# ---- statuses ----------------------------------------------------------------------------------------------------------
def test_a_length_above_max_len(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs4096")
    pos = [10, 5000, 9000, 4090, 20000]
    lens = [100, 101, 100, 4000000, 7]
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, lens, max_len=100)
    assert list(errs) == [OK, ARGUMENT, OK, ARGUMENT, OK] and list(raws) == [100, 0, 100, 0, 7]
    for i in (1, 3):
        assert np.all(got[3 + i * stride:3 + (i + 1) * stride] == GUARD)
    check_good(enc, got, errs, raws, pos, lens, stride, only=(0, 2, 4))


def served_again(torch, codec, enc, got, errs, pos, ln, stride, lead=3):
    """records with a non-zero status, by decode_ranges without the flag: the input's bytes"""
    idx = [i for i in range(len(pos)) if errs[i] != OK]
    if not idx:
        return
    ref, rerrs, rraws = by_ranges(torch, codec, enc, [pos[i] for i in idx], ln, False, sub=None)
    for k, i in enumerate(idx):
        c = cut(enc, pos[i], ln)
        assert (rerrs[k], rraws[k]) == (OK, c) and np.array_equal(ref[k], enc.data[pos[i]:pos[i] + c])


@pytest.mark.parametrize("shape", ["bs4096", "bs65536", "oneblock"])
def test_foreign_sub_index(torch_mod, codec, shape):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", shape)
    rng = np.random.default_rng(13)
    ln = 300
    pos = positions_for(enc, ln, 41)[300:]
    # a bit count of 0 or of 65 535 cannot be that of 32 codewords: every tile fails its checks
    for name, sub in (("zeros", torch.zeros_like(enc.sub)), ("ones", torch.full_like(enc.sub, -1))):
        got, errs, raws, stride = gather(torch, codec, enc, pos, ln, sub=sub)
        check_guards(enc, got, pos, ln, stride)
        for i, p in enumerate(pos):
            assert raws[i] == cut(enc, p, ln) and errs[i] == (RW if raws[i] else OK), (name, i, errs[i])
        served_again(torch, codec, enc, got, errs, pos, ln, stride)
    # contents that may pass by chance: no byte outside the cut slots; status 0 or "ask again"
    other = Enc(torch, codec, make("two", enc.n, enc.bs), enc.bs, sub=True)
    for name, sub in (("random", torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()), ("stale", other.sub)):
        got, errs, raws, stride = gather(torch, codec, enc, pos, ln, sub=sub)
        check_guards(enc, got, pos, ln, stride)
        assert set(errs.tolist()) <= {OK, RW} and all(raws[i] == cut(enc, p, ln) for i, p in enumerate(pos)), name
        served_again(torch, codec, enc, got, errs, pos, ln, stride)


def payload_byte_of(codec, enc, pos):
    """the stream byte behind the one that holds the first payload bit of the group of raw position `pos`"""
    nbytes = codec.sub_index_bytes(enc.n, enc.bs)
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
    return enc.with_stream(st)


def as_the_call_without_the_flag(torch, codec, bad, got, errs, raws, pos, ln, stride, hit):
    """TILES points 1-3 on a damaged stream: records off the damage are served with the input's bytes; a record on it is
    either not served, or served with what decode_ranges without the flag delivers with success"""
    check_guards(bad, got, pos, ln, stride)
    ref, rerrs, rraws = by_ranges(torch, codec, bad, pos, ln, False)
    for i, p in enumerate(pos):
        c = cut(bad, p, ln)
        mine = got[3 + i * stride:3 + i * stride + c]
        assert raws[i] == c
        if i in hit:
            assert errs[i] == RW or (errs[i] == OK and rerrs[i] == OK and np.array_equal(mine, ref[i])), (i, errs[i], rerrs[i])
        else:
            assert errs[i] == OK and np.array_equal(mine, bad.data[p:p + c]), (i, errs[i])
    return [errs[i] for i in hit]


@pytest.mark.parametrize("shape", ["bs65536", "oneblock"])
def test_payload_damage(torch_mod, codec, shape):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", shape)
    b = enc.bs or enc.n
    p = (2 * b if enc.bs else 0) + 5 * TILE             # a tile in the middle of a block
    ln = 300
    pos = [p + 100, p + TILE + 7, 7, p + 100, p + 1500]
    seen = []
    # inside a touched tile: records 0 and 3 deliver the damaged group, record 4 lies in the same tile
    for xor in (0x10, 0x01, 0x80):
        bad = damaged(enc, payload_byte_of(codec, enc, p + 128), xor)
        got, errs, raws, stride = gather(torch, codec, bad, pos, ln)
        seen += as_the_call_without_the_flag(torch, codec, bad, got, errs, raws, pos, ln, stride, hit=(0, 3, 4))
    assert RW in seen, "no damage was noticed"
    # in an earlier, untouched tile of the same block: not seen
    bad = damaged(enc, payload_byte_of(codec, enc, p - 3 * TILE + 64), 0x10)
    got, errs, raws, stride = gather(torch, codec, bad, pos, ln)
    check_good(enc, got, errs, raws, pos, ln, stride)


def test_tree_and_header_damage(torch_mod, codec):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", "bs65536")
    p = 2 * 65536
    ln = 100
    pos = [p + 5000, p - 10, 100, 3 * 65536 - 50, 4 * 65536]
    bo = int(enc.h_offs[2])
    seen = []
    for at, xor in ((bo + 10 + 2 * 9, 0x55), (bo + 10 + 2 * 4 + 1, 0x80), (bo + 10 + 2 * 30, 0x01)):
        bad = damaged(enc, at, xor)
        got, errs, raws, stride = gather(torch, codec, bad, pos, ln)
        seen += as_the_call_without_the_flag(torch, codec, bad, got, errs, raws, pos, ln, stride, hit=(0, 1, 3))
    assert RW in seen
    # a header whose block_len is not the layout's, a tree_len that reaches past the block's record: not served
    for at, xor in ((bo, 0x01), (bo + 9, 0x40)):
        bad = damaged(enc, at, xor)
        got, errs, raws, stride = gather(torch, codec, bad, pos, ln)
        check_guards(enc, got, pos, ln, stride)
        assert list(errs) == [RW, RW, OK, RW, OK] and list(raws) == [ln] * 5
        check_good(enc, got, errs, raws, pos, ln, stride, only=(2, 4))


def test_one_symbol_payload_damage(torch_mod, codec):
    enc = encoded(torch_mod, codec, "const41", "bs4096")
    bo = int(enc.h_offs[1])
    bad = damaged(enc, bo + 20 + 100 // 8, 0x80 >> (100 % 8))      # the bit of symbol 100 of block 1
    pos = [4096 + 90, 4096 + 101, 4096 - 5, 4096 + 100, 10]
    got, errs, raws, stride = gather(torch_mod, codec, bad, pos, 11)
    check_guards(enc, got, pos, 11, stride)
    assert list(errs) == [RW, OK, OK, RW, OK]
    check_good(enc, got, errs, raws, pos, 11, stride, only=(1, 2, 4))


def test_a_short_block_in_the_middle(torch_mod, codec):
    """a batch's stream with batch geometry (nblocks x row_blocksize, row_blocksize): block b's bytes are addressed from
    b * row_blocksize; the items' short last blocks do not have the layout's length and are not served"""
    torch = torch_mod
    bs = 4096
    lens = [5000, 0, 70000, 3, 12345, 4096]
    data = np.concatenate([datagen.zipf255(x, seed=50 + i) if x else np.zeros(0, np.uint8) for i, x in enumerate(lens)])
    batch = codec.encode_batch(dev(torch, data), lens, bs, sub_index=True)
    block_lens = [min(bs, x - o) for x in lens for o in range(0, x, bs)]
    enc = Enc(torch, codec, data, bs, stream=batch.stream, offsets=batch.offsets, block_lens=block_lens)
    enc.sub, enc.raw_size, enc.row_bs = batch.sub_index, batch.nblocks * batch.row_blocksize, batch.row_blocksize
    assert enc.nb == batch.nblocks and batch.row_blocksize == bs
    full = [b for b in range(enc.nb) if block_lens[b] == bs]
    short = [b for b in range(enc.nb) if block_lens[b] != bs]
    assert short and min(short) < max(full)
    ln = 200
    recs = [(b, o) for b in full for o in (0, 1000, 2047, bs - ln)] + [(b, 0) for b in short] + [(full[3], bs - 50)]
    pos = [b * bs + o for b, o in recs]
    got, errs, raws, stride = gather(torch, codec, enc, pos, ln)
    check_guards(enc, got, pos, ln, stride, n=enc.raw_size)
    true_pos = []
    for i, (b, o) in enumerate(recs):
        if b in short or (o + ln > bs and b + 1 in short):
            assert errs[i] == RW, (i, b, o)
            continue
        assert errs[i] == OK and raws[i] == ln
        # (full blocks that follow one another hold bytes that follow one another)
        assert np.array_equal(got[3 + i * stride:3 + i * stride + ln], data[int(enc.P[b]) + o:int(enc.P[b]) + o + ln]), (i, b, o)
        true_pos.append((i, int(enc.P[b]) + o))
    ref, rerrs, _ = by_ranges(torch, codec, enc, [p for _, p in true_pos], ln, True)
    for k, (i, _) in enumerate(true_pos):
        assert rerrs[k] == OK and np.array_equal(got[3 + i * stride:3 + i * stride + ln], ref[k])


def test_a_wrong_layout_that_gives_nblocks(torch_mod, codec):
    """a data error, not a fault: blocks whose header length is not the claimed layout's are not served"""
    enc = encoded(torch_mod, codec, "zipf255", "bs4096")
    assert enc.nb == 10
    ln = 64
    pos = [0, 5000, 9 * 4096 - 10, 9 * 4096 + 10, 9 * 4096 + 790, 9 * 4096 + 900, 38000]
    # raw_size 700 short: the last block is not the layout's, records are cut at the claimed end
    n2 = enc.n - 700
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, ln, raw_size=n2)
    check_guards(enc, got, pos, ln, stride, n=n2)
    assert list(raws) == [cut(enc, p, ln, n2) for p in pos]
    assert list(errs) == [OK, OK, RW, RW, RW, OK, OK]
    check_good(enc, got, errs, raws, pos, ln, stride, only=(0, 1))
    # another blocksize with the same block count: no block is the layout's
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, ln, raw_size=38000, blocksize=4000)
    check_guards(enc, got, pos, ln, stride, n=38000)
    assert all(e == (RW if r else OK) for e, r in zip(errs, raws)) and list(raws) == [cut(enc, p, ln, 38000) for p in pos]


# ---- other behaviour ---------------------------------------------------------------------------------------------------
def test_built_sub_index(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs65536")
    built, unbuilt = codec.build_sub_index(enc.stream, enc.length, enc.offsets, enc.n, enc.bs)
    assert unbuilt == 0
    pos = positions_for(enc, 300, 51)
    got, errs, raws, stride = gather(torch_mod, codec, enc, pos, 300, sub=built)
    check_good(enc, got, errs, raws, pos, 300, stride)


def test_two_gathers_back_to_back(torch_mod, codec):
    """no synchronise between the two calls, one behind them: buffers and positions are made first"""
    torch = torch_mod
    jobs = []
    for kind, shape, ln, seed in (("zipf255", "bs4096", 64, 61), ("long", "bs65536", 2049, 62)):
        enc = encoded(torch, codec, kind, shape)
        pos = positions_for(enc, ln, seed)[350:]
        stride = ln + 5
        buf = torch.full((3 + len(pos) * stride + 9,), GUARD, dtype=torch.uint8, device="cuda")
        jobs.append((enc, pos, ln, stride, buf, torch.tensor(pos, dtype=torch.int64).cuda()))
    torch.cuda.synchronize()
    res = []
    for enc, pos, ln, stride, buf, base in jobs:
        out = buf[3:3 + len(pos) * stride].view(len(pos), stride)
        res.append(codec.gather(enc.stream, enc.length, enc.offsets, enc.nb, base + 0, ln, sub_index=enc.sub, raw_size=enc.n,
                                blocksize=enc.bs, out=out))
    torch.cuda.synchronize()
    for (enc, pos, ln, stride, buf, _), (_, errs, raws) in zip(jobs, res):
        check_good(enc, buf.cpu().numpy(), errs.cpu().numpy(), raws.cpu().numpy(), pos, ln, stride)


def test_between_two_decodes(torch_mod, codec):
    torch = torch_mod
    a = encoded(torch, codec, "zipf255", "bs4096")
    b = encoded(torch, codec, "zipf255", "bs65536")
    out = torch.full((b.n + 3,), GUARD, dtype=torch.uint8, device="cuda")
    assert codec.decode(b.stream, b.length, b.offsets, b.nb, out, sub_index=b.sub, raw_size=b.n, blocksize=b.bs) == b.n
    pos = positions_for(a, 33, 71)
    got, errs, raws, stride = gather(torch, codec, a, pos, 33)
    check_good(a, got, errs, raws, pos, 33, stride)
    h = out.cpu().numpy()
    assert np.array_equal(h[:b.n], b.data) and np.all(h[b.n:] == GUARD)
    assert codec.decode(a.stream, a.length, a.offsets, a.nb, out[:a.n]) == a.n
    assert np.array_equal(out.cpu().numpy()[:a.n], a.data)


def test_no_records(torch_mod, codec):
    enc = encoded(torch_mod, codec, "zipf255", "bs4096")
    out, errs, raws = codec.gather(enc.stream, enc.length, enc.offsets, enc.nb, torch_mod.zeros(0, dtype=torch_mod.int64, device="cuda"),
                                   64, sub_index=enc.sub, raw_size=enc.n, blocksize=enc.bs)
    assert tuple(out.shape) == (0, 64) and errs.numel() == 0 and raws.numel() == 0

"""GPU tests of hufgpu_scatter (GpuCodec.scatter / scatter_result / redact): records at device-resident positions
overwritten in one indexed stream, out of place, enqueue-only.

Bit-exact, no tolerance.  The expected stream, block index and sub-index are the oracle's encode of D' - the data with the
records applied by tests/scatter_model.py - the way tests/test_gpu_update.py gets its expectation.  Every output - the
stream, the index, the sub-index, the four result words - lies between guard words that must still hold their fill after
every call, and the old stream is compared with a copy taken before the call.  The damaged streams are the kind the update
tests feed: a flipped payload bit, a tree_len no tree has.
"""
import ctypes as C
import gc
import re

import numpy as np
import pytest

import scatter_model as model
import sub_index_ref as sref
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 80
IDX_GUARD = -0x5A5A5A5A5A5A5A5B
SUB_GUARD = 0x7B7B7B7B7B7B7B7B
RES_GUARD = 0x3C3C3C3C3C3C3C3C
HUFE_OK, HUFE_MEMORY, HUFE_ARGUMENT, HUFE_RW = 0, 1, 2, 3
FILL_FLAG = 0x100
NONE64 = 0xFFFFFFFFFFFFFFFF
KIB = 1 << 10
SIZES = {"4K": 4 * KIB, "64K": 64 * KIB, "256K": 256 * KIB}    # the fused counts; the lane-private counters; pack's long codes (> 121 392)


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def make(kind, n, seed=0):
    return datagen.zipf255(n, seed=3 + seed) if kind == "zipf255" else datagen.logtext(n, seed=5 + seed)


class Enc:
    """an encoded input with its sub-index, on the device"""

    def __init__(self, torch, codec, data, bs):
        self.data, self.bs, self.n = data, bs, int(data.size)
        self.sub = codec.new_sub_index(self.n, bs)
        self.stream, self.offsets, _ = codec.encode(dev(torch, data), bs, sub_index=self.sub)
        self.nb = codec.block_count(self.n, bs)
        self.length = int(self.stream.numel())
        self.h_offs = self.offsets.cpu().numpy().astype(np.int64)

    def variant(self, **kw):
        other = object.__new__(Enc)
        other.__dict__.update(self.__dict__)
        other.__dict__.update(kw)
        return other


_ENCS = {}


def enc_of(torch, codec, kind, bs, n):
    """one encode per input, shared among the tests and never written"""
    key = (kind, bs, n)
    if key not in _ENCS:
        _ENCS[key] = Enc(torch, codec, make(kind, n), bs)
    return _ENCS[key]


class Result:
    pass


def slots_of(target, pos, lens, max_len, n, width=None):
    """record i's new bytes = target[pos_i : pos_i + len_i]: records that overlap agree.  Bytes of a slot behind len_i are 0xEE."""
    width = width or max(1, max_len)
    s = np.full((len(pos), width), 0xEE, np.uint8)
    for i, p in enumerate(pos):
        p, k = model.cut(p, max_len if lens is None else lens[i], n)
        s[i, :k] = target[p:p + k]
    return s


def scatter(torch, codec, enc, pos, lens, max_len, fill=None, slots=None, src_off=1, cap=None, old_sub=None, want_sub=False,
            out_cap=None, relaxed=False, out_off=1, stream=None, d_pos=None, d_len=None, d_src=None, stride=None, outs=None):
    """One call through the C ABI with guarded buffers, then a wait and a look at the guards.  The slots lie src_off bytes
    behind an aligned address; d_out 4 out_off bytes behind one.  d_pos / d_len / d_src: device buffers of the caller's in
    the place of pos / lens / slots.  outs: the buffers of an earlier call, to be used again."""
    lib = codec.lib
    nrec = len(pos) if d_pos is None else int(d_pos.numel())
    if d_pos is None:
        d_pos = torch.from_numpy(np.asarray(pos, np.uint64).astype(np.int64)).cuda() if nrec else torch.zeros(1, dtype=torch.int64, device="cuda")
    if d_len is None and lens is not None:
        d_len = torch.from_numpy(np.asarray(lens, np.uint32).view(np.int32) if nrec else np.zeros(1, np.int32)).cuda()
    if fill is None and d_src is None:
        stride = slots.shape[1] if nrec else max(1, max_len)
        flat = np.concatenate([np.full(src_off, 0xEE, np.uint8), slots.reshape(-1), np.full(9, 0xEE, np.uint8)])
        d_src = dev(torch, flat)[src_off:]
    bs_eff = enc.bs or enc.n
    if cap is None:
        cap = max(1, min(enc.nb, model.touched_bound(enc.nb, enc.bs, nrec, max_len)))
    if outs is None:
        room = enc.length + cap * codec.encode_bound(min(bs_eff, enc.n), 0) + 64 if out_cap is None else out_cap
        out_off *= 4
        o = Result()
        o.room, o.lead = room, GUARD_BYTES + out_off
        o.big = torch.full((room + 2 * GUARD_BYTES + out_off + 3,), GUARD, dtype=torch.uint8, device="cuda")
        o.out = o.big[o.lead:o.lead + room]
        o.idx_big = torch.full((enc.nb + 1 + 4,), IDX_GUARD, dtype=torch.int64, device="cuda")
        o.idx = o.idx_big[2:2 + enc.nb + 1]
        o.sub_big = o.sub = None
        if want_sub:
            words = -(-codec.sub_index_bytes(enc.n, enc.bs) // 8)
            o.sub_big = torch.full((words + 4,), SUB_GUARD, dtype=torch.int64, device="cuda")
            o.sub = o.sub_big[2:2 + words]
        o.res_big = torch.full((8,), RES_GUARD, dtype=torch.int64, device="cuda")
        o.res = o.res_big[2:6]
        outs = o
    o = outs
    before = enc.stream.clone() if stream is None else None
    flags = (1 if relaxed else 0) | (FILL_FLAG if fill is not None else 0)
    rc = lib.hufgpu_scatter(codec._ctx, enc.stream.data_ptr(), enc.length, enc.offsets.data_ptr(), enc.nb,
                            old_sub.data_ptr() if old_sub is not None else None, enc.n, enc.bs, nrec, d_pos.data_ptr(),
                            d_len.data_ptr() if d_len is not None else None, max_len,
                            d_src.data_ptr() if d_src is not None else None, stride or 0, fill or 0, cap,
                            o.out.data_ptr(), o.room, o.idx.data_ptr(), o.sub.data_ptr() if o.sub is not None else None,
                            o.res.data_ptr(), flags, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    r = Result()
    r.rc, r.outs, r.cap = int(rc), o, cap
    if stream is not None:
        return r                                         # (the caller waits, then calls fetch)
    torch.cuda.synchronize()
    assert torch.equal(before, enc.stream), "the old stream was written"
    return fetch(r, enc)


def fetch(r, enc):
    o = r.outs
    hb = o.big.cpu().numpy()
    assert np.all(hb[:o.lead] == GUARD) and np.all(hb[o.lead + o.room:] == GUARD), "guard bytes around d_out"
    hi = o.idx_big.cpu().numpy()
    assert np.all(hi[:2] == IDX_GUARD) and np.all(hi[2 + enc.nb + 1:] == IDX_GUARD), "guard words around the index"
    if o.sub_big is not None:
        hs = o.sub_big.cpu().numpy()
        assert np.all(hs[:2] == SUB_GUARD) and np.all(hs[-2:] == SUB_GUARD), "guard words around the sub-index"
    hr = o.res_big.cpu().numpy()
    assert np.all(hr[:2] == RES_GUARD) and np.all(hr[6:] == RES_GUARD), "guard words around d_result"
    r.status, r.length, r.touched, r.who = (int(x) for x in hr[2:6].view(np.uint64))
    r.out_all = hb[o.lead:o.lead + o.room]
    r.stream = r.out_all[:r.length]
    r.index = hi[2:2 + enc.nb + 1].astype(np.uint64)
    r.d_stream, r.d_index, r.sub = o.out[:r.length], o.idx, o.sub
    if r.status != HUFE_OK:
        assert r.length == 0, "with a non-zero status the length is 0"
    return r


def check_sub(r, exp, hit=None):
    """the new sub-index on the entries the encoder writes; hit: the touched blocks when no old sub-index was given"""
    e = exp.sub()
    if hit is not None:
        mask = np.zeros(e.lay.nb, bool)
        mask[list(hit)] = True
        for w, per in ((e.w_tiles, e.lay.tpb), (e.w_groups, e.lay.gpb), (e.w_lens, 256)):
            w &= np.repeat(mask, per)
    got = r.sub.cpu().numpy().view(np.uint8)
    assert sref.mismatches(got, e) == [], "(block, array, index, found, expected)"
    held = np.full(got.size // 8, SUB_GUARD, dtype=np.int64).view(np.uint8)
    assert sref.unwritten_changed(got, held, e) == [], "(block, array, index, found, held)"


def check_model(oracle, enc, r, pos, lens, max_len, fill=None, slots=None, what="", sub=None):
    """stream and index equal the oracle's encode of the model's D'; the touched count is the model's.  sub: None - no look
    at the sub-index -, "whole" - an old one was given - or "touched"."""
    assert (r.rc, r.status) == (HUFE_OK, HUFE_OK), (what, r.rc, r.status, r.who)
    new = model.apply(enc.data, pos, lens, max_len, fill=fill, slots=slots)
    exp = model.Expected(oracle, new, enc.bs)
    hit = model.touched_blocks(enc.n, enc.bs, pos, lens, max_len)
    assert r.touched == len(hit) and r.who == NONE64, (what, r.touched, len(hit))
    assert r.length == exp.length, (what, r.length, exp.length)
    bad = np.flatnonzero(r.stream != exp.stream)
    assert bad.size == 0, (what, "stream differs from the oracle's at", bad[:8])
    assert np.array_equal(r.index, exp.offs), (what, "index")
    if sub is not None:
        check_sub(r, exp, hit if sub == "touched" else None)
    return new, exp


def shapes(n, bs):
    """name -> (positions, lengths or None, max_len)"""
    b = bs or n
    return {
        "one record inside a tile": ([b + 10], [90], 128),
        "across the tile seam and across a block seam": ([2048 - 7, b - 5, 3 * b + 2048 - 1], [20, 11, 2], 20),
        "three whole blocks": ([b], [3 * b], 3 * b),
        "byte 0 and the last byte": ([0, n - 9], [7, 9], 9),
        "cut at raw_size, starting at raw_size, behind it, empty": ([n - 4, n, n + 1000, 100, 2 * b + 1], [50, 5, 5, 0, 3], 64),
        "d_len = NULL": ([5, b - 1, 2 * b + 77, n - 3, b - 1], None, 33),
        "duplicated records": ([b + 500, 17, b + 500, b + 500, 17], [40, 3, 40, 40, 3], 40),
        "overlapping records": ([100, 110, 105, b - 20, b - 10, 2 * b - 1, 2 * b - 3], [30, 30, 2, 30, 30, 5, 9], 30),
        "every byte": ([0], [n], n),
    }


@pytest.mark.parametrize("bs", list(SIZES), ids=list(SIZES))
@pytest.mark.parametrize("kind", ["zipf255", "logtext"])
def test_output_equals_the_model(torch_mod, codec, oracle, kind, bs):
    torch = torch_mod
    bs = SIZES[bs]
    n = 5 * bs + 100
    enc = enc_of(torch, codec, kind, bs, n)
    target = np.random.default_rng(bs).integers(0x20, 0x7B, n, dtype=np.uint8)
    for k, (name, (pos, lens, max_len)) in enumerate(shapes(n, bs).items()):
        sub = (None, "whole", "touched")[k % 3]
        old = enc.sub if sub == "whole" else None
        r = scatter(torch, codec, enc, pos, lens, max_len, fill=0x2A, old_sub=old, want_sub=sub is not None, out_off=k % 4)
        check_model(oracle, enc, r, pos, lens, max_len, fill=0x2A, what=(kind, bs, name, "fill"), sub=sub)
        slots = slots_of(target, pos, lens, max_len, n, width=max_len + k % 3)
        r = scatter(torch, codec, enc, pos, lens, max_len, slots=slots, src_off=k % 5, old_sub=enc.sub if k % 2 else None,
                    want_sub=sub is not None, out_off=(k + 1) % 4)
        check_model(oracle, enc, r, pos, lens, max_len, slots=slots, what=(kind, bs, name, "source"),
                    sub=None if sub is None else ("whole" if k % 2 else "touched"))


def random_records(n, count, seed, longest):
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, n, count) | 1                             # odd positions
    lens = rng.integers(0, longest + 1, count)
    return [int(p) for p in pos], [int(x) for x in lens]


@pytest.mark.parametrize("case", ["4K", "64K", "300 blocks"])
def test_400_random_records_at_odd_positions(torch_mod, codec, oracle, case):
    """overlaps included: the slots are cut from one target, so records that overlap agree; 300 blocks cross SCAN_GROUP"""
    torch = torch_mod
    bs = 4 * KIB if case == "300 blocks" else SIZES[case]
    n = 300 * bs if case == "300 blocks" else 5 * bs + 100
    enc = enc_of(torch, codec, "zipf255", bs, n)
    target = np.random.default_rng(7).integers(0, 200, n, dtype=np.uint8)
    for seed, longest in ((1, 300), (2, 2 * bs + 5)):
        pos, lens = random_records(n, 400, seed, longest)
        r = scatter(torch, codec, enc, pos, lens, longest, fill=0, old_sub=enc.sub, want_sub=True, out_off=seed)
        check_model(oracle, enc, r, pos, lens, longest, fill=0, what=(case, seed, "fill"), sub="whole" if seed == 1 else None)
        slots = slots_of(target, pos, lens, longest, n)
        r = scatter(torch, codec, enc, pos, lens, longest, slots=slots, src_off=3, want_sub=True)
        check_model(oracle, enc, r, pos, lens, longest, slots=slots, what=(case, seed, "source"), sub="touched" if seed == 1 else None)


def test_10000_overlapping_5_byte_fill_records_in_one_block(torch_mod, codec, oracle):
    torch = torch_mod
    bs = 64 * KIB
    enc = enc_of(torch, codec, "logtext", bs, 5 * bs + 100)
    rng = np.random.default_rng(11)
    pos = [int(p) for p in 2 * bs + rng.integers(0, bs - 5, 10000)]
    pos[:3] = [2 * bs, 3 * bs - 5, 2 * bs + 1]
    r = scatter(torch, codec, enc, pos, None, 5, fill=0x58, old_sub=enc.sub, want_sub=True)
    check_model(oracle, enc, r, pos, None, 5, fill=0x58, what="10 000 records", sub="whole")
    assert r.touched == 1


@pytest.mark.parametrize("bs", ["4K", "64K"])
def test_a_block_becomes_one_byte_value_and_a_one_symbol_block_becomes_mixed(torch_mod, codec, oracle, bs):
    """record sizes change in both directions: block 1 shrinks to a five-entry tree, block 2 (all 0x41) grows"""
    torch = torch_mod
    bs = SIZES[bs]
    n = 5 * bs + 99
    data = make("zipf255", n)
    data[2 * bs:3 * bs] = 0x41
    enc = Enc(torch, codec, data, bs)
    pos, lens = [bs, 2 * bs + 5], [bs, 45]
    slots = np.full((2, bs), 0x07, np.uint8)
    slots[1, :45] = np.random.default_rng(1).integers(0, 256, 45, dtype=np.uint8)
    r = scatter(torch, codec, enc, pos, lens, bs, slots=slots, old_sub=enc.sub, want_sub=True)
    new, exp = check_model(oracle, enc, r, pos, lens, bs, slots=slots, what="one byte", sub="whole")
    assert int(exp.offs[2] - exp.offs[1]) == 10 + 2 * 5 + bs // 8 and r.touched == 2      # a five-entry tree, one bit a byte
    # a fill does the same, and a fill of a one-symbol block with its own byte changes nothing
    r = scatter(torch, codec, enc, [bs, 2 * bs + 100], [bs, 50], bs, fill=0x41, old_sub=enc.sub, want_sub=True)
    check_model(oracle, enc, r, [bs, 2 * bs + 100], [bs, 50], bs, fill=0x41, what="fill to one byte", sub="whole")


def test_blocksize_0_is_one_block(torch_mod, codec, oracle):
    torch = torch_mod
    n = 150 * KIB + 13
    data = make("logtext", n)
    enc = Enc(torch, codec, data, 0)
    assert enc.nb == 1
    pos, lens = random_records(n, 300, 3, 200)
    r = scatter(torch, codec, enc, pos, lens, 200, fill=0x2E, old_sub=enc.sub, want_sub=True)
    check_model(oracle, enc, r, pos, lens, 200, fill=0x2E, what="one block", sub="whole")
    target = np.random.default_rng(2).integers(0x30, 0x3A, n, dtype=np.uint8)
    slots = slots_of(target, pos, lens, 200, n)
    r = scatter(torch, codec, enc, pos, lens, 200, slots=slots)
    check_model(oracle, enc, r, pos, lens, 200, slots=slots, what="one block, source")


# ---- identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", ["4K", "64K"])
def test_records_that_do_not_overlap_give_what_update_ranges_gives(torch_mod, codec, bs):
    torch = torch_mod
    bs = SIZES[bs]
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "zipf255", bs, n)
    ranges = [(bs // 2 + 3, 2 * bs + 9), (3 * bs, 3 * bs + 40), (n - 5, n), (7, 8)]
    rng = np.random.default_rng(4)
    patches = [rng.integers(0, 100, hi - lo, dtype=np.uint8) for lo, hi in ranges]
    st, length, offs, sub, count = codec.update_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges,
                                                       dev(torch, np.concatenate(patches)), sub_index=enc.sub, raw_size=n,
                                                       blocksize=bs, want_sub_index=True)
    max_len = max(hi - lo for lo, hi in ranges)
    slots = np.zeros((len(ranges), max_len), np.uint8)
    for i, p in enumerate(patches):
        slots[i, :p.size] = p
    r = scatter(torch, codec, enc, [lo for lo, _ in ranges], [hi - lo for lo, hi in ranges], max_len, slots=slots,
                old_sub=enc.sub, want_sub=True)
    assert (r.rc, r.status, r.length, r.touched) == (HUFE_OK, HUFE_OK, length, count)
    assert np.array_equal(r.stream, st.cpu().numpy()) and np.array_equal(r.index.astype(np.int64), offs.cpu().numpy())
    # the two new sub-indexes agree on every entry the encoder writes (update_ranges' buffer is the witness here)
    new = enc.data.copy()
    for (lo, hi), p in zip(ranges, patches):
        new[lo:hi] = p
    exp = sref.expected(r.stream, r.index, new, bs)
    assert sref.mismatches(r.sub.cpu().numpy().view(np.uint8), exp) == []
    assert sref.mismatches(sub.cpu().numpy().view(np.uint8), exp) == []


@pytest.mark.parametrize("bs", ["4K", "64K"])
def test_no_records_is_a_copy(torch_mod, codec, bs):
    torch = torch_mod
    bs = SIZES[bs]
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "zipf255", bs, n)
    for pos, lens, max_len in (([], [], 16), ([5, 9], [0, 0], 0)):
        r = scatter(torch, codec, enc, pos, lens, max_len, fill=1, old_sub=enc.sub, want_sub=True, cap=1)
        assert (r.rc, r.status, r.length, r.touched, r.who) == (HUFE_OK, HUFE_OK, enc.length, 0, NONE64)
        assert np.array_equal(r.stream, enc.stream.cpu().numpy()) and np.array_equal(r.index.astype(np.int64), enc.h_offs)
        exp = sref.expected(r.stream, r.index, enc.data, bs)
        got = r.sub.cpu().numpy().view(np.uint8)
        assert sref.mismatches(got, exp) == []
        held = np.full(got.size // 8, SUB_GUARD, dtype=np.int64).view(np.uint8)
        assert sref.unwritten_changed(got, held, exp) == []
    r = scatter(torch, codec, enc, [], [], 16, fill=1, cap=1, out_cap=enc.length - 1)
    assert (r.rc, r.status, r.length, r.touched, r.who) == (HUFE_OK, HUFE_MEMORY, 0, 0, NONE64)
    assert np.all(r.out_all == GUARD)
    # records that write nothing, with records: no block is touched, the stream is the old one
    r = scatter(torch, codec, enc, [n, n + 5, 3], [4, 4, 0], 4, fill=1)
    assert (r.status, r.length, r.touched) == (HUFE_OK, enc.length, 0) and np.array_equal(r.stream, enc.stream.cpu().numpy())


def test_any_old_sub_index_gives_the_same_bytes(torch_mod, codec, oracle):
    """with the stream's own, without one, zeroed, random, another input's: the stream, the index, the touched rows"""
    torch = torch_mod
    bs = 64 * KIB
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "logtext", bs, n)
    pos, lens = random_records(n, 60, 9, 500)
    want = scatter(torch, codec, enc, pos, lens, 500, fill=0x23, old_sub=enc.sub, want_sub=True)
    new, exp = check_model(oracle, enc, want, pos, lens, 500, fill=0x23, what="own", sub="whole")
    other = enc_of(torch, codec, "zipf255", bs, n).sub
    rnd = torch.from_numpy(np.random.default_rng(3).integers(-2**62, 2**62, enc.sub.numel(), dtype=np.int64)).cuda()
    for name, old in (("none", None), ("zeroed", torch.zeros_like(enc.sub)), ("random", rnd), ("foreign", other)):
        r = scatter(torch, codec, enc, pos, lens, 500, fill=0x23, old_sub=old, want_sub=True)
        assert (r.rc, r.status, r.touched) == (HUFE_OK, HUFE_OK, want.touched), name
        assert np.array_equal(r.stream, want.stream) and np.array_equal(r.index, want.index), name
        e = exp.sub()
        hit = np.zeros(e.lay.nb, bool)
        hit[model.touched_blocks(n, bs, pos, lens, 500)] = True
        for w, per in ((e.w_tiles, e.lay.tpb), (e.w_groups, e.lay.gpb), (e.w_lens, 256)):
            w &= np.repeat(hit, per)
        assert sref.mismatches(r.sub.cpu().numpy().view(np.uint8), e) == [], name


# ---- every status of d_result ----------------------------------------------------------------------------------------------
def test_a_record_longer_than_max_len(torch_mod, codec):
    torch = torch_mod
    bs = 4 * KIB
    enc = enc_of(torch, codec, "zipf255", bs, 5 * bs + 100)
    pos = [10, bs + 5, 2 * bs, 3 * bs + 1, 99]
    lens = [8, 9, 8, 4000, 9]
    r = scatter(torch, codec, enc, pos, lens, 8, fill=0)
    assert (r.rc, r.status, r.length, r.who) == (HUFE_OK, HUFE_ARGUMENT, 0, 1)          # the lowest such record
    assert r.touched == 2                                                              # (those records touch nothing)
    lens[1] = 2**32 - 1
    r = scatter(torch, codec, enc, pos, lens, 8, slots=np.zeros((5, 8), np.uint8))
    assert (r.status, r.who) == (HUFE_ARGUMENT, 1)


@pytest.mark.parametrize("bs", ["4K", "64K"])
def test_touched_cap_one_too_small(torch_mod, codec, oracle, bs):
    torch = torch_mod
    bs = SIZES[bs]
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "zipf255", bs, n)
    pos, lens = [5, bs - 2, 2 * bs + 1, 3 * bs + 9, n - 1], [3, 4, 2, 3, 1]             # blocks 0, 1, 2, 3 and 5
    roomy = scatter(torch, codec, enc, pos, lens, 4, fill=0x30, cap=5)
    check_model(oracle, enc, roomy, pos, lens, 4, fill=0x30, what="cap = touched")
    assert roomy.touched == 5
    # a d_out with room for the true count of blocks, so that only the cap is short; scatter() looks at the guards and the input
    r = scatter(torch, codec, enc, pos, lens, 4, fill=0x30, cap=4, out_cap=roomy.outs.room)
    assert (r.rc, r.status, r.length, r.touched, r.who) == (HUFE_OK, HUFE_MEMORY, 0, 5, NONE64)
    r = scatter(torch, codec, enc, pos, lens, 4, fill=0x30, cap=1, out_cap=roomy.outs.room, old_sub=enc.sub, want_sub=True)
    assert (r.status, r.touched) == (HUFE_MEMORY, 5)
    # the context is as good as before
    again = scatter(torch, codec, enc, pos, lens, 4, fill=0x30, cap=5)
    assert again.status == HUFE_OK and np.array_equal(again.stream, roomy.stream)


def flip_payload_bit(enc, b, at=0.5):
    """the input with one payload bit of block b flipped"""
    st = enc.stream.clone()
    o0, o1 = int(enc.h_offs[b]), int(enc.h_offs[b + 1])
    tree_len = int(np.frombuffer(enc.stream[o0 + 8:o0 + 10].cpu().numpy().tobytes(), "<i2")[0])
    pay = o0 + 10 + 2 * tree_len
    st[pay + int((o1 - pay) * at)] ^= 0x10
    return enc.variant(stream=st)


def decode_block(codec, torch, enc, b, relaxed=False):
    room = min(enc.bs, enc.n - b * enc.bs)
    out = torch.empty(room, dtype=torch.uint8, device="cuda")
    raw = C.c_uint64(0)
    offs = enc.offsets[b:b + 2].contiguous()
    return int(codec.lib.hufgpu_decode(codec._ctx, enc.stream.data_ptr(), enc.length, offs.data_ptr(), 1, out.data_ptr(), room,
                                       1 if relaxed else 0, C.byref(raw), None))


@pytest.mark.parametrize("bs", ["4K", "64K"])
def test_payload_damage_in_a_touched_and_in_an_untouched_block(torch_mod, codec, oracle, bs):
    torch = torch_mod
    bs = SIZES[bs]
    n = 8 * bs + 500
    data = datagen.uniform255(n, seed=2)                 # (every code is 8 bits or so: a flipped bit is another symbol or a short payload)
    clean = Enc(torch, codec, data, bs)
    pos, lens = [bs + 100, 5 * bs + 7], [3 * bs, 20]                                    # blocks 1 .. 4 and 5
    want = scatter(torch, codec, clean, pos, lens, 3 * bs, fill=0x11)
    check_model(oracle, clean, want, pos, lens, 3 * bs, fill=0x11, what="clean")
    # untouched: carried over byte for byte, unseen
    enc = flip_payload_bit(clean, 7)
    r = scatter(torch, codec, enc, pos, lens, 3 * bs, fill=0x11)
    assert (r.rc, r.status, r.touched, r.length) == (HUFE_OK, HUFE_OK, 5, want.length) and np.array_equal(r.index, want.index)
    diff = np.flatnonzero(r.stream != want.stream)
    assert diff.size == 1 and int(r.index[7]) <= diff[0] < int(r.index[8])
    # touched, even where the records cover all of the block (2 and 3 do): what hufgpu_decode says of the block.  Damage
    # that only changes symbols decodes - to other bytes, which the records then cover or not
    for b in (5, 2):
        for at in (0.5, 0.999):
            enc = flip_payload_bit(clean, b, at)
            expect = decode_block(codec, torch, enc, b)
            r = scatter(torch, codec, enc, pos, lens, 3 * bs, fill=0x11, old_sub=clean.sub if at == 0.5 else None)
            assert r.rc == HUFE_OK and r.status == expect, (b, at, r.status, expect)
            assert r.who == (b if expect else NONE64)
            if expect == HUFE_OK and b == 2:
                assert np.array_equal(r.stream, want.stream)              # every byte of the block was overwritten
    # a payload cut short fails for sure: the index gives block 5 fewer bytes than its symbols need
    offs = clean.offsets.clone()
    cut = int(clean.h_offs[6]) - (int(clean.h_offs[6]) - int(clean.h_offs[5])) // 2
    st = torch.cat([clean.stream[:cut], clean.stream[int(clean.h_offs[6]):]])
    offs[6:] -= int(clean.h_offs[6]) - cut
    enc = clean.variant(stream=st, offsets=offs, length=int(st.numel()), h_offs=offs.cpu().numpy().astype(np.int64))
    expect = decode_block(codec, torch, enc, 5)
    assert expect != HUFE_OK
    r = scatter(torch, codec, enc, pos, lens, 3 * bs, fill=0x11)
    assert (r.rc, r.status, r.who, r.touched) == (HUFE_OK, expect, 5, 5)
    r = scatter(torch, codec, enc, [10], [20], 20, fill=0x11)                            # the same block untouched: no error
    assert (r.status, r.touched) == (HUFE_OK, 1)


@pytest.mark.parametrize("relaxed", [False, True], ids=["strict", "relaxed"])
def test_a_header_that_does_not_parse(torch_mod, codec, oracle, relaxed):
    torch = torch_mod
    bs = 4 * KIB
    n = 10 * bs + 5
    clean = enc_of(torch, codec, "zipf255", bs, n)
    st = clean.stream.clone()
    for bad_b in (6, 3):
        o = int(clean.h_offs[bad_b])
        st[o + 8], st[o + 9] = 0xFF, 0x7F                # tree_len = 0x7fff: no tree is that long
    enc = clean.variant(stream=st)
    header_err = decode_block(codec, torch, enc, 6, relaxed)
    assert header_err != HUFE_OK
    # around the bad blocks: served; their records are carried over
    pos, lens = [bs + 5, 4 * bs + 1, 7 * bs, n - 3], [bs, 700, 2 * bs + 1, 3]
    r = scatter(torch, codec, enc, pos, lens, 2 * bs + 1, fill=0x5F, relaxed=relaxed)
    want = scatter(torch, codec, clean, pos, lens, 2 * bs + 1, fill=0x5F, relaxed=relaxed)
    check_model(oracle, clean, want, pos, lens, 2 * bs + 1, fill=0x5F, what="clean")
    assert (r.rc, r.status, r.touched, r.length) == (HUFE_OK, HUFE_OK, want.touched, want.length)
    diff = set(np.flatnonzero(r.stream != want.stream).tolist())
    assert diff and diff <= {int(r.index[b]) + k for b in (6, 3) for k in (8, 9)} and np.array_equal(r.index, want.index)
    # a record in a bad block: that header's error, the first such block in stream order
    for pos, who in (([6 * bs + 9], 6), ([6 * bs - 1], 6), ([8 * bs, 6 * bs, 3 * bs + 5, 10], 3), ([2 * bs + 100], 3)):
        r = scatter(torch, codec, enc, pos, None, bs, fill=0x5F, relaxed=relaxed)
        assert (r.rc, r.status, r.who) == (HUFE_OK, header_err, who), (pos, r.status, r.who)
    # a block_len that is not the layout's: HUF_ERROR_READ_WRITE
    st = clean.stream.clone()
    st[int(clean.h_offs[2])] += 1                        # block 2 says bs + 1 symbols
    enc = clean.variant(stream=st)
    r = scatter(torch, codec, enc, [2 * bs + 50, 5], [10, 3], 10, fill=0x5F, relaxed=relaxed)
    assert (r.rc, r.status, r.who, r.touched) == (HUFE_OK, HUFE_RW, 2, 2)
    r = scatter(torch, codec, enc, [3 * bs + 50, 5], [10, 3], 10, fill=0x5F, relaxed=relaxed)
    assert (r.status, r.touched) == (HUFE_OK, 2)


def test_out_cap_one_byte_short(torch_mod, codec, oracle):
    torch = torch_mod
    bs = 4 * KIB
    n = 9 * bs + 10
    enc = enc_of(torch, codec, "logtext", bs, n)
    pos, lens = [bs + 3, 5 * bs], [2 * bs + 6, bs]
    slots = np.random.default_rng(2).integers(0, 256, (2, 2 * bs + 6), dtype=np.uint8)
    full = scatter(torch, codec, enc, pos, lens, 2 * bs + 6, slots=slots)
    check_model(oracle, enc, full, pos, lens, 2 * bs + 6, slots=slots, what="roomy")
    assert full.length > enc.length                      # (random bytes: the new stream is longer than the old one)
    exact = scatter(torch, codec, enc, pos, lens, 2 * bs + 6, slots=slots, out_cap=full.length)
    assert exact.status == HUFE_OK and np.array_equal(exact.stream, full.stream)
    short = scatter(torch, codec, enc, pos, lens, 2 * bs + 6, slots=slots, out_cap=full.length - 1)
    assert (short.rc, short.status, short.length, short.touched, short.who) == (HUFE_OK, HUFE_MEMORY, 0, 4, NONE64)
    assert np.all(short.out_all == GUARD)                # a stream that does not fit is not written at all


def test_the_order_of_the_statuses(torch_mod, codec):
    torch = torch_mod
    bs = 4 * KIB
    n = 10 * bs + 5
    clean = enc_of(torch, codec, "zipf255", bs, n)
    st = clean.stream.clone()
    o = int(clean.h_offs[6])
    st[o + 8], st[o + 9] = 0xFF, 0x7F
    enc = clean.variant(stream=st)
    header_err = decode_block(codec, torch, enc, 6)
    pos, lens = [5, bs + 5, 6 * bs + 1, 8 * bs], [4, 4, 4, 99]
    tiny = 64                                            # an out_cap every new stream is longer than
    # 1 before 2, 3, 4: a record that is too long, a cap that is too small, a bad block, no room
    r = scatter(torch, codec, enc, pos, lens, 4, fill=0, cap=1, out_cap=tiny)
    assert (r.status, r.who, r.touched) == (HUFE_ARGUMENT, 3, 3)
    lens[3] = 4
    # 2 before 3 and 4
    r = scatter(torch, codec, enc, pos, lens, 4, fill=0, cap=3, out_cap=tiny)
    assert (r.status, r.who, r.touched) == (HUFE_MEMORY, NONE64, 4)
    # 3 before 4
    r = scatter(torch, codec, enc, pos, lens, 4, fill=0, cap=4, out_cap=tiny)
    assert (r.status, r.who, r.touched) == (header_err, 6, 4)
    # 4 alone
    r = scatter(torch, codec, clean, pos, lens, 4, fill=0, cap=4, out_cap=tiny)
    assert (r.status, r.who, r.touched) == (HUFE_MEMORY, NONE64, 4)
    assert np.all(r.out_all == GUARD)


# ---- enqueue-only ----------------------------------------------------------------------------------------------------------
def sleep_cycles_per_ms(torch):
    """cycles of torch.cuda._sleep a millisecond, by two events; the spin is made longer until it takes 2 ms"""
    cycles, ms = 1_000_000, 0.0
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 2.0:
            break
        cycles *= 10
    assert ms >= 2.0, ("torch.cuda._sleep does not hold a stream", cycles, ms)
    return cycles / ms


def test_on_a_side_stream_behind_a_long_kernel(torch_mod, codec, oracle):
    """The positions the call reads are uploaded on the side stream BEHIND a kernel that holds it for 50 ms.  A call that
    only enqueues returns with that kernel still running; a launch that went to another stream would read the decoy
    positions that the buffer holds until then, and the output would be the decoy's."""
    torch = torch_mod
    bs = 4 * KIB
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "logtext", bs, n)
    real, rlens = random_records(n, 100, 21, 40)
    decoy = [p ^ 0x400 for p in real]
    d_pos = torch.from_numpy(np.asarray(decoy, np.int64)).cuda()
    d_real = torch.from_numpy(np.asarray(real, np.int64)).cuda()
    d_len = torch.from_numpy(np.asarray(rlens, np.int32)).cuda()
    warm = scatter(torch, codec, enc, decoy, rlens, 40, fill=0x7E, d_pos=d_pos, d_len=d_len, old_sub=enc.sub, want_sub=True)
    assert warm.status == HUFE_OK                        # the workspaces stand: the next call has nothing to grow
    per_ms = sleep_cycles_per_ms(torch)
    s = torch.cuda.Stream()
    before = enc.stream.clone()
    # the call once on s itself, on the decoy, and a wait: a stream's first launch of a kernel that needs scratch memory (the
    # exact decoder) can take the host longer than the long kernel runs - that is the stream's first use, not the call
    with torch.cuda.stream(s):
        primed = scatter(torch, codec, enc, None, None, 40, fill=0x7E, d_pos=d_pos, d_len=d_len, old_sub=enc.sub, want_sub=True,
                         stream=s, outs=warm.outs)
        s.synchronize()
    assert primed.rc == HUFE_OK
    torch.cuda.synchronize()
    collecting = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(50 * per_ms))
            opened = torch.cuda.Event()
            opened.record(s)
            d_pos.copy_(d_real, non_blocking=True)
            r = scatter(torch, codec, enc, None, None, 40, fill=0x7E, d_pos=d_pos, d_len=d_len, old_sub=enc.sub, want_sub=True,
                        stream=s, outs=warm.outs)
            closed = not opened.query()
    finally:
        if collecting:
            gc.enable()
    s.synchronize()
    torch.cuda.synchronize()
    assert r.rc == HUFE_OK
    assert closed, "the long kernel had ended before the call returned: this run has proved nothing"
    assert torch.equal(before, enc.stream)
    r = fetch(r, enc)
    check_model(oracle, enc, r, real, rlens, 40, fill=0x7E, what="side stream", sub="whole")


def capture(torch, s, enqueue):
    """enqueue() captured on s in global mode - any wait ends the capture with an error.  Nothing may be finalised while s
    captures, so the collector rests; a capture that fails fails the test and nothing else."""
    graph, outs, error = torch.cuda.CUDAGraph(), None, None
    gc.collect()
    collecting = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(s):
            graph.capture_begin(capture_error_mode="global")
            try:
                outs = enqueue()
            except Exception as e:                       # noqa: BLE001 - whatever it is, the capture has to end first
                error = e
            try:
                graph.capture_end()
            except Exception as e:                       # noqa: BLE001
                error = error or e
    finally:
        if collecting:
            gc.enable()
    if error is not None:
        message = f"the call could not be captured: {type(error).__name__}: {error}"
        outs = error = None
        del graph
        torch.cuda.synchronize()
        raise AssertionError(message)
    return graph, outs


def test_captured_in_a_graph_and_replayed_twice(torch_mod, codec, oracle):
    """source mode; positions, lengths and new bytes change between the replays: a replay reads them anew"""
    torch = torch_mod
    bs = 64 * KIB
    n = 5 * bs + 100
    enc = enc_of(torch, codec, "zipf255", bs, n)
    sets = []
    for seed in (31, 32):
        pos, lens = random_records(n, 50, seed, 64)
        target = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        sets.append((pos, lens, slots_of(target, pos, lens, 64, n)))
    d_pos = torch.zeros(50, dtype=torch.int64, device="cuda")
    d_len = torch.zeros(50, dtype=torch.int32, device="cuda")
    d_src = torch.zeros(50 * 64, dtype=torch.uint8, device="cuda")
    kw = dict(d_pos=d_pos, d_len=d_len, d_src=d_src, stride=64, old_sub=enc.sub, want_sub=True, cap=enc.nb)
    warm = scatter(torch, codec, enc, None, None, 64, **kw)
    assert warm.status == HUFE_OK
    s = torch.cuda.Stream()
    graph, r = capture(torch, s, lambda: scatter(torch, codec, enc, None, None, 64, stream=s, outs=warm.outs, **kw))
    assert r.rc == HUFE_OK
    for pos, lens, slots in sets:
        with torch.cuda.stream(s):
            d_pos.copy_(torch.from_numpy(np.asarray(pos, np.int64)).cuda())
            d_len.copy_(torch.from_numpy(np.asarray(lens, np.int32)).cuda())
            d_src.copy_(dev(torch, slots.reshape(-1)))
            warm.outs.out.fill_(GUARD)
            warm.outs.res.fill_(RES_GUARD)
            graph.replay()
            s.synchronize()
        got = fetch(r, enc)
        check_model(oracle, enc, got, pos, lens, 64, slots=slots, what="replay", sub="whole")
    del graph
    torch.cuda.synchronize()


def lines_input(torch, codec, nlines=400, bs=4 * KIB):
    text = make("logtext", 64 * KIB).tobytes()
    cut = -1
    for _ in range(nlines):
        cut = text.index(b"\n", cut + 1)
    data = np.frombuffer(text[:cut + 1], np.uint8).copy()
    return Enc(torch, codec, data, bs)


def test_find_pattern_then_scatter_captured_as_one_graph(torch_mod, codec, oracle):
    """hufgpu_find_pattern writes the starts, hufgpu_scatter blanks them, one graph, no host step in between.  The scatter
    is given the search's cap as its number of records: the positions are set to raw_size by a device op in front of the
    search, so the rows behind the found count are records that write nothing.  Every buffer is made outside the capture."""
    torch = torch_mod
    enc = lines_input(torch, codec)
    text = enc.data.tobytes()
    pattern, cap = b"cache", 512
    starts = [m.start() for m in re.finditer(pattern, text)]
    assert 0 < len(starts) < cap
    d_pos = torch.zeros(cap, dtype=torch.int64, device="cuda")
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    errs = torch.zeros(enc.nb, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def enqueue(outs=None):
        d_pos.fill_(enc.n)
        rc = codec.lib.hufgpu_find_pattern(codec._ctx, enc.stream.data_ptr(), enc.length, enc.offsets.data_ptr(), enc.nb,
                                           enc.sub.data_ptr(), enc.n, enc.bs, pattern, len(pattern), d_pos.data_ptr(), cap, None,
                                           totals.data_ptr(), errs.data_ptr(), 0, C.c_void_p(s.cuda_stream))
        assert rc == HUFE_OK
        return scatter(torch, codec, enc, None, None, len(pattern), fill=0x23, d_pos=d_pos, old_sub=enc.sub, want_sub=True,
                       stream=s, outs=outs)

    def look(r):
        assert r.rc == HUFE_OK and totals.cpu().tolist() == [len(starts), len(starts), 0, 0]
        check_model(oracle, enc, fetch(r, enc), starts, None, len(pattern), fill=0x23, what="find -> scatter", sub="whole")

    with torch.cuda.stream(s):                           # warm-up on the stream itself: the workspaces stand
        warm = enqueue()
        s.synchronize()
    look(warm)
    graph, r = capture(torch, s, lambda: enqueue(warm.outs))
    for _ in range(2):
        with torch.cuda.stream(s):
            warm.outs.out.fill_(GUARD)
            warm.outs.res.fill_(RES_GUARD)
            totals.fill_(-1)
            graph.replay()
            s.synchronize()
        look(r)
    del graph
    torch.cuda.synchronize()


class GuardedOut:
    """A d_out for the Python layer between guard bytes.  GpuCodec.scatter / redact make the new index, the result words and
    the new sub-index themselves, as torch tensors of exactly the size the call is told - those three cannot be given guard
    words from here (the C-ABI helper above has them around all four, for the same kernels); the output buffer can."""

    def __init__(self, torch, codec, enc, blocks=None):
        room = enc.length + (enc.nb if blocks is None else blocks) * codec.encode_bound(min(enc.bs or enc.n, enc.n), 0) + 64
        self.big = torch.full((room + 2 * GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
        self.out, self.room = self.big[GUARD_BYTES:GUARD_BYTES + room], room

    def check(self, length):
        hb = self.big.cpu().numpy()
        assert np.all(hb[:GUARD_BYTES] == GUARD) and np.all(hb[GUARD_BYTES + self.room:] == GUARD), "guard bytes around d_out"
        assert np.all(hb[GUARD_BYTES + length:GUARD_BYTES + self.room] == GUARD), "bytes behind the new stream were written"

    def fresh(self):
        self.big.fill_(GUARD)
        return self.out


def test_redact_against_re_sub(torch_mod, codec, oracle):
    """400 log lines: a literal, an ignore-case class pattern, whole lines; then the search finds nothing in the result"""
    torch = torch_mod
    enc = lines_input(torch, codec)
    text = enc.data.tobytes()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
    stars = lambda m: b"*" * len(m.group())             # noqa: E731
    guarded = GuardedOut(torch, codec, enc)
    cases = [
        ("literal", dict(pattern=b"request"), re.sub(rb"request", stars, text)),
        ("classes, ignore case", dict(pattern=[b"e", b"r", b"r", b"o", b"r", b" "], ignore_case=True), re.sub(rb"(?i)error ", stars, text)),
        ("any of one length", dict(pattern=codec.AnyOf(b"WARN ", b"INFO ", b"http.")), re.sub(rb"WARN |INFO |http\.", stars, text)),
        ("lines", dict(pattern=b"WARN", lines=True, max_len=256), re.sub(rb"(?m)^.*WARN.*$", stars, text)),
    ]
    for name, kw, want in cases:
        assert want != text, name
        out, offs, result, sub, totals = codec.redact(*args, max_matches=2048, want_sub_index=True, out=guarded.fresh(), **kw)
        length, touched = codec.scatter_result(result)
        guarded.check(length)
        exp = model.Expected(oracle, np.frombuffer(want, np.uint8), enc.bs)
        assert length == exp.length and np.array_equal(out[:length].cpu().numpy(), exp.stream), name
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), exp.offs), name
        assert 0 < int(totals[1]) == int(totals[0]) < 2048, name        # the cap was not reached: rows behind the count were harmless
        find = {k: v for k, v in kw.items() if k not in ("lines", "max_len")}
        totals2, errs2 = codec.count_pattern(out, length, offs, enc.nb, sub, enc.n, enc.bs, **find)
        assert int(totals2[0]) == 0 and int(totals2[2]) == 0, name       # nothing is found, in blocks that are all served
    # a cap below the count: the first max_matches occurrences are blanked, ascending
    out, offs, result, sub, totals = codec.redact(*args, b"request", max_matches=7, out=guarded.fresh())
    length, _ = codec.scatter_result(result)
    guarded.check(length)
    assert int(totals[0]) == text.count(b"request") > 7 and int(totals[1]) == 7
    want = re.sub(rb"request", stars, text, count=7)
    exp = model.Expected(oracle, np.frombuffer(want, np.uint8), enc.bs)
    assert length == exp.length and np.array_equal(out[:length].cpu().numpy(), exp.stream)


def test_the_python_layer_and_interleaved_calls(torch_mod, codec, oracle):
    """call after call on one context, with update_ranges, append, gather and decodes in between"""
    torch = torch_mod
    bs = 64 * KIB
    n = 4 * bs + 100
    data = make("zipf255", n)
    enc = Enc(torch, codec, data, bs)
    args = (enc.stream, enc.length, enc.offsets, enc.nb)
    pos, lens = random_records(n, 30, 41, 100)
    d_pos = torch.from_numpy(np.asarray(pos, np.int64)).cuda()
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    new = model.apply(data, pos, lens, 100, fill=0x20)
    exp = model.Expected(oracle, new, bs)

    guarded = GuardedOut(torch, codec, enc)

    def one_scatter():
        out, offs, result, sub = codec.scatter(*args, d_pos, d_len, fill=0x20, raw_size=n, blocksize=bs, sub_index=enc.sub,
                                               max_len=100, want_sub_index=True, out=guarded.fresh())
        length, touched = codec.scatter_result(result)
        guarded.check(length)
        assert length == exp.length and touched == len(model.touched_blocks(n, bs, pos, lens, 100))
        assert np.array_equal(out[:length].cpu().numpy(), exp.stream)
        return out, offs, length, sub

    out1, offs1, length1, sub1 = one_scatter()
    ranges = [(100, bs + 100), (3 * bs - 1, 3 * bs + 1)]
    patch = dev(torch, np.random.default_rng(3).integers(0, 100, bs + 2, dtype=np.uint8))
    u1 = codec.update_ranges(*args, ranges, patch, blocksize=bs)
    out2, offs2, length2, sub2 = one_scatter()
    # gather -> the caller's kernel -> scatter: the slots go back as they came, at gather's stride
    wide = torch.zeros((30, 128), dtype=torch.uint8, device="cuda")
    got, errs, raws = codec.gather(*args, d_pos, d_len, sub_index=enc.sub, raw_size=n, blocksize=bs, max_len=100, out=wide[:, :100])
    upper = torch.where((got >= 0x61) & (got <= 0x7A), got - 0x20, got)
    wide[:, :100] = upper
    other = GuardedOut(torch, codec, enc)
    out3, offs3, result3, _ = codec.scatter(*args, d_pos, d_len, data=wide[:, :100], raw_size=n, blocksize=bs, max_len=100,
                                            out=other.fresh())
    length3, _ = codec.scatter_result(result3)
    other.check(length3)
    assert int(errs.abs().sum()) == 0
    full = data.copy()
    lower = (full >= 0x61) & (full <= 0x7A)
    mask = np.zeros(n, bool)
    for p, k in zip(pos, lens):
        mask[p:p + k] = True
    full[mask & lower] -= 0x20
    exp3 = model.Expected(oracle, full, bs)
    assert length3 == exp3.length and np.array_equal(out3[:length3].cpu().numpy(), exp3.stream)
    # append works in place on a copy; then the same scatter again, and an update that still gives what it gave
    st = torch.zeros(enc.length + codec.encode_bound(bs + 1000, bs), dtype=torch.uint8, device="cuda")
    st[:enc.length] = enc.stream
    offs = torch.zeros(enc.nb + 2, dtype=torch.int64, device="cuda")
    offs[:enc.nb + 1] = enc.offsets
    codec.append(st, enc.length, offs, n, bs, dev(torch, np.arange(1000) % 251))
    out4, offs4, length4, sub4 = one_scatter()
    u2 = codec.update_ranges(*args, ranges, patch, blocksize=bs)
    assert u1[1] == u2[1] and torch.equal(u1[0], u2[0])
    # the new stream decodes to D' with its new sub-index, every row verified
    outd = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert codec.decode(out4, length4, offs4, enc.nb, outd, sub_index=sub4, raw_size=n, blocksize=bs) == n
    assert np.array_equal(outd.cpu().numpy(), new) and codec.decode_counters()[0] == 0
    # a failure is raised by scatter_result with the record that caused it
    d_long = d_len.clone()
    d_long[4] = 101
    _, _, result, _ = codec.scatter(*args, d_pos, d_long, fill=0, raw_size=n, blocksize=bs, max_len=100)
    with pytest.raises(Exception) as e:
        codec.scatter_result(result)
    assert e.value.err == HUFE_ARGUMENT and e.value.raw == 4

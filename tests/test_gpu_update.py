"""GPU tests of hufgpu_update_ranges (GpuCodec.update_ranges / update_range): byte ranges of the original data
overwritten in one indexed stream, out of place.

Bit-exact, no tolerance.  The expected stream and block index are the oracle's encode of D' (the data with the ranges
replaced) and, as a second witness, hufgpu_encode of D'.  The number of re-encoded blocks is counted on the CPU from the
block positions P and the ranges.  Every output - the stream, the index, the sub-index - lies between guard bytes that
must still hold their fill, and the old stream is compared with a copy taken before the call.
"""
import ctypes as C

import numpy as np
import pytest

import sub_index_ref as sref
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 80
HUFE_OK, HUFE_MEMORY, HUFE_ARGUMENT = 0, 1, 2
TREE_STRICT, TREE_MAX = 1024, 1025
KIB, MIB = 1 << 10, 1 << 20


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
    if kind == "zipf255":
        return datagen.zipf255(n, seed=3 + seed)
    if kind == "uniform256":
        return datagen.uniform256(n, seed=1 + seed)
    if kind == "logtext":
        return datagen.logtext(n, seed=5 + seed)
    raise ValueError(kind)


class Enc:
    """an encoded input: the stream and index on the device, P = where each block's bytes start in the raw data"""

    def __init__(self, torch, codec, data, bs, stream=None, offsets=None, block_lens=None, sub=False):
        self.data, self.bs, self.n = data, bs, int(data.size)
        self.sub = None
        if stream is None:
            self.sub = codec.new_sub_index(self.n, bs) if sub else None
            stream, offsets, _ = codec.encode(dev(torch, data), bs, sub_index=self.sub)
            nb = codec.block_count(self.n, bs)
            block_lens = [min(bs or self.n, self.n - b * (bs or self.n)) for b in range(nb)]
        self.stream, self.offsets = stream, offsets
        self.length = int(stream.numel())
        self.block_lens = list(block_lens)
        self.nb = len(block_lens)
        self.P = np.concatenate([[0], np.cumsum(block_lens)]).astype(np.int64)
        self.h_offs = offsets.cpu().numpy().astype(np.int64)


def patched(data, ranges, patches):
    out = data.copy()
    for (lo, hi), p in zip(ranges, patches):
        assert p.size == hi - lo
        out[lo:hi] = p
    return out


def touched_blocks(P, ranges):
    """the blocks (of non-zero length) that hold a byte of a range: the CPU's count"""
    hit = np.zeros(P.size - 1, bool)
    for lo, hi in ranges:
        if lo < hi:
            fb = int(np.searchsorted(P, lo, side="right")) - 1
            lb = int(np.searchsorted(P, hi, side="left")) - 1
            hit[fb:lb + 1] = True
    hit &= np.diff(P) > 0
    return hit


def random_patches(ranges, seed, kind="uniform"):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return [rng.integers(0, 256, hi - lo, dtype=np.uint8) for lo, hi in ranges]
    return [rng.integers(0x30, 0x3a, hi - lo, dtype=np.uint8) for lo, hi in ranges]          # ten values: short codes


class Result:
    pass


def update(torch, codec, enc, ranges, patches, scatter_seed=None, old_sub=None, want_sub=False, relaxed=False, out_cap=None,
           out_off=4, layout=None, idx_lead=2):
    """one call through the C ABI with guarded buffers; the new bytes at odd offsets of d_src when scatter_seed is given;
    d_out lies 4 out_off bytes behind a 16-byte aligned address (the packer wants whole words of the destination); the new
    index lies idx_lead words behind one (1: the index kernel's stores go word by word)"""
    out_off *= 4
    lib = codec.lib
    nr = len(ranges)
    lens = [hi - lo for lo, hi in ranges]
    if scatter_seed is None:
        so, src = None, (np.concatenate(patches) if patches else np.zeros(0, np.uint8))
    else:
        rng = np.random.default_rng(scatter_seed)
        order = rng.permutation(nr)
        so, pos = [0] * nr, 1
        for i in order:
            so[i] = pos
            pos += lens[i] + int(rng.integers(0, 6)) * 2 + 1
        src = np.full(pos + 8, 0xEE, np.uint8)
        for i in range(nr):
            src[so[i]:so[i] + lens[i]] = patches[i]
    d_src = dev(torch, src if src.size else np.zeros(1, np.uint8))
    hit = touched_blocks(enc.P, ranges)
    room = int((np.diff(enc.P)[hit] * 9 // 8 + 2100).sum())          # every touched block at its bound
    cap = enc.length + room + 64 if out_cap is None else out_cap
    big = torch.full((cap + 2 * GUARD_BYTES + out_off + 3,), GUARD, dtype=torch.uint8, device="cuda")
    out = big[GUARD_BYTES + out_off:GUARD_BYTES + out_off + cap]
    idx_big = torch.full((enc.nb + 1 + 4,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    idx = idx_big[idx_lead:idx_lead + enc.nb + 1]
    n_lay, bs_lay = layout if layout is not None else (enc.n, enc.bs)
    sub_big = sub_new = None
    if want_sub:
        words = -(-codec.sub_index_bytes(n_lay, bs_lay) // 8)
        sub_big = torch.full((words + 4,), 0x7B7B7B7B7B7B7B7B, dtype=torch.int64, device="cuda")
        sub_new = sub_big[2:2 + words]
    with_layout = want_sub or old_sub is not None
    before = enc.stream.clone()
    out_len, count = C.c_uint64(0), C.c_uint64(0)
    rc = lib.hufgpu_update_ranges(codec._ctx, enc.stream.data_ptr(), enc.length, enc.offsets.data_ptr(), enc.nb, nr,
                                  (C.c_uint64 * max(1, nr))(*[lo for lo, _ in ranges]),
                                  (C.c_uint64 * max(1, nr))(*[hi for _, hi in ranges]),
                                  (C.c_uint64 * max(1, nr))(*so) if so is not None else None, d_src.data_ptr(),
                                  old_sub.data_ptr() if old_sub is not None else None,
                                  n_lay if with_layout else 0, bs_lay if with_layout else 0,
                                  out.data_ptr(), cap, idx.data_ptr(), sub_new.data_ptr() if sub_new is not None else None,
                                  1 if relaxed else 0, C.byref(out_len), C.byref(count), None)
    r = Result()
    r.rc, r.length, r.count = int(rc), int(out_len.value), int(count.value)
    hb = big.cpu().numpy()
    lead = GUARD_BYTES + out_off
    assert np.all(hb[:lead] == GUARD) and np.all(hb[lead + cap:] == GUARD), "guard bytes around d_out"
    hi_ = idx_big.cpu().numpy()
    assert np.all(hi_[:idx_lead] == -0x5A5A5A5A5A5A5A5B) and np.all(hi_[idx_lead + enc.nb + 1:] == -0x5A5A5A5A5A5A5A5B), "guard words around the index"
    if sub_big is not None:
        hs = sub_big.cpu().numpy()
        assert np.all(hs[:2] == 0x7B7B7B7B7B7B7B7B) and np.all(hs[-2:] == 0x7B7B7B7B7B7B7B7B), "guard words around the sub-index"
    assert torch.equal(before, enc.stream), "the old stream was written"
    r.out_all = hb[lead:lead + cap]
    r.stream = r.out_all[:r.length]
    r.d_stream = out[:r.length]
    r.d_index = idx
    r.index = hi_[idx_lead:idx_lead + enc.nb + 1].astype(np.uint64)
    r.sub = sub_new
    r.cap = cap
    if rc != HUFE_OK:
        assert r.length == 0 and r.count == 0, "on any error *out_len = 0"
    return r


def check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, what, relaxed=False):
    """stream and index equal the oracle's and hufgpu_encode's encode of D'; the count is the CPU's"""
    assert r.rc == HUFE_OK, (what, r.rc, codec.lib.hufgpu_last_error(codec._ctx).decode())
    new = patched(enc.data, ranges, patches)
    want, woffs = oracle.encode(new, enc.bs, with_offsets=True)
    assert r.length == want.size, (what, r.length, want.size)
    bad = np.flatnonzero(r.stream != want)
    assert bad.size == 0, (what, "stream differs from the oracle's at", bad[:8], "index", woffs[:6])
    assert np.array_equal(r.index, woffs), (what, "index")
    st2, offs2, len2 = codec.encode(dev(torch, new), enc.bs)
    assert len2 == r.length and np.array_equal(st2.cpu().numpy(), r.stream), (what, "hufgpu_encode of D'")
    assert np.array_equal(offs2.cpu().numpy().astype(np.uint64), r.index), (what, "hufgpu_encode's index")
    assert r.count == int(touched_blocks(enc.P, ranges).sum()), (what, "blocks_reencoded", r.count)
    return new, want, woffs


def shapes(n, bs):
    s = {
        "inside a block": [(bs + 10, bs + 100)],
        "exactly a block": [(bs, 2 * bs)],
        "border to border": [(bs, min(3 * bs, n - n % bs))],
        "across many blocks, cut on both sides": [(bs // 2 + 3, n - bs // 3 - 1)],
        "several ranges in one block": [(bs + 100, bs + 301), (bs + 1, bs + 5), (bs + 7, bs + 8)],
        "first and last byte": [(0, 1), (n - 1, n)],
        "empty ranges": [(5, 5), (n, n), (bs + 3, bs + 9), (n + 100, n + 100), (bs + 5, bs + 5)],
        "a whole block and a cut one in one range, a block shared by two": [(bs - 7, 2 * bs), (2 * bs, 2 * bs + 9)],
        "the last, short block exactly": [(n - n % bs, n)],
        "everything": [(0, n)],
    }
    return s


SIZES = {4 * KIB: 21 * 4 * KIB + 1234, 64 * KIB: 6 * 64 * KIB + 777, MIB: 3 * MIB + 4321, 2 * MIB: 2 * 2 * MIB + 99999}


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB, MIB, 2 * MIB], ids=["4K", "64K", "1M", "2M"])
@pytest.mark.parametrize("kind", ["zipf255", "uniform256", "logtext"])
def test_output_and_index_equal_the_encode_of_the_new_data(torch_mod, codec, oracle, kind, bs):
    torch = torch_mod
    n = SIZES[bs]
    assert n % bs != 0                                   # a short last block
    data = make(kind, n)
    enc = Enc(torch, codec, data, bs)
    for k, (name, ranges) in enumerate(shapes(n, bs).items()):
        patches = random_patches(ranges, 100 + k, "digits" if kind == "uniform256" else "uniform")
        # (uniform bytes: blocks with all 256 values have the 1 025-entry tree that only the relaxed flag takes)
        r = update(torch, codec, enc, ranges, patches, scatter_seed=(k if k % 2 else None), out_off=k % 5,
                   relaxed=kind == "uniform256")
        check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, (kind, bs, name))
        if name == "everything":
            assert r.count == enc.nb


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_no_ranges_is_a_copy(torch_mod, codec, bs):
    torch = torch_mod
    data = make("zipf255", SIZES[bs])
    enc = Enc(torch, codec, data, bs, sub=True)
    for ranges in ([], [(7, 7), (0, 0)]):
        r = update(torch, codec, enc, ranges, [np.zeros(0, np.uint8)] * len(ranges), old_sub=enc.sub, want_sub=True)
        assert (r.rc, r.count, r.length) == (HUFE_OK, 0, enc.length)
        assert np.array_equal(r.stream, enc.stream.cpu().numpy())
        assert np.array_equal(r.index.astype(np.int64), enc.h_offs)
        # the sub-index: every entry the encoder writes, and nothing else
        exp = sref.expected(r.stream, r.index, data, bs)
        got = r.sub.cpu().numpy().view(np.uint8)
        assert sref.mismatches(got, exp) == []
        fill = np.full(got.size // 8, 0x7B7B7B7B7B7B7B7B, dtype=np.int64).view(np.uint8)
        assert sref.unwritten_changed(got, fill, exp) == []


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_a_block_becomes_one_byte_and_a_one_byte_block_becomes_mixed(torch_mod, codec, oracle, bs):
    """record sizes change in both directions: block 1 shrinks to a five-entry tree, block 2 (all 0x41) grows"""
    torch = torch_mod
    n = 5 * bs + 99
    data = make("zipf255", n)
    data[2 * bs:3 * bs] = 0x41
    enc = Enc(torch, codec, data, bs, sub=True)
    ranges = [(bs, 2 * bs), (2 * bs + 5, 2 * bs + 50)]
    patches = [np.full(bs, 0x07, np.uint8), np.random.default_rng(1).integers(0, 256, 45, dtype=np.uint8)]
    r = update(torch, codec, enc, ranges, patches, old_sub=enc.sub, want_sub=True)
    new, want, woffs = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, ("one byte", bs))
    assert woffs[2] - woffs[1] == 10 + 2 * 5 + bs // 8 and r.count == 2          # a five-entry tree, one bit a byte
    check_sub_index(torch, codec, r, new, want, woffs, bs)
    # and the other way round in one block: a cut edge turns a mixed block into one byte
    ranges = [(3 * bs + 1, 4 * bs)]
    first = int(data[3 * bs])
    patches = [np.full(bs - 1, first, np.uint8)]
    r = update(torch, codec, enc, ranges, patches)
    _, _, woffs = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, ("one byte by a cut", bs))
    assert woffs[4] - woffs[3] == 10 + 2 * 5 + bs // 8


def random_ranges(n, count, seed, longest):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n - 1), size=2 * count, replace=False))
    out = []
    for i in range(count):
        lo, hi = int(cuts[2 * i]), int(cuts[2 * i + 1])
        out.append((lo, min(hi, lo + 1 + int(rng.integers(0, longest)))))
    order = rng.permutation(count)
    return [out[i] for i in order]


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_400_random_ranges_at_odd_positions(torch_mod, codec, oracle, bs):
    torch = torch_mod
    n = 3 * MIB + 12345
    data = make("zipf255", n)
    enc = Enc(torch, codec, data, bs, sub=True)
    for seed, longest in ((1, 300), (2, 3 * bs)):
        ranges = random_ranges(n, 400, seed, longest)
        patches = random_patches(ranges, seed)
        r = update(torch, codec, enc, ranges, patches, scatter_seed=seed, old_sub=enc.sub, want_sub=True, out_off=seed)
        new, want, woffs = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, ("400 ranges", bs, seed))
        check_sub_index(torch, codec, r, new, want, woffs, bs)


def check_sub_index(torch, codec, r, new, want, woffs, bs):
    """the new sub-index against the CPU reference on the entries the encoder writes, and both decoders with it give D'"""
    n = new.size
    exp = sref.expected(want, woffs, new, bs)
    got = r.sub.cpu().numpy().view(np.uint8)
    assert sref.mismatches(got, exp) == [], "(block, array, index, found, expected)"
    fill = np.full(got.size // 8, 0x7B7B7B7B7B7B7B7B, dtype=np.int64).view(np.uint8)
    assert sref.unwritten_changed(got, fill, exp) == [], "(block, array, index, found, held)"
    nb = exp.lay.nb
    out = torch.full((n + 32,), GUARD, dtype=torch.uint8, device="cuda")
    raw = codec.decode(r.d_stream, r.length, r.d_index, nb, out[:n], relaxed=True, sub_index=r.sub, raw_size=n, blocksize=bs)
    assert raw == n and np.array_equal(out.cpu().numpy()[:n], new) and np.all(out.cpu().numpy()[n:] == GUARD)
    assert codec.decode_counters()[0] == 0               # every row verified: no block went to the exact decoder
    probes = [(0, min(n, 5000)), (n // 3, n // 3 + 2 * bs + 17), (n - 77, n)]
    outr, errs, raws = codec.decode_ranges(r.d_stream, r.length, r.d_index, nb, probes, relaxed=True, sub_index=r.sub,
                                           raw_size=n, blocksize=bs)
    assert errs == [0, 0, 0]
    got_r, at = outr.cpu().numpy(), 0
    for (lo, hi), raw_i in zip(probes, raws):
        assert raw_i == hi - lo and np.array_equal(got_r[at:at + raw_i], new[lo:hi])
        at += raw_i


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB, MIB], ids=["4K", "64K", "1M"])
def test_the_new_sub_index(torch_mod, codec, oracle, bs):
    """with the old sub-index the buffer holds the whole new one; zeroed, random or stale old ones change nothing"""
    torch = torch_mod
    n = SIZES[bs]
    data = make("logtext", n)
    enc = Enc(torch, codec, data, bs, sub=True)
    ranges = [(bs // 2 + 3, 2 * bs + 9), (3 * bs, 3 * bs + 40), (n - 5, n)]
    patches = random_patches(ranges, 7)
    r = update(torch, codec, enc, ranges, patches, old_sub=enc.sub, want_sub=True)
    new, want, woffs = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, ("sub", bs))
    check_sub_index(torch, codec, r, new, want, woffs, bs)
    good = r.sub.cpu().numpy().copy()

    # only the new one: the touched rows, nothing else
    r2 = update(torch, codec, enc, ranges, patches, want_sub=True)
    check_equals_encode(torch, codec, oracle, enc, ranges, patches, r2, ("sub, no old one", bs))
    exp = sref.expected(want, woffs, new, bs)
    hit = touched_blocks(enc.P, ranges)
    lay = exp.lay
    for w, per in ((exp.w_tiles, lay.tpb), (exp.w_groups, lay.gpb), (exp.w_lens, 256)):
        w &= np.repeat(hit, per)
    got2 = r2.sub.cpu().numpy().view(np.uint8)
    assert sref.mismatches(got2, exp) == []
    fill = np.full(got2.size // 8, 0x7B7B7B7B7B7B7B7B, dtype=np.int64).view(np.uint8)
    assert sref.unwritten_changed(got2, fill, exp) == []

    # an old sub-index that is zeroed, random or stale (another input's): the stream, the index and the touched rows are the same
    other = Enc(torch, codec, make("zipf255", n), bs, sub=True).sub
    rnd = torch.from_numpy(np.random.default_rng(3).integers(-2**62, 2**62, enc.sub.numel(), dtype=np.int64)).cuda()
    for name, old in (("zeroed", torch.zeros_like(enc.sub)), ("random", rnd), ("stale", other)):
        r3 = update(torch, codec, enc, ranges, patches, old_sub=old, want_sub=True)
        assert r3.rc == HUFE_OK and r3.count == r.count, name
        assert np.array_equal(r3.stream, r.stream) and np.array_equal(r3.index, r.index), name
        assert sref.mismatches(r3.sub.cpu().numpy().view(np.uint8), exp) == [], name
    assert np.array_equal(good, r.sub.cpu().numpy())


def flip_payload_bit(torch, enc, b, at=0.5):
    """a copy of the stream with one payload bit of block b flipped"""
    st = enc.stream.clone()
    o0, o1 = int(enc.h_offs[b]), int(enc.h_offs[b + 1])
    tree_len = int(np.frombuffer(enc.stream[o0 + 8:o0 + 10].cpu().numpy().tobytes(), "<i2")[0])
    pay = o0 + 10 + 2 * tree_len
    pos = pay + int((o1 - pay) * at)
    st[pos] ^= 0x10
    other = object.__new__(Enc)
    other.__dict__.update(enc.__dict__)
    other.stream = st
    return other


def decode_block(codec, torch, enc, b, relaxed=False):
    room = int(enc.block_lens[b])
    out = torch.empty(room, dtype=torch.uint8, device="cuda")
    raw = C.c_uint64(0)
    offs = enc.offsets[b:b + 2].contiguous()
    return int(codec.lib.hufgpu_decode(codec._ctx, enc.stream.data_ptr(), enc.length, offs.data_ptr(), 1, out.data_ptr(), room,
                                       1 if relaxed else 0, C.byref(raw), None))


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_payload_damage(torch_mod, codec, oracle, bs):
    torch = torch_mod
    n = 8 * bs + 500
    data = make("uniform256", n)                        # (every code is 8 or 9 bits: a flipped bit is another symbol or a short payload)
    data[::7] = 0                                       # (all 256 values in a block: the relaxed flag)
    clean = Enc(torch, codec, data, bs)
    # blocks 2 .. 4 are direct, 1 and 5 staged
    ranges = [(bs + 100, 5 * bs + 100)]
    patches = random_patches(ranges, 11)
    want = update(torch, codec, clean, ranges, patches, relaxed=True)
    check_equals_encode(torch, codec, oracle, clean, ranges, patches, want, ("clean", bs))

    # untouched: carried over byte for byte
    enc = flip_payload_bit(torch, clean, 7)
    r = update(torch, codec, enc, ranges, patches, relaxed=True)
    assert r.rc == HUFE_OK and r.count == 5 and r.length == want.length
    diff = np.flatnonzero(r.stream != want.stream)
    assert diff.size == 1 and int(r.index[7]) <= diff[0] < int(r.index[8])
    assert np.array_equal(r.stream[int(r.index[7]):int(r.index[8])], enc.stream[int(enc.h_offs[7]):int(enc.h_offs[8])].cpu().numpy())
    assert np.array_equal(r.index, want.index)

    # direct: the old payload is never looked at
    enc = flip_payload_bit(torch, clean, 3)
    r = update(torch, codec, enc, ranges, patches, relaxed=True)
    assert r.rc == HUFE_OK and r.count == 5
    assert np.array_equal(r.stream, want.stream) and np.array_equal(r.index, want.index)

    # staged: what hufgpu_decode of the block says - damage that shortens the payload is an error, damage that only changes
    # symbols decodes (to other bytes, which are encoded)
    for at in (0.5, 0.999):
        enc = flip_payload_bit(torch, clean, 5, at)
        expect = decode_block(codec, torch, enc, 5, relaxed=True)
        r = update(torch, codec, enc, ranges, patches, relaxed=True)
        assert r.rc == expect, (at, r.rc, expect)
    # a payload cut short fails for sure: the index gives the block fewer bytes than its symbols need
    enc = object.__new__(Enc)
    enc.__dict__.update(clean.__dict__)
    offs = clean.offsets.clone()
    cut = int(clean.h_offs[6]) - (int(clean.h_offs[6]) - int(clean.h_offs[5])) // 2
    st = torch.cat([clean.stream[:cut], clean.stream[int(clean.h_offs[6]):]])
    offs[6:] -= int(clean.h_offs[6]) - cut
    enc.stream, enc.offsets, enc.length, enc.h_offs = st, offs, int(st.numel()), offs.cpu().numpy().astype(np.int64)
    expect = decode_block(codec, torch, enc, 5, relaxed=True)
    assert expect != HUFE_OK
    r = update(torch, codec, enc, ranges, patches, relaxed=True)
    assert r.rc == expect
    # the same block untouched or direct: no error
    r = update(torch, codec, enc, [(10, 20)], random_patches([(10, 20)], 1), relaxed=True)
    assert r.rc == HUFE_OK and r.count == 1
    r = update(torch, codec, enc, [(5 * bs, 6 * bs)], random_patches([(5 * bs, 6 * bs)], 1), relaxed=True)
    assert r.rc == HUFE_OK and r.count == 1
    check = update(torch, codec, clean, [(5 * bs, 6 * bs)], random_patches([(5 * bs, 6 * bs)], 1), relaxed=True)
    assert np.array_equal(r.stream, check.stream)


@pytest.mark.parametrize("relaxed", [False, True], ids=["strict", "relaxed"])
def test_a_header_that_does_not_parse(torch_mod, codec, oracle, relaxed):
    torch = torch_mod
    bs = 4 * KIB
    n = 10 * bs + 5
    data = make("zipf255", n)
    clean = Enc(torch, codec, data, bs)
    bad_b = 6
    enc = object.__new__(Enc)
    enc.__dict__.update(clean.__dict__)
    st = clean.stream.clone()
    o = int(clean.h_offs[bad_b])
    st[o + 8] = 0xFF                                    # tree_len = 0x7fff: no tree is that long
    st[o + 9] = 0x7F
    enc.stream = st
    header_err = decode_block(codec, torch, enc, bad_b, relaxed)
    assert header_err != HUFE_OK

    # in front of the bad block: served; the bad record and everything behind it is carried over
    ranges = [(bs + 5, 3 * bs + 7), (5 * bs, 6 * bs)]
    patches = random_patches(ranges, 5)
    r = update(torch, codec, enc, ranges, patches, relaxed=relaxed)
    want = update(torch, codec, clean, ranges, patches, relaxed=relaxed)
    check_equals_encode(torch, codec, oracle, clean, ranges, patches, want, "clean")
    assert r.rc == HUFE_OK and r.count == want.count == 4 and r.length == want.length
    assert np.array_equal(r.index, want.index)
    diff = np.flatnonzero(r.stream != want.stream)
    assert set(diff.tolist()) <= {int(r.index[bad_b]) + 8, int(r.index[bad_b]) + 9}

    # inside the range, and behind it: that header's error
    for ranges in ([(5 * bs + 1, 7 * bs)], [(6 * bs, 6 * bs + 1)], [(8 * bs, 8 * bs + 10)], [(0, 5), (9 * bs, n)]):
        r = update(torch, codec, enc, ranges, random_patches(ranges, 5), relaxed=relaxed)
        assert r.rc == header_err, (ranges, r.rc, header_err)
    # the clean stream: a range past the end of the data is an argument error, an empty one there is ignored
    for ranges in ([(n - 1, n + 1)], [(n, n + 1)], [(n + 5, n + 9)], [(0, 3), (n - 3, n + 3)]):
        r = update(torch, codec, clean, ranges, random_patches(ranges, 5), relaxed=relaxed)
        assert r.rc == HUFE_ARGUMENT, ranges
    r = update(torch, codec, clean, [(n + 5, n + 5), (1, 2)], random_patches([(5, 5), (1, 2)], 5), relaxed=relaxed)
    assert r.rc == HUFE_OK and r.count == 1


def test_a_batch_stream(torch_mod, codec, oracle):
    """ragged blocks: the items' short last blocks lie in the middle of the stream"""
    torch = torch_mod
    bs = 4 * KIB
    item_lens = [3 * bs + 17, 1, 2 * bs, 5, bs - 1, 4 * bs + 4000]
    data = make("logtext", sum(item_lens))
    batch = codec.encode_batch(dev(torch, data), item_lens, bs, sub_index=True)
    block_lens = []
    for ln in item_lens:
        block_lens += [min(bs, ln - o) for o in range(0, ln, bs)]
    enc = Enc(torch, codec, data, bs, stream=batch.stream, offsets=batch.offsets, block_lens=block_lens)
    assert enc.nb == batch.nblocks
    P = enc.P
    ranges = [(int(P[3]) - 9, int(P[5]) + 3), (int(P[8]), int(P[9])), (int(P[-1]) - 1, int(P[-1])), (2, 9), (11, 12)]
    patches = random_patches(ranges, 21)
    layout = (enc.nb * batch.row_blocksize, batch.row_blocksize)
    r = update(torch, codec, enc, ranges, patches, scatter_seed=4, old_sub=batch.sub_index, want_sub=True, layout=layout)
    assert r.rc == HUFE_OK, codec.lib.hufgpu_last_error(codec._ctx).decode()
    assert r.count == int(touched_blocks(P, ranges).sum())
    new = patched(data, ranges, patches)
    want = codec.encode_batch(dev(torch, new), item_lens, bs, sub_index=True)
    assert r.length == want.stream_len and np.array_equal(r.stream, want.stream.cpu().numpy())
    assert np.array_equal(r.index.astype(np.int64), want.offsets.cpu().numpy())
    # block by block the oracle's encode of the block's bytes
    for b in range(enc.nb):
        rec = oracle.encode(new[int(P[b]):int(P[b + 1])], 0)
        assert np.array_equal(r.stream[int(r.index[b]):int(r.index[b + 1])], rec), b
    # the new batch sub-index decodes the new stream
    nb2 = object.__new__(type(batch))
    nb2.__dict__.update(batch.__dict__)
    nb2.stream, nb2.offsets, nb2.sub_index = r.d_stream, r.d_index, r.sub
    nb2.item_offsets = [int(r.index[k]) for k in batch.item_blocks]
    out, errs, raws = codec.decode_batch(nb2, relaxed=True)          # (the random patch gave a block all 256 values)
    assert errs == [0] * len(item_lens) and raws == item_lens
    assert np.array_equal(out.cpu().numpy()[:new.size], new)
    assert codec.decode_counters()[0] == 0


def test_a_reference_written_stream(torch_mod, codec, oracle, reference):
    """untouched records stay the reference's, touched ones become this encoder's: the same bits"""
    torch = torch_mod
    bs = 64 * KIB
    n = 5 * bs + 321
    data = make("zipf255", n)
    ref_stream = reference.encode(data, bs)
    length = int(ref_stream.size)
    raw = torch.zeros(length + 64, dtype=torch.uint8, device="cuda")
    raw[:length] = dev(torch, ref_stream)
    d_index, nb, used = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    lib = codec.lib
    rc = lib.hufgpu_block_index(codec._ctx, C.c_void_p(raw.data_ptr()), C.c_uint64(length), C.c_uint64(length), C.c_uint32(0),
                                C.byref(d_index), C.byref(nb), C.byref(used), None)
    assert rc == 0 and nb.value == codec.block_count(n, bs) and used.value == length
    index = torch.empty(nb.value + 1, dtype=torch.int64, device="cuda")
    assert lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(index.data_ptr()), d_index, C.c_uint64(8 * (nb.value + 1))) == 0
    enc = Enc(torch, codec, data, bs, stream=raw[:length], offsets=index, block_lens=[min(bs, n - b * bs) for b in range(nb.value)])
    ranges = [(bs + 1, 2 * bs + 5), (4 * bs, 5 * bs), (n - 3, n - 1)]
    patches = random_patches(ranges, 9)
    r = update(torch, codec, enc, ranges, patches)
    new, want, _ = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r, "reference stream")
    assert np.array_equal(reference.encode(new, bs), r.stream)


def test_out_cap_one_byte_short(torch_mod, codec, oracle):
    torch = torch_mod
    bs = 4 * KIB
    n = 9 * bs + 10
    enc = Enc(torch, codec, make("logtext", n), bs)
    ranges = [(bs + 3, 3 * bs + 9), (5 * bs, 6 * bs)]
    patches = random_patches(ranges, 2)
    full = update(torch, codec, enc, ranges, patches)
    check_equals_encode(torch, codec, oracle, enc, ranges, patches, full, "roomy")
    exact = update(torch, codec, enc, ranges, patches, out_cap=full.length)
    assert exact.rc == HUFE_OK and np.array_equal(exact.stream, full.stream)
    short = update(torch, codec, enc, ranges, patches, out_cap=full.length - 1)
    assert short.rc == HUFE_MEMORY
    assert np.all(short.out_all == GUARD)                # a stream that does not fit is not written at all
    r = update(torch, codec, enc, [], [], out_cap=enc.length - 1)
    assert r.rc == HUFE_MEMORY


def test_relaxed_trees_and_interleaved_calls(torch_mod, codec, oracle):
    """strict and relaxed flags give the same result on the encoder's streams; decodes of the same context in between"""
    torch = torch_mod
    bs = 64 * KIB
    n = 4 * bs + 100
    data = make("zipf255", n)
    enc = Enc(torch, codec, data, bs)
    ranges = [(100, bs + 100), (3 * bs - 1, 3 * bs + 1)]
    patches = random_patches(ranges, 3)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    r1 = update(torch, codec, enc, ranges, patches)
    assert codec.decode(enc.stream, enc.length, enc.offsets, enc.nb, out) == n and np.array_equal(out.cpu().numpy(), data)
    r2 = update(torch, codec, enc, ranges, patches, relaxed=True)
    got = codec.decode_range(enc.stream, enc.length, enc.offsets, enc.nb, 50, 2 * bs + 50)
    assert np.array_equal(got.cpu().numpy(), data[50:2 * bs + 50])
    r3 = update(torch, codec, enc, ranges, patches)
    new, _, _ = check_equals_encode(torch, codec, oracle, enc, ranges, patches, r1, "first")
    for r in (r2, r3):
        assert r.rc == HUFE_OK and np.array_equal(r.stream, r1.stream) and np.array_equal(r.index, r1.index)
    # the Python layer: update_ranges and update_range
    st, length, offs, sub, count = codec.update_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges,
                                                       dev(torch, np.concatenate(patches)), blocksize=bs)
    assert length == r1.length and count == r1.count and sub is None and np.array_equal(st.cpu().numpy(), r1.stream)
    # (block 1 is now 64 KiB of random bytes: all 256 values, the 1 025-entry tree that only the relaxed flag decodes)
    assert codec.decode(st, length, offs, enc.nb, out, relaxed=True) == n and np.array_equal(out.cpu().numpy(), new)
    st, length, offs, sub, count = codec.update_range(enc.stream, enc.length, enc.offsets, enc.nb, 100, dev(torch, patches[0]),
                                                      want_sub_index=True, raw_size=n, blocksize=bs)
    assert count == 2 and sub is not None
    assert codec.decode(st, length, offs, enc.nb, out, relaxed=True) == n
    assert codec.decode(st, length, offs, enc.nb, out, relaxed=True, sub_index=sub, raw_size=n, blocksize=bs) == n
    assert np.array_equal(out.cpu().numpy(), patched(data, ranges[:1], patches[:1]))

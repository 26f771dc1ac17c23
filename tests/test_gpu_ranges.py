"""GPU tests of hufgpu_decode_ranges (GpuCodec.decode_ranges / decode_range): byte ranges of the original data out of
one indexed stream.

Bit-exact, no tolerance: the expected bytes of a range are a slice of the original input; expected errors and delivered
counts come from the oracle decoding the records of the touched blocks, with hufgpu_decode of the same block sub-range
as a second witness.  Every output buffer is filled with 0xA5 first: the bytes between and behind the slots and in the
spare room of every slot must still hold it.
"""
import ctypes as C

import numpy as np
import pytest

import sub_index_ref as sref
from libhuffman_amd import datagen
from stream_support import GUARD, Enc, dev, touched

pytestmark = pytest.mark.gpu

HUFE_OK, HUFE_MEMORY, HUFE_OVERFLOW = 0, 1, 5
TREE_STRICT, TREE_MAX = 1024, 1025


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


def slots_for(ranges, n, gaps=(13, 0, 7, 1, 16, 3), lead=5, shrink=None):
    """slot i holds range i cut at n, plus a few spare bytes that vary (odd slot addresses); shrink: {i: bytes less}"""
    oo = [lead]
    for i, (lo, hi) in enumerate(ranges):
        need = min(hi, n) - min(lo, n)
        size = need + gaps[i % len(gaps)]
        if shrink and i in shrink:
            size = need - shrink[i]
        oo.append(oo[-1] + size)
    return oo


def run(torch, codec, enc, ranges, oo=None, relaxed=False, use_sub=True, sub_index=None):
    oo = slots_for(ranges, enc.n) if oo is None else oo
    out = torch.full((oo[-1] + 9,), GUARD, dtype=torch.uint8, device="cuda")
    kw = enc.sub_args() if use_sub else {}
    if sub_index is not None:
        kw = dict(sub_index=sub_index, raw_size=enc.n, blocksize=enc.bs)
    _, errs, raws = codec.decode_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges, out=out, out_offsets=oo,
                                        relaxed=relaxed, **kw)
    return out.cpu().numpy(), errs, raws, oo


def check_all_good(enc, ranges, got, errs, raws, oo, only=None):
    """every range (or those in `only`) succeeded with its slice; nothing else in the buffer was written when all are checked"""
    want = np.full(got.size, GUARD, np.uint8)
    idx = range(len(ranges)) if only is None else only
    for i in idx:
        lo, hi = ranges[i]
        lo_c, hi_c = min(lo, enc.n), min(hi, enc.n)
        assert (errs[i], raws[i]) == (0, hi_c - lo_c), f"range {i} {ranges[i]}: ({errs[i]}, {raws[i]})"
        want[oo[i]:oo[i] + hi_c - lo_c] = enc.data[lo_c:hi_c]
        if only is not None:
            assert np.array_equal(got[oo[i]:oo[i + 1]], want[oo[i]:oo[i + 1]]), f"range {i} {ranges[i]}: slot bytes"
    if only is None:
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, f"bytes differ at {diff[:8]} (slots start at {oo[:8]})"
    assert np.all(got[:oo[0]] == GUARD) and np.all(got[oo[-1]:] == GUARD)


def witnesses(torch, codec, oracle, enc, fb, lb, relaxed=False):
    """(err, bytes) of the blocks fb .. lb decoded on their own: by the oracle from their records, and by hufgpu_decode"""
    room = int(enc.P[lb + 1] - enc.P[fb])
    # record by record, as the index cuts them (a damaged payload moves the end of its block in a raw stream; the index keeps it)
    st = enc.stream[enc.h_offs[fb]:enc.h_offs[lb + 1]].cpu().numpy()
    oerr, parts = 0, []
    for b in range(fb, lb + 1):
        rec = st[enc.h_offs[b] - enc.h_offs[fb]:enc.h_offs[b + 1] - enc.h_offs[fb]]
        oerr, part, _ = oracle.decode(rec, int(enc.P[b + 1] - enc.P[b]), TREE_MAX if relaxed else TREE_STRICT)
        parts.append(part)
        if oerr:
            break
    oout = np.concatenate(parts)
    out = torch.full((room,), GUARD, dtype=torch.uint8, device="cuda")
    raw = C.c_uint64(0)
    offs = enc.offsets[fb:lb + 2].contiguous()
    gerr = codec.lib.hufgpu_decode(codec._ctx, enc.stream.data_ptr(), enc.length, offs.data_ptr(), lb - fb + 1,
                                   out.data_ptr(), room, 1 if relaxed else 0, C.byref(raw), None)
    return (int(oerr), oout), (int(gerr), out.cpu().numpy()[:int(raw.value)])


def check_failing(torch, codec, oracle, enc, ranges, got, errs, raws, oo, i, relaxed=False):
    lo, hi = ranges[i]
    fb, lb = touched(enc, lo, hi)
    (oerr, oout), (gerr, gout) = witnesses(torch, codec, oracle, enc, fb, lb, relaxed)
    assert oerr != 0 and oerr == gerr and oout.size == gout.size and np.array_equal(oout, gout), "the witnesses disagree"
    p0 = int(enc.P[fb])
    lo_c, hi_c = min(lo, enc.n), min(hi, enc.n)
    delivered = max(0, min(hi_c, p0 + oout.size) - lo_c)
    assert (errs[i], raws[i]) == (oerr, delivered), f"range {i} {ranges[i]}: ({errs[i]}, {raws[i]}) != ({oerr}, {delivered})"
    assert np.array_equal(got[oo[i]:oo[i] + delivered], oout[lo_c - p0:lo_c - p0 + delivered]), f"range {i}: delivered bytes"
    assert np.all(got[oo[i] + (hi_c - lo_c):oo[i + 1]] == GUARD), f"range {i}: spare room written"


def make(kind, n, seed=3):
    return datagen.zipf255(n, seed=seed) if kind == "zipf255" else datagen.logtext(n)


def fixed_ranges(bs, n):
    r = [(bs + 17, bs + 900), (bs, 2 * bs), (0, bs), (bs - 333, 2 * bs), (bs // 2 + 1, bs + bs // 2), (3, n - 5), (0, n),
         (0, 0), (bs // 3, bs // 3), (bs, bs), (n, n), (n - 101, n + 1000), (n, n + 50), (n + 10, n + 20), (1, 2),
         (n - 1, n), (2 * bs - 1, 2 * bs + 1)]
    if n > 3 * bs + 1:
        r += [(bs - 1, 3 * bs + 1), (bs + 1, 4 * bs - 1 if n >= 4 * bs else n)]
    return r


CASES = [(4096, 40 * 4096 + 123), (65536, 9 * 65536 + 777), (1 << 20, (3 << 20) + 4567), (1 << 21, (2 << 21) + 99999)]


@pytest.mark.parametrize("kind", ["zipf255", "logtext"])
@pytest.mark.parametrize("bs,n", CASES, ids=[f"bs{c[0]}" for c in CASES])
def test_fixed_ranges(torch_mod, codec, kind, bs, n):
    enc = Enc(torch_mod, codec, make(kind, n), bs)
    ranges = fixed_ranges(bs, n)
    got, errs, raws, oo = run(torch_mod, codec, enc, ranges)
    check_all_good(enc, ranges, got, errs, raws, oo)
    # one range per call, and the convenience call
    for lo, hi in ((bs + 17, bs + 900), (0, n), (n - 101, n + 1000)):
        got, errs, raws, oo = run(torch_mod, codec, enc, [(lo, hi)])
        check_all_good(enc, [(lo, hi)], got, errs, raws, oo)
        one = codec.decode_range(enc.stream, enc.length, enc.offsets, enc.nb, lo, hi)
        assert np.array_equal(one.cpu().numpy(), enc.data[lo:min(hi, n)])


def random_ranges(rng, n, bs, count):
    ranges = []
    for _ in range(count):
        lo = int(rng.integers(0, n + 10))
        span = int(rng.choice([0, 1, 17, bs // 2, bs, bs + 1, 3 * bs + 5])) + int(rng.integers(0, 64))
        ranges.append((lo, lo + int(rng.integers(0, span + 1))))
    ranges += ranges[:20] + [(0, n), (0, n)]            # repeats, and the whole twice
    order = rng.permutation(len(ranges))
    return [ranges[int(j)] for j in order]


@pytest.mark.parametrize("bs,n", [(4096, 64 * 4096 + 1001), (65536, 20 * 65536 + 31)], ids=["bs4096", "bs65536"])
def test_hundreds_of_random_ranges(torch_mod, codec, bs, n):
    rng = np.random.default_rng(bs)
    enc = Enc(torch_mod, codec, make("zipf255", n, seed=9), bs)
    ranges = random_ranges(rng, n, bs, 400)
    got, errs, raws, oo = run(torch_mod, codec, enc, ranges)
    check_all_good(enc, ranges, got, errs, raws, oo)


@pytest.mark.parametrize("bs,n", [(4096, 64 * 4096 + 1001), (65536, 20 * 65536 + 31)], ids=["bs4096", "bs65536"])
def test_sub_index_good_and_bad(torch_mod, codec, bs, n):
    torch = torch_mod
    rng = np.random.default_rng(bs + 1)
    enc = Enc(torch, codec, make("zipf255", n, seed=10), bs, sub=True)
    other = Enc(torch, codec, make("logtext", n), bs, sub=True)
    ranges = random_ranges(rng, n, bs, 300)
    ref = run(torch, codec, enc, ranges, use_sub=False)
    check_all_good(enc, ranges, *ref)
    got = run(torch, codec, enc, ranges)
    check_all_good(enc, ranges, *got)
    bad = {"zeros": torch.zeros_like(enc.sub),
           "random": torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda(),
           "stale": other.sub.clone()}
    for name, sub in bad.items():
        got = run(torch, codec, enc, ranges, sub_index=sub)
        assert got[1:3] == ref[1:3] and np.array_equal(got[0], ref[0]), name
        assert codec.decode_counters()[0] > 0, f"{name}: no block went to the exact decoder"


def flip_payload(torch, enc, k, byte=40, xor=0x10):
    bo = int(enc.h_offs[k])
    tl = int.from_bytes(bytes(enc.stream[bo + 8:bo + 10].cpu().numpy()), "little")
    st = enc.stream.clone()
    st[bo + 10 + 2 * tl + byte] ^= xor
    return enc.with_stream(st)


def test_untouched_blocks_are_not_decoded(torch_mod, codec, oracle):
    from libhuffman_amd.codec import HuffmanGpuError
    torch = torch_mod
    bs, k = 4096, 5
    n = 12 * bs + 321
    good = Enc(torch, codec, make("zipf255", n, seed=21), bs, sub=True)
    bad = flip_payload(torch, good, k)
    with pytest.raises(HuffmanGpuError):
        codec.decode(bad.stream, bad.length, bad.offsets, bad.nb, torch.empty(n, dtype=torch.uint8, device="cuda"))
    p = int(bad.P[k])
    ranges = [(0, p), (p + bs, n), (17, 3 * bs + 1), (p - 1, p), (p + bs, p + bs + 1), (p + bs + 5, n + 7), (0, 0),
              (p + 100, p + 200), (p - bs - 7, p + bs + 9), (p + bs - 1, p + 2 * bs), (0, n), (p - 50, p + 3)]
    fine, failing = [0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11]
    for use_sub in (False, True):
        got, errs, raws, oo = run(torch, codec, bad, ranges, use_sub=use_sub)
        check_all_good(bad, ranges, got, errs, raws, oo, only=fine)
        for i in failing:
            check_failing(torch, codec, oracle, bad, ranges, got, errs, raws, oo, i)
        assert errs[11] != 0
        errs11, raw11 = errs[11], raws[11]
    # ranges that do not touch the block: the call as a whole succeeds
    clean = [ranges[i] for i in fine]
    got, errs, raws, oo = run(torch, codec, bad, clean)
    check_all_good(bad, clean, got, errs, raws, oo)
    with pytest.raises(HuffmanGpuError) as e:
        codec.decode_range(bad.stream, bad.length, bad.offsets, bad.nb, p - 50, p + 3)
    assert e.value.err == errs11 and e.value.raw == raw11


@pytest.mark.parametrize("tree_len", [1025, 0xFFFF], ids=["tree_len_1025", "tree_len_negative"])
def test_header_damage(torch_mod, codec, tree_len):
    torch = torch_mod
    bs, k = 4096, 6
    n = 11 * bs + 77
    good = Enc(torch, codec, make("logtext", n), bs)
    st = good.stream.clone()
    bo = int(good.h_offs[k])
    st[bo + 8] = tree_len & 0xFF
    st[bo + 9] = tree_len >> 8
    bad = good.with_stream(st)
    # what hufgpu_decode says to that block alone
    raw = C.c_uint64(0)
    offs = bad.offsets[k:k + 2].contiguous()
    tmp = torch.empty(bs, dtype=torch.uint8, device="cuda")
    herr = codec.lib.hufgpu_decode(codec._ctx, bad.stream.data_ptr(), bad.length, offs.data_ptr(), 1, tmp.data_ptr(), bs, 0,
                                   C.byref(raw), None)
    assert herr == HUFE_OVERFLOW and raw.value == 0
    p = int(bad.P[k])
    ranges = [(0, p), (p - 10, p), (5, 2 * bs + 3), (p, p), (p, p + 1), (p - 100, p + 100), (p + bs, p + 2 * bs), (0, n),
              (n, n + 5), (p + 5, p + 5)]
    got, errs, raws, oo = run(torch, codec, bad, ranges)
    check_all_good(bad, ranges, got, errs, raws, oo, only=[0, 1, 2, 3])
    for i in range(4, len(ranges)):
        lo, hi = ranges[i]
        delivered = max(0, p - lo)
        assert (errs[i], raws[i]) == (herr, delivered), f"range {i} {ranges[i]}: ({errs[i]}, {raws[i]})"
        assert np.array_equal(got[oo[i]:oo[i] + delivered], bad.data[lo:lo + delivered])
        assert np.all(got[oo[i] + delivered:oo[i + 1]] == GUARD), f"range {i}: bytes behind the delivered ones written"


def test_a_slot_one_byte_short(torch_mod, codec):
    torch = torch_mod
    bs = 4096
    n = 9 * bs + 5
    enc = Enc(torch, codec, make("zipf255", n, seed=33), bs)
    ranges = [(10, bs + 10), (bs, 3 * bs), (2 * bs + 1, 2 * bs + 700), (0, n), (5 * bs, 5 * bs + 1)]
    for short in (1, 2, 4):
        oo = slots_for(ranges, n, shrink={short: 1})
        got, errs, raws, _ = run(torch, codec, enc, ranges, oo=oo)
        assert (errs[short], raws[short]) == (HUFE_MEMORY, 0)
        assert np.all(got[oo[short]:oo[short + 1]] == GUARD), "the short slot was written"
        check_all_good(enc, ranges, got, errs, raws, oo, only=[i for i in range(len(ranges)) if i != short])


def test_batch_stream(torch_mod, codec):
    torch = torch_mod
    bs = 4096
    lens = [5000, 0, 70000, 3, 65536 + 17, 12345, 4096]
    items = [datagen.zipf255(x, seed=50 + i) if x else np.zeros(0, np.uint8) for i, x in enumerate(lens)]
    data = np.concatenate(items)
    batch = codec.encode_batch(dev(torch, data), lens, bs, sub_index=True)
    block_lens = [min(bs, x - o) for x in lens for o in range(0, x, bs)]
    assert len(block_lens) == batch.nblocks
    enc = Enc(torch, codec, data, bs, stream=batch.stream, offsets=batch.offsets, block_lens=block_lens)
    cut = np.concatenate([[0], np.cumsum(lens)])
    ranges = [(0, enc.n), (4990, 5010), (int(cut[2]), int(cut[3])), (int(cut[3]) - 1, int(cut[4]) + 1), (4096, 5000),
              (5000, 5000 + 4096), (int(cut[5]) - 3000, int(cut[6]) + 2), (enc.n - 1, enc.n + 9), (903, 4097)]
    ranges += random_ranges(np.random.default_rng(4), enc.n, bs, 100)
    got, errs, raws, oo = run(torch, codec, enc, ranges)
    check_all_good(enc, ranges, got, errs, raws, oo)
    # the batch's sub-index: nblocks rows of row_blocksize symbols = the layout of (nblocks * row_blocksize, row_blocksize)
    oo = slots_for(ranges, enc.n)
    out = torch.full((oo[-1] + 9,), GUARD, dtype=torch.uint8, device="cuda")
    _, errs, raws = codec.decode_ranges(enc.stream, enc.length, enc.offsets, enc.nb, ranges, out=out, out_offsets=oo,
                                        sub_index=batch.sub_index, raw_size=batch.nblocks * batch.row_blocksize,
                                        blocksize=batch.row_blocksize)
    check_all_good(enc, ranges, out.cpu().numpy(), errs, raws, oo)


def test_foreign_index(torch_mod, codec):
    torch = torch_mod
    bs = 16384
    n = 13 * bs + 4001
    data = make("logtext", n)
    stream, _, length = codec.encode(dev(torch, data), bs)
    raw = torch.zeros(length + 64, dtype=torch.uint8, device="cuda")          # (torch allocations are 16-byte aligned)
    raw[:length] = stream
    d_index, nb, used = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    lib = codec.lib
    rc = lib.hufgpu_block_index(codec._ctx, C.c_void_p(raw.data_ptr()), C.c_uint64(length), C.c_uint64(length), C.c_uint32(0),
                                C.byref(d_index), C.byref(nb), C.byref(used), None)
    assert rc == 0 and nb.value == codec.block_count(n, bs) and used.value == length
    index = torch.empty(nb.value + 1, dtype=torch.int64, device="cuda")      # the context's array lives until its next decode
    assert lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(index.data_ptr()), d_index, C.c_uint64(8 * (nb.value + 1))) == 0
    block_lens = [min(bs, n - b * bs) for b in range(nb.value)]
    enc = Enc(torch, codec, data, bs, stream=raw[:length], offsets=index, block_lens=block_lens)
    ranges = fixed_ranges(bs, n) + random_ranges(np.random.default_rng(8), n, bs, 60)
    got, errs, raws, oo = run(torch, codec, enc, ranges)
    check_all_good(enc, ranges, got, errs, raws, oo)


def test_relaxed_and_strict_trees(torch_mod, codec, oracle):
    torch = torch_mod
    bs = 8192
    rng = np.random.default_rng(77)
    data = np.concatenate([datagen.zipf255(2 * bs, seed=1), sref.all_values(rng, bs), datagen.zipf255(2 * bs + 99, seed=2)])
    enc = Enc(torch, codec, data, bs)
    p = 2 * bs
    ranges = [(0, p), (p + 10, p + 20), (p - 5, p + bs + 5), (p + bs, enc.n), (0, enc.n)]
    got, errs, raws, oo = run(torch, codec, enc, ranges, relaxed=True)
    check_all_good(enc, ranges, got, errs, raws, oo)
    got, errs, raws, oo = run(torch, codec, enc, ranges)
    # (the block fails in its header: behind it positions are not known, so the range behind it fails as well)
    check_all_good(enc, ranges, got, errs, raws, oo, only=[0])
    for i in (1, 2, 3, 4):
        lo, hi = ranges[i]
        delivered = max(0, p - lo)
        assert (errs[i], raws[i]) == (HUFE_OVERFLOW, delivered)
        assert np.array_equal(got[oo[i]:oo[i] + delivered], data[lo:lo + delivered])
    # the oracle on the all-values block alone: the same error in strict mode, none in relaxed mode
    (oerr, _), (gerr, _) = witnesses(torch, codec, oracle, enc, 2, 2)
    assert oerr == gerr == HUFE_OVERFLOW
    (oerr, oout), _ = witnesses(torch, codec, oracle, enc, 2, 2, relaxed=True)
    assert oerr == 0 and np.array_equal(oout, data[p:p + bs])


def test_workspaces_do_not_leak_between_calls(torch_mod, codec):
    torch = torch_mod
    a = Enc(torch, codec, make("zipf255", 30 * 4096 + 11, seed=91), 4096, sub=True)
    b = Enc(torch, codec, make("logtext", 7 * 65536 + 5), 65536)
    ra = random_ranges(np.random.default_rng(1), a.n, a.bs, 80)
    rb = [(65536 + 5, 3 * 65536 - 9), (0, 10)]
    got, errs, raws, oo = run(torch, codec, a, ra)
    check_all_good(a, ra, got, errs, raws, oo)
    out = torch.full((b.n + 3,), GUARD, dtype=torch.uint8, device="cuda")
    assert codec.decode(b.stream, b.length, b.offsets, b.nb, out) == b.n        # every block again: nothing stays switched off
    assert np.array_equal(out.cpu().numpy()[:b.n], b.data) and np.all(out.cpu().numpy()[b.n:] == GUARD)
    got, errs, raws, oo = run(torch, codec, b, rb)
    check_all_good(b, rb, got, errs, raws, oo)
    out.fill_(GUARD)
    assert codec.decode(a.stream, a.length, a.offsets, a.nb, out[:a.n], **a.sub_args()) == a.n
    assert np.array_equal(out.cpu().numpy()[:a.n], a.data)
    got, errs, raws, oo = run(torch, codec, a, ra[:5])
    check_all_good(a, ra[:5], got, errs, raws, oo)

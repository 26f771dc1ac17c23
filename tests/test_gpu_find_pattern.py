"""GPU tests of hufgpu_find_pattern (GpuCodec.find_pattern / count_pattern): where a pattern of 1 to 64 bytes starts in
the original data, straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the model of tests/find_pattern_model.py (itself checked against a
bytes.find loop in tests/test_find_pattern_args.py).  As in tests/test_gpu_find.py the position buffer has guard words in
front and behind and is filled with the guard first: the words beyond totals[1] must still hold it.  Inputs are zipf-like
bytes with the pattern planted at chosen offsets - the smallest shapes that reach each seam (lane, tile, chunk, block, the
256-tile scan group, the end of the data); after planting the model's count is seen to be neither 0 nor everything.
"""
import functools

import numpy as np
import pytest

from find_model import find_model
from find_pattern_model import find_pattern_model
from find_support import (CHUNK, GUARD64, LEAD, OK, RW, TAIL, TILE, as_is, check, codec, damaged, encode, exact_positions, mixed_blocks,
                          pattern_upto_255, payload_start, planted, positions_exact_or_not_served, psearch, torch_mod)
from libhuffman_amd import datagen
from stream_support import make, max_code_len

pytestmark = pytest.mark.gpu

exact = functools.partial(exact_positions, find_pattern_model, as_is)
exact_or_not_served = functools.partial(positions_exact_or_not_served, find_pattern_model, as_is)


# ---- case 1: lane, tile and block seams; the two ends of the data --------------------------------------------------------
@pytest.mark.parametrize("length", [2, 5, 33, 64])
def test_seams_of_blocks_of_4099_bytes(torch_mod, codec, length):
    """five blocks of 4 099 bytes = tiles of 2 048, 2 048 and 3 symbols; no block start but the first is 32-aligned"""
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(length, length)
    # in the block: the data's first byte, the middle of a tile, the tile seam | a lane seam, through the 3-byte tile into
    # the next block | the same from the 3-byte tile's first byte, two tiles | from the block's last byte, the tile seam
    starts = [0, 1000, 2047, bs + 31, bs + 2 * TILE - 10, 2 * bs + 2000, 2 * bs + 4096, 3 * bs + 2047, 3 * bs + 4098]
    base = datagen.zipf255(n, seed=21)
    ends_with_it = planted(base, pat, starts + [n - length])
    one_short = planted(base, pat, starts + [n - length + 1])           # ... would end one byte past the data
    enc = encode(torch_mod, codec, ends_with_it, bs)
    exact(torch_mod, codec, enc, pat, must=starts + [n - length], what=("ends with it", length))
    enc = encode(torch_mod, codec, one_short, bs)
    exact(torch_mod, codec, enc, pat, must=starts, must_not=[n - length + 1, n - length], what=("one short", length))


# ---- case 2: blocks of 64 bytes, across the scan group of 256 tiles --------------------------------------------------------
def test_blocks_of_64_bytes(torch_mod, codec):
    bs, nb = 64, 300
    n = (nb - 1) * bs + 21
    base = datagen.zipf255(n, seed=22)
    p64, p33 = pattern_upto_255(64, 64), pattern_upto_255(33, 33)
    # 64 bytes over two blocks, in exactly one block, over the blocks 255 | 256 of two scan groups
    s64 = [1, 5 * bs, 255 * bs + 1, 270 * bs + 63]
    # 33 bytes over every seam of three neighbouring blocks, and in front of the short last block
    s33 = [10 * bs + 40, 11 * bs + 50, 253 * bs + 60, 256 * bs + 32, (nb - 2) * bs + 50]
    data = planted(planted(base, p64, s64), p33, s33)
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, p64, must=s64, what="64 bytes")
    exact(torch_mod, codec, enc, p33, must=s33, what="33 bytes")
    exact(torch_mod, codec, enc, p33[:2], must=s33, what="2 bytes")


# ---- case 3: the smallest blocks -----------------------------------------------------------------------------------------
def test_blocks_of_3_bytes(torch_mod, codec):
    """Blocks of 3 bytes - encode_sub writes a sub-index the tile item accepts at this size, so none larger is needed: 200
    blocks, and a pattern of 64 bytes from offset 1 touches 22 of them, its bytes coming from 21 other tiles' heads."""
    bs, nb = 3, 200
    n = nb * bs - 1
    base = datagen.zipf255(n, seed=23)
    p64, p7 = pattern_upto_255(64, 3), pattern_upto_255(7, 7)
    s64 = [1, 100 * bs, n - 64]
    s7 = [70, 80 * bs + 2, 90 * bs + 1]
    data = planted(planted(base, p64, s64), p7, s7)
    data[150 * bs:153 * bs + 1] = 9                        # one-symbol blocks among them, and the value once more
    enc = encode(torch_mod, codec, data, bs)
    assert (s64[0] + 63) // bs - s64[0] // bs + 1 == 22
    exact(torch_mod, codec, enc, p64, must=s64, what="64 bytes")
    exact(torch_mod, codec, enc, p7, must=s7, what="7 bytes")
    exact(torch_mod, codec, enc, bytes([9] * 10), must=[150 * bs], must_not=[150 * bs + 1], what="a run of 10")
    exact(torch_mod, codec, enc, bytes([9] * 4), what="a run's 4")


# ---- case 4: one block of several chunks ---------------------------------------------------------------------------------
def test_chunk_seams_of_one_block(torch_mod, codec):
    n = 3 * CHUNK + 77
    base = datagen.zipf255(n, seed=24)
    p64, p5 = pattern_upto_255(64, 4), pattern_upto_255(5, 5)
    s64 = [CHUNK - 10, 2 * CHUNK - 63, 2 * CHUNK + 3 * TILE - 1, n - 64]
    s5 = [CHUNK - 70, 2 * CHUNK - 68, CHUNK + TILE - 4, 3 * CHUNK - 1]
    data = planted(planted(base, p64, s64), p5, s5)
    enc = encode(torch_mod, codec, data, 0)
    assert enc.nb == 1
    exact(torch_mod, codec, enc, p64, must=s64, what="64 bytes")
    exact(torch_mod, codec, enc, p5, must=s5, what="5 bytes")


# ---- case 5: overlapping matches, one-symbol blocks ------------------------------------------------------------------------
def test_a_run_of_one_value(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    want = find_pattern_model(enc.data, b")" * 7, bs, n + 3)
    assert np.array_equal(want[0], np.arange(n - 6)) and want[1].tolist() == [bs] * 4 + [bs - 6]
    res = psearch(torch, codec, enc, b")" * 7, n + 3)
    assert not res[2].any()
    check(res, want, n + 3, "seven")
    for pat in (b")" * 64, b")"):
        res = psearch(torch, codec, enc, pat, n)
        check(res, find_pattern_model(enc.data, pat, bs, n), n, len(pat))
    for pat in (b")" * 6 + b"(", b"(" + b")" * 6, b")))()))"):
        res = psearch(torch, codec, enc, pat, 4)
        assert not res[2].any()
        check(res, find_pattern_model(enc.data, pat, bs, 4), 4, pat)
        assert res[1].tolist() == [0, 0, 0, 0]


def test_a_run_inside_ordinary_blocks(torch_mod, codec):
    """the matcher's worst case: every start of a run is a candidate and is verified to the pattern's end"""
    bs, n = 4096, 3 * 4096 + 500
    data = datagen.zipf255(n, seed=25).copy()
    data[1000:9000] = 41
    enc = encode(torch_mod, codec, data, bs)
    for pat in (b")" * 7, b")" * 64, b")" * 63 + bytes([int(data[9000])])):
        exact(torch_mod, codec, enc, pat, what=len(pat))


@pytest.mark.parametrize("bs", [4096, 4099])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs):
    torch = torch_mod
    data = mixed_blocks(bs, 6, 26)
    out_of, into = b")" * 4 + pattern_upto_255(6, 1), pattern_upto_255(5, 2) + b")" * 3
    s_out, s_in = [bs - 4, 3 * bs - 4], [2 * bs - 5, 4 * bs - 5]
    data = planted(planted(data, out_of, s_out), into, s_in)
    data[5 * bs:5 * bs + 2] = 41                           # the last run goes on into the ordinary block behind it
    data[5 * bs + 2] = 40
    one_leaf = [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)]
    assert one_leaf == [True, False] * 3
    enc = encode(torch, codec, data, bs)
    exact(torch, codec, enc, out_of, must=s_out, what="out of a one-symbol block")
    exact(torch, codec, enc, into, must=s_in, what="into a one-symbol block")
    exact(torch, codec, enc, b")" * 7, must=[bs - 7, 2 * bs, 3 * bs - 7, 5 * bs - 7, 5 * bs - 5],
          must_not=[bs - 6, 2 * bs - 1, 5 * bs - 4], what="seven")
    exact(torch, codec, enc, b")" * 64, must=[bs - 64, 5 * bs - 62], must_not=[bs - 63, 5 * bs - 61], what="sixty-four")


def test_abab(torch_mod, codec):
    bs, n = 4099, 5 * 4099                                 # an odd block size: the blocks start with a and with b in turn
    data = np.frombuffer((b"ab" * (n // 2 + 1))[:n], np.uint8).copy()
    enc = encode(torch_mod, codec, data, bs)
    total, _ = exact(torch_mod, codec, enc, b"abab", what="abab")
    assert total == (n - 4) // 2 + 1
    exact(torch_mod, codec, enc, b"ba" * 32, what="ba x 32")


# ---- case 6: long codes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,longest", [("l2", 13), ("long", 19)])
def test_second_level_and_long_codes(torch_mod, codec, kind, longest):
    bs, n = CHUNK, 3 * CHUNK + 77
    data = make(kind, n, bs)
    pat = bytes(data[100:109])                             # nine bytes of the input: the codes stay what they are
    starts = [bs - 4, TILE - 8, 2 * bs + 31]
    enc = encode(torch_mod, codec, planted(data, pat, starts), bs)
    assert max_code_len(enc) >= longest
    exact(torch_mod, codec, enc, pat, must=starts + [100], what=kind)


# ---- case 7: one byte is find_bytes --------------------------------------------------------------------------------------
def test_one_byte_is_find_bytes(torch_mod, codec):
    torch = torch_mod
    for data, bs in ((datagen.zipf255(5 * 4099, seed=27), 4099), (mixed_blocks(4096, 5, 28), 4096)):
        enc = encode(torch, codec, data, bs)
        for v in (int(np.bincount(data).argmax()), 41, 255):
            want = find_model(data, [v], bs, enc.n)
            cap = int(want[2][0]) + 5
            buf = torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda")
            _, totals, errs, cnt = codec.find_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, bs, [v],
                                                    max_positions=cap, block_counts=True, out=buf[LEAD:LEAD + cap])
            res = psearch(torch, codec, enc, bytes([v]), cap)
            assert np.array_equal(res[0], buf.cpu().numpy()) and np.array_equal(res[1], totals.cpu().numpy())
            assert np.array_equal(res[2], errs.cpu().numpy()) and np.array_equal(res[3], cnt.cpu().numpy())
            check(res, find_model(data, [v], bs, cap), cap, v)


# ---- case 8: the cap -----------------------------------------------------------------------------------------------------
def test_caps(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(5, 8)
    starts = [0, 2047, bs - 2, 2 * bs + 4096, 3 * bs + 4098, n - 5]
    enc = encode(torch, codec, planted(datagen.zipf255(n, seed=29), pat, starts), bs)
    total = int(find_pattern_model(enc.data, pat, bs)[2][0])
    assert total == len(starts)
    for cap in (0, total, total - 1, 1, total + 100):
        for counts in (True, False):
            res = psearch(torch, codec, enc, pat, cap, counts=counts)        # (cap 0: d_pos is NULL)
            assert not res[2].any() and int(res[1][0]) == total
            check(res, find_pattern_model(enc.data, pat, bs, cap), cap, (cap, counts))
    totals, errs = codec.count_pattern(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, pat)
    assert totals.cpu().tolist() == [total, 0, 0, 0] and not errs.cpu().numpy().any()
    for bad in (b"", b"x" * 65):
        with pytest.raises(ValueError):
            codec.find_pattern(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, bad)


# ---- case 9: a block that is not served ----------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """two byte values have the codes 00 and 01: a 1 at an even payload bit leaves the tree.  A match is reported only
    when every block it touches is served: those inside block 1, into it and out of it are absent, all others present."""
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(30)
    base = (rng.integers(0, 2, n) * 200 + 7).astype(np.uint8)
    pat = bytes((rng.integers(0, 2, 33) * 200 + 7).astype(np.uint8))
    inside, into, out_of = [bs + 1000, bs + 2040], [bs - 10], [2 * bs - 1]
    others = [0, 500, bs - 43, 2 * bs + 40, 2 * bs + 2030, 3 * bs - 33, 4 * bs - 5, n - 33]
    enc = encode(torch, codec, planted(base, pat, inside + into + out_of + others), bs)
    exact(torch, codec, enc, pat, must=inside + into + out_of + others, what="undamaged")
    if damage == "a payload bit":
        bad = damaged(enc, payload_start(enc, 1) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
    else:
        bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    served = np.array([True, False, True, True, True])
    for p, cap in ((pat, 40), (pat[:3], n), (pat[:2], n)):
        want = find_pattern_model(enc.data, p, bs, cap, served=served)
        res = psearch(torch, codec, bad, p, cap)
        assert res[2].tolist() == [OK, RW, OK, OK, OK] and int(res[1][2]) == 1, (damage, res[2], res[1])
        check(res, want, cap, (damage, len(p)))
    found = set(find_pattern_model(enc.data, pat, bs, 40, served=served)[0].tolist())
    assert found == set(others)


# ---- case 10: any content of the sub-index -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["zipf", "mixed"])
def test_sub_index_abuse(torch_mod, codec, shape):
    torch = torch_mod
    bs = 4096
    pat = pattern_upto_255(6, 10)
    if shape == "zipf":
        data = planted(datagen.zipf255(5 * bs + 1500, seed=31), pat, [100, bs - 3, 2 * bs + 2045, 5 * bs + 1494])
    else:
        data = planted(mixed_blocks(bs, 6, 32), b")))" + pat, [bs - 3, 3 * bs - 3, 3 * bs + 2040])
    enc = encode(torch, codec, data, bs)
    one_leaf = np.array([np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)])
    rng = np.random.default_rng(33)
    for p in (pat, b"))))", pat[:2]):
        cap = int(find_pattern_model(data, p, bs)[2][0]) + 3
        errs = exact_or_not_served(torch, codec, enc, p, cap, what="own")
        assert not errs.any()
        errs = exact_or_not_served(torch, codec, enc, p, cap, sub=torch.zeros_like(enc.sub), what="zeros")
        assert np.array_equal(errs != OK, ~one_leaf)      # (a bit count of 0 cannot be that of 32 codewords)
        random = torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
        errs = exact_or_not_served(torch, codec, enc, p, cap, sub=random, what="random")
        assert not errs[one_leaf].any()                   # (one-symbol blocks have no rows to be wrong)


# ---- case 11: one context, call after call ---------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """64 bytes, find_bytes, 2 bytes, 33 bytes on another stream's layout, without a synchronise in between: edges and mask
    bits of an earlier call must not show in a later one"""
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    p64 = pattern_upto_255(64, 11)
    a = encode(torch, codec, planted(datagen.zipf255(n, seed=34), p64, [5, 2047, bs - 1, 3 * bs + 4090]), bs)
    b = encode(torch, codec, planted(datagen.zipf255(3 * 64 + 9, seed=35), p64[:33], [40, 100]), 64)
    v = int(np.bincount(a.data).argmax())
    jobs = [(a, p64), (a, None), (a, p64[:2]), (b, p64[:33]), (a, p64[:3])]
    bufs = []
    for enc, p in jobs:
        want = find_pattern_model(enc.data, p, enc.bs, enc.n) if p else find_model(enc.data, [v], enc.bs, enc.n)
        cap = int(want[2][0]) + 2
        bufs.append((cap, torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda")))
    torch.cuda.synchronize()
    res = []
    for (enc, p), (cap, buf) in zip(jobs, bufs):
        args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
        kw = dict(max_positions=cap, block_counts=True, out=buf[LEAD:LEAD + cap])
        res.append(codec.find_pattern(*args, p, **kw) if p else codec.find_bytes(*args, [v], **kw))
    torch.cuda.synchronize()
    for (enc, p), (cap, buf), (_, totals, errs, cnt) in zip(jobs, bufs, res):
        want = find_pattern_model(enc.data, p, enc.bs, cap) if p else find_model(enc.data, [v], enc.bs, cap)
        assert int(want[2][0]) > 0
        check((buf.cpu().numpy(), totals.cpu().numpy(), errs.cpu().numpy(), cnt.cpu().numpy()), want, cap, p)


def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    pos, totals, errs, cnt = codec.find_pattern(empty, 0, offsets, 0, codec.new_sub_index(0, 4096), 0, 4096, b"ERROR",
                                                max_positions=4, block_counts=True, out=buf)
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    assert buf.cpu().tolist() == [GUARD64] * 4


# ---- case 12: the pipeline -----------------------------------------------------------------------------------------------
def test_grep_lines_with_error(torch_mod, codec):
    """find_bytes(newline) and find_pattern(ERROR) -> torch.searchsorted: the start of every match's line ->
    gather(max_len=128), with no host synchronisation before the comparison with what splitlines gives (the caps are
    host-known: a line has at least 40 bytes)"""
    torch = torch_mod
    n, bs = (1 << 20) + 1, 65536
    data = datagen.logtext(n)
    enc = encode(torch, codec, data, bs)
    cap = n // 40
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    nl, nl_totals, nl_errs, _ = codec.find_bytes(*args, b"\n", max_positions=cap)
    hit, hit_totals, hit_errs, _ = codec.find_pattern(*args, b"ERROR", max_positions=cap)
    slots = torch.arange(cap, device="cuda")
    nl = torch.where(slots < nl_totals[1], nl, n)                           # (behind the written ones: the end of the data)
    hit = torch.where(slots < hit_totals[1], hit, n)
    k = torch.searchsorted(nl, hit)                                         # newlines in front of the match
    starts = torch.where(k > 0, nl[(k - 1).clamp(min=0)] + 1, 0)
    starts = torch.where(hit < n, starts, n)                                # (past the end: a record of 0 bytes)
    rows, gerrs, raws = codec.gather(enc.stream, enc.length, enc.offsets, enc.nb, starts, 128, sub_index=enc.sub, raw_size=n,
                                     blocksize=bs)
    torch.cuda.synchronize()
    want = []                                                               # (line start, its first 128 bytes) per match
    at = 0
    for line in bytes(data).splitlines(keepends=True):
        want += [(at, (bytes(data[at:at + 128])))] * line.count(b"ERROR")
        at += len(line)
    assert 0 < len(want) <= cap
    assert nl_totals.cpu().tolist()[2:] == [0, 0] and hit_totals.cpu().tolist() == [len(want), len(want), 0, 0]
    assert not nl_errs.cpu().numpy().any() and not hit_errs.cpu().numpy().any()
    rows, gerrs, raws, starts = rows.cpu().numpy(), gerrs.cpu().numpy(), raws.cpu().numpy(), starts.cpu().numpy()
    assert not gerrs.any() and not raws[len(want):].any()
    assert starts[:len(want)].tolist() == [s for s, _ in want]
    for i, (s, first) in enumerate(want):
        assert raws[i] == len(first) and bytes(rows[i, :raws[i]]) == first, i

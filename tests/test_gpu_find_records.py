"""GPU tests of hufgpu_find_records (GpuCodec.find_records / count_records / grep): the records - the pieces of the
original data between delimiters - that hold a pattern, each once, as a start and a length, straight from stream, block
index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the model of tests/find_records_model.py (itself checked against a plain
loop over `bytes` in tests/test_find_records_args.py).  As in tests/test_gpu_find.py both output buffers have guard words in
front and behind and are filled with the guard first: the words beyond totals[1] must still hold it.  Inputs are zipf-like
bytes without the delimiter's value, with delimiters and the pattern planted at chosen offsets - the shapes of
tests/test_gpu_find_pattern.py, the smallest that reach each seam (lane, tile, chunk, block, the 256-tile scan group, the
end of the data).
"""
import functools

import numpy as np
import pytest

from find_model import find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from find_support import (CHUNK, GUARD32, GUARD64, LEAD, NL, OK, RW, TAIL, TILE, as_is, base_without, check, codec, damaged, encode,
                          exact_records, mixed_blocks, pattern_upto_255, payload_start, planted, records_exact_or_not_served, rsearch,
                          torch_mod, with_delimiters)
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu


# ---- checks --------------------------------------------------------------------------------------------------------------
exact = functools.partial(exact_records, find_records_model, as_is)
exact_or_not_served = functools.partial(records_exact_or_not_served, find_records_model, as_is)


def one_record(torch, codec, enc, pattern, what=""):
    """no delimiter in the data: the empty set and a value that never occurs both give ONE entry, (0, n)"""
    assert not (enc.data == NL).any()
    for delims in (b"", b"\n"):
        res = rsearch(torch, codec, enc, pattern, delims, 3)
        assert res[2].tolist() == [1, 1, 0, 0] and not res[3].any(), (what, delims, res[2])
        assert res[0][LEAD] == 0 and int(res[1].view(np.uint32)[LEAD]) == enc.n, (what, delims)
        check(res, find_records_model(enc.data, pattern, delims, enc.bs, 3), 3, (what, delims))
        assert res[4].tolist() == [1] + [0] * (enc.nb - 1)


# ---- case 1: lane, tile and block seams; the two ends of the data --------------------------------------------------------
@pytest.mark.parametrize("length", [1, 5, 64])
def test_seams_of_blocks_of_4099_bytes(torch_mod, codec, length):
    """five blocks of 4 099 bytes = tiles of 2 048, 2 048 and 3 symbols; no block start but the first is 32-aligned"""
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(length, 40 + length)
    base = base_without(n, 41)
    # delimiters: a lane seam's two sides, a tile seam's two sides, two in a row, a block's last and its first byte, a
    # 3-byte tile's last two bytes (one of them a block's last byte alone), another block's first byte alone
    nl = [31, 32, 300, 2047, 2048, 2500, 2501, 3000, bs - 1, bs, 2 * bs + 100, 2 * bs + 4097, 3 * bs - 1, 3 * bs + 1500,
          4 * bs, 4 * bs + 200]
    # matches: at byte 0 (a record without a delimiter in front) | right behind a delimiter and right in front of the next
    # (the record's first and last bytes) | across the tile seam at bs + 2048 and the block seam at 2 bs inside the record
    # (bs, 2 bs + 100) | in front of a delimiter in block 3 | behind block 4's first byte | in the last record, which no delimiter ends
    starts = [0, 301, 2047 - length, bs + 2048 - (length + 1) // 2, 2 * bs - (length + 1) // 2, 3 * bs + 1500 - length, 4 * bs + 1,
              n - length]
    data = planted(with_delimiters(base, nl), pat, starts)
    enc = encode(torch_mod, codec, data, bs)
    pos, lens, _ = exact(torch_mod, codec, enc, pat, must=[0, 301, bs + 1, 3 * bs, 4 * bs + 1, 4 * bs + 201], what=("no end", length))
    assert pos[-1] + lens[-1] == n and lens[0] == (31 if length <= 31 else 300)     # (64 bytes at 0 cover the delimiters at 31 and 32)
    data[n - 1] = NL                                       # ... and the same with a delimiter as the data's last byte
    data[n - 1 - length:n - 1] = np.frombuffer(pat, np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    pos, lens, _ = exact(torch_mod, codec, enc, pat, must=[0, 4 * bs + 201], what=("an end", length))
    assert pos[-1] + lens[-1] == n - 1


# ---- case 2: blocks of 64 bytes, across the scan group of 256 tiles --------------------------------------------------------
def test_blocks_of_64_bytes(torch_mod, codec):
    bs, nb = 64, 300
    n = (nb - 1) * bs + 21
    base = base_without(n, 42)
    p5, p33 = pattern_upto_255(5, 45), pattern_upto_255(33, 46)
    # a record over the blocks 240 .. 270 - its delimiters lie in other scan groups than the match at 258 | records whose
    # delimiters are a block's last and first byte | two delimiters in a row | a short record in the short last block
    nl = [70, 5 * bs - 1, 6 * bs, 7 * bs + 10, 7 * bs + 11, 100 * bs + 31, 100 * bs + 32, 240 * bs + 5, 270 * bs + 60, (nb - 1) * bs + 3]
    s5 = [0, 5 * bs, 6 * bs - 5, 7 * bs + 12, 100 * bs + 33, 258 * bs + 62, n - 5]
    s33 = [20, 50 * bs + 40, 255 * bs + 50, 280 * bs + 1]
    data = planted(planted(with_delimiters(base, nl), p5, s5), p33, s33)
    enc = encode(torch_mod, codec, data, bs)
    pos, lens, _ = exact(torch_mod, codec, enc, p5, must=[0, 5 * bs, 7 * bs + 12, 100 * bs + 33, 240 * bs + 6, (nb - 1) * bs + 4], what="5 bytes")
    assert lens[pos.tolist().index(240 * bs + 6)] == 30 * bs + 54
    exact(torch_mod, codec, enc, p33, must=[0, 7 * bs + 12, 240 * bs + 6, 270 * bs + 61], what="33 bytes")
    exact(torch_mod, codec, enc, p33[:2], what="2 bytes")
    exact(torch_mod, codec, enc, p5, delims=bytes([NL, int(p33[0])]), what="two delimiters")
    # ONE record over all 300 tiles, a match in every tile
    data = planted(base, p5[:3], [b * bs + 7 for b in range(nb)])
    one_record(torch_mod, codec, encode(torch_mod, codec, data, bs), p5[:3], "300 tiles")


# ---- case 3: the smallest blocks -----------------------------------------------------------------------------------------
def test_blocks_of_3_bytes(torch_mod, codec):
    bs, nb = 3, 200
    n = nb * bs - 1
    base = base_without(n, 43)
    p7, p2 = pattern_upto_255(7, 47), pattern_upto_255(2, 48)
    nl = [2, 3, 40, 41, 42, 100, 150 * bs - 1, 160 * bs, 400, n - 9]
    s7 = [4, 50, 120 * bs + 2, 170 * bs + 1, n - 7]
    data = planted(with_delimiters(base, nl), p7, s7)
    data[150 * bs:153 * bs + 1] = 9                        # one-symbol blocks among them, and the value once more
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, p7, must=[4, 43, 101, 160 * bs + 1, n - 8], what="7 bytes")
    exact(torch_mod, codec, enc, bytes([9] * 4), must=[150 * bs], what="a run's 4")
    exact(torch_mod, codec, enc, p7[:1], delims=bytes([9, NL]), must_not=[150 * bs], what="the run's value is a delimiter")
    data = planted(base, p2, [b * bs for b in range(nb)])  # ONE record over 200 tiles of 3 and 2 bytes, a match in each
    one_record(torch_mod, codec, encode(torch_mod, codec, data, bs), p2, "200 tiles")


# ---- case 4: one block of several chunks ---------------------------------------------------------------------------------
def test_chunk_seams_of_one_block(torch_mod, codec):
    n = 3 * CHUNK + 77
    base = base_without(n, 44)
    p64, p5 = pattern_upto_255(64, 59), pattern_upto_255(5, 50)
    nl = [CHUNK - 100, CHUNK - 1, CHUNK, CHUNK + 500, 2 * CHUNK - 2000, 2 * CHUNK + 3 * TILE + 100, 3 * CHUNK + 70]
    s64 = [CHUNK - 99, 2 * CHUNK - 63, 2 * CHUNK + 3 * TILE - 1, n - 64]
    s5 = [1000, CHUNK + 1, CHUNK + TILE - 4, 3 * CHUNK - 1]
    data = planted(planted(with_delimiters(base, nl), p64, s64), p5, s5)
    assert np.unique(data).size < 256                      # (a block of all 256 values needs the relaxed flag)
    enc = encode(torch_mod, codec, data, 0)
    assert enc.nb == 1
    pos, lens, _ = exact(torch_mod, codec, enc, p64, must=[CHUNK - 99, 2 * CHUNK - 1999], what="64 bytes")
    assert lens[pos.tolist().index(2 * CHUNK - 1999)] == 2000 + 3 * TILE + 99                # over the chunk seam and three tiles
    exact(torch_mod, codec, enc, p5, must=[0, CHUNK + 1, CHUNK + 501, 2 * CHUNK + 3 * TILE + 101], what="5 bytes")
    data = planted(base, p5, np.arange(7, n - 5, TILE))    # ONE record over both chunk seams, a match in every tile
    one_record(torch_mod, codec, encode(torch_mod, codec, data, 0), p5, "one block")


def test_one_record_over_blocks_of_4099_bytes(torch_mod, codec):
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(5, 51)
    every_tile = [b * bs + t * TILE for b in range(5) for t in range(2)] + [b * bs + 4096 for b in range(4)] + [n - 5]
    data = planted(base_without(n, 45), pat, every_tile)  # (the 3-byte tiles start a match that ends in the next block)
    one_record(torch_mod, codec, encode(torch_mod, codec, data, bs), pat, "15 tiles")


# ---- case 5: many matches in one record ----------------------------------------------------------------------------------
def test_many_matches_are_one_entry(torch_mod, codec):
    bs = 4099
    line = b"ab" * 3 + b"\n" + b"xyxyxyxyab\n" + b"ababab" * 400 + b"\n" + b"b" * 50 + b"abab\n" + b"ba" * 30 + b"\n"
    raw = (line * 8)[:5 * bs]
    data = np.frombuffer(raw, np.uint8).copy()
    enc = encode(torch_mod, codec, data, bs)
    pos, lens, _ = exact(torch_mod, codec, enc, b"abab", must=[0, 18, 18 + 2401], must_not=[7], what="abab")
    assert lens[:3].tolist() == [6, 2400, 54]
    assert int(find_pattern_model(data, b"abab", bs)[2][0]) > 100 * pos.size                # (hundreds of matches a record)
    exact(torch_mod, codec, enc, b"ab", must_not=[], what="ab")
    exact(torch_mod, codec, enc, b"ba" * 20, what="ba x 20")


# ---- case 6: one-symbol blocks ---------------------------------------------------------------------------------------------
def test_one_symbol_blocks_of_delimiters(torch_mod, codec):
    """blocks that hold nothing but the delimiter: thousands of empty records, which never match, between two real ones"""
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(5, 52)
    data = base_without(n, 46)
    data[bs:2 * bs] = NL
    data[3 * bs:4 * bs] = NL
    data = planted(data, pat, [bs - 5, 2 * bs, 2 * bs + 2047, 3 * bs - 5, n - 5])
    data[100] = NL
    enc = encode(torch_mod, codec, data, bs)
    pos, lens, _ = exact(torch_mod, codec, enc, pat, must=[101, 2 * bs, 4 * bs], what="delimiter blocks")
    assert pos.tolist() == [101, 2 * bs, 4 * bs] and lens.tolist() == [bs - 101, bs, bs]
    res = rsearch(torch_mod, codec, enc, pat, b"\n", 0)
    assert res[2].tolist() == [3, 0, 0, 0]


def test_one_symbol_blocks_of_the_pattern(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    for pat in (b")", b")" * 7, b")" * 64):
        one = rsearch(torch, codec, enc, pat, b"\n", 2)
        assert one[2].tolist() == [1, 1, 0, 0]
        check(one, find_records_model(enc.data, pat, b"\n", bs, 2), 2, pat)
    res = rsearch(torch, codec, enc, b"(", b")", 4)          # every byte a delimiter: no record has a byte
    check(res, find_records_model(enc.data, b"(", b")", bs, 4), 4, "all delimiters")
    assert res[2].tolist() == [0, 0, 0, 0]
    res = rsearch(torch, codec, enc, b")))(", b"\n", 4)
    assert res[2].tolist() == [0, 0, 0, 0] and not res[3].any()


@pytest.mark.parametrize("bs", [4096, 4099])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs):
    """records run out of the one-symbol blocks into the ordinary ones behind them, and into them from the ones in front"""
    torch = torch_mod
    data = mixed_blocks(bs, 6, 47)
    data[data == NL] = NL + 1
    data = with_delimiters(data, [bs + 50, bs + 51, 2 * bs - 20, 3 * bs + 2047, 3 * bs + 2048, 5 * bs + 1, 6 * bs - 1])
    out_of = b")" * 4 + pattern_upto_255(6, 53)
    data = planted(data, out_of, [bs - 4, 3 * bs - 4])
    one_leaf = [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)]
    assert one_leaf == [True, False] * 3
    enc = encode(torch, codec, data, bs)
    pos, lens, _ = exact(torch, codec, enc, out_of, must=[0, 2 * bs - 19], what="out of a one-symbol block")
    assert lens.tolist() == [bs + 50, bs + 2047 + 19]
    pos, lens, _ = exact(torch, codec, enc, b")" * 7, must=[0, 2 * bs - 19, 3 * bs + 2049], what="seven")
    assert lens[2] == 2 * bs + 1 - 2049
    exact(torch, codec, enc, b")" * 64, what="sixty-four")
    exact(torch, codec, enc, out_of[4:], delims=b")", must=[bs, 3 * bs], what="the leaf is the delimiter")


# ---- case 7: the caps ----------------------------------------------------------------------------------------------------
def capped_input(torch, codec):
    bs, n = 4099, 5 * 4099
    pat = pattern_upto_255(5, 54)
    nl = [99, 2047, bs - 1, bs + 3000, 2 * bs + 4096, 3 * bs + 10, 4 * bs + 4000]
    starts = [0, 2040, 2100, bs, 2 * bs + 4097, 3 * bs + 11, n - 5]       # records of 99, 1947, 2050, 3000, 12, 8088, 98 bytes
    data = planted(with_delimiters(base_without(n, 48), nl), pat, starts)
    return encode(torch, codec, data, bs), pat


def test_record_caps(torch_mod, codec):
    torch = torch_mod
    enc, pat = capped_input(torch, codec)
    total = int(find_records_model(enc.data, pat, b"\n", enc.bs)[3][0])
    assert total == 7
    for cap in (0, 1, total - 1, total, total + 100):
        for counts in (True, False):
            res = rsearch(torch, codec, enc, pat, b"\n", cap, counts=counts)     # (cap 0: both outputs are NULL)
            assert not res[3].any() and int(res[2][0]) == total
            check(res, find_records_model(enc.data, pat, b"\n", enc.bs, cap), cap, (cap, counts))
    totals, errs = codec.count_records(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, pat)
    assert totals.cpu().tolist() == [total, 0, 0, 0] and not errs.cpu().numpy().any()
    for bad in (b"", b"x" * 65, b"a\nb", b"\n"):
        with pytest.raises(ValueError):
            codec.find_records(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, bad)
    with pytest.raises(ValueError):
        codec.count_records(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, b"a;b", delimiters=b";")


def test_length_caps(torch_mod, codec):
    torch = torch_mod
    enc, pat = capped_input(torch, codec)
    lens = find_records_model(enc.data, pat, b"\n", enc.bs, 7)[1].tolist()
    assert lens == [99, 1947, 2050, 3000, 12, 8088, 98]
    for max_len, cut in ((11, 7), (12, 6), (13, 6), (98, 5), (99, 4), (100, 4), (3000, 1), (8088, 0), (100000, 0), (0, 0)):   # below, at, above
        for cap in (7, 3):
            want = find_records_model(enc.data, pat, b"\n", enc.bs, cap, max_len)
            res = rsearch(torch, codec, enc, pat, b"\n", cap, max_len)
            check(res, want, cap, (max_len, cap))
            if cap == 7:
                assert int(res[2][3]) == cut, (max_len, res[2])


# ---- case 8: a block that is not served ----------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """two byte values have the codes 00 and 01: a 1 at an even payload bit leaves the tree.  One of the two is the
    delimiter, the records are the runs of the other.  The records that touch block 1 - inside it, into it, and the one whose
    delimiter in front is its last byte - are absent, all others present; then the same for blocks 0, 2 and 4, which records
    run out of and into."""
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(55)
    data = (rng.integers(0, 4, n) != 0).astype(np.uint8) * 200 + 7          # 207: the records' bytes, 7: the delimiter
    data[bs - 40:bs + 30] = 207                                               # a record into block 1
    data[3 * bs - 30:4 * bs + 40] = 207                                       # one out of block 2, over all of block 3, into block 4
    data[[bs - 41, 2 * bs + 40, 2 * bs + 41 + 9, 3 * bs - 31, 4 * bs + 40]] = 7
    data[2 * bs + 41:2 * bs + 50] = 207                                       # behind the delimiter at 2 bs + 40: known
    data[0:9] = 207
    data[9] = 7
    data[bs - 50:bs - 41] = 207                                               # in front of the delimiter at bs - 41: known
    data[bs - 51] = 7
    data[2 * bs - 1] = 7                                                      # block 1's last byte is the delimiter in front of ...
    data[2 * bs:2 * bs + 40] = 207                                            # ... a record that is therefore open
    data[n - 9:] = 207
    data[n - 10] = 7
    enc = encode(torch, codec, data, bs)
    delim, pat = bytes([7]), bytes([207] * 9)
    pos, _, _ = exact(torch, codec, enc, pat, delims=delim, must=[0, bs - 50, bs - 40, 2 * bs, 2 * bs + 41, 3 * bs - 30, n - 9], what="undamaged")
    if damage == "a payload bit":
        bad = damaged(enc, payload_start(enc, 1) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
    else:
        bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    served = np.array([True, False, True, True, True])
    for p, cap, max_len in ((pat, n, 0), (pat[:1], n, 5), (pat[:3], 50, 0), (bytes([207] * 64), n, 0)):
        want = find_records_model(enc.data, p, delim, bs, cap, max_len, served=served)
        res = rsearch(torch, codec, bad, p, delim, cap, max_len)
        assert res[3].tolist() == [OK, RW, OK, OK, OK] and int(res[2][2]) == 1, (damage, res[3], res[2])
        check(res, want, cap, (damage, len(p)))
    found = set(find_records_model(enc.data, pat, delim, bs, n, served=served)[0].tolist())
    assert found >= {0, bs - 50, 2 * bs + 41, 3 * bs - 30, n - 9} and not found & {bs - 40, 2 * bs}
    assert found == {int(p) for p in pos if p < bs - 40 or p > 2 * bs}
    # the first, the middle and the last block: the records in front of and behind an open end
    for b in (0, 2, 4):
        sv = np.arange(5) != b
        want = find_records_model(enc.data, pat, delim, bs, n, served=sv)
        res = rsearch(torch, codec, damaged(enc, int(enc.h_offs[b]), 0x01), pat, delim, n)
        assert res[3].tolist() == [OK if k else RW for k in sv]
        check(res, want, n, ("block", b))


# ---- case 9: any content of the sub-index --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["zipf", "mixed"])
def test_sub_index_abuse(torch_mod, codec, shape):
    torch = torch_mod
    bs = 4096
    pat = pattern_upto_255(6, 56)
    if shape == "zipf":
        data = planted(base_without(5 * bs + 1500, 49), pat, [100, bs - 3, 2 * bs + 2045, 5 * bs + 1494])
    else:
        data = mixed_blocks(bs, 6, 50)
        data[data == NL] = NL + 1
        data = planted(data, b")))" + pat, [bs - 3, 3 * bs - 3, 3 * bs + 2040])
    data = with_delimiters(data, np.arange(37, data.size, 1201))
    enc = encode(torch, codec, data, bs)
    one_leaf = np.array([np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)])
    rng = np.random.default_rng(57)
    for p in (pat, b"))))", pat[:2]):
        cap = int(find_records_model(data, p, b"\n", bs)[3][0]) + 3
        errs = exact_or_not_served(torch, codec, enc, p, b"\n", cap, what="own")
        assert not errs.any()
        errs = exact_or_not_served(torch, codec, enc, p, b"\n", cap, sub=torch.zeros_like(enc.sub), what="zeros")
        assert np.array_equal(errs != OK, ~one_leaf)      # (a bit count of 0 cannot be that of 32 codewords)
        random = torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
        errs = exact_or_not_served(torch, codec, enc, p, b"\n", cap, sub=random, what="random")
        assert not errs[one_leaf].any()                   # (one-symbol blocks have no rows to be wrong)


# ---- case 10: one context, call after call ---------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """find_pattern, find_records, find_bytes, find_records with another pattern length and other delimiters, on two layouts,
    without a synchronise in between: masks, edges, counts and record bits of an earlier call must not show in a later one"""
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    p64 = pattern_upto_255(64, 58)
    nl = np.arange(50, n, 777)
    a = encode(torch, codec, planted(with_delimiters(base_without(n, 51), nl), p64, [105, 2100, bs + 5, 3 * bs + 3200]), bs)
    b = encode(torch, codec, planted(with_delimiters(base_without(3 * 64 + 9, 52), [30, 90, 150]), p64[:33], [40, 100]), 64)
    v = int(np.bincount(a.data).argmax())
    jobs = [(a, "pattern", p64, None), (a, "records", p64, b"\n"), (a, "bytes", None, None), (a, "records", p64[:2], bytes([NL, v])),
            (b, "records", p64[:33], b"\n"), (a, "pattern", p64[:3], None), (a, "records", p64[:1], b"")]

    def model(enc, kind, p, delims, cap):
        if kind == "records":
            return find_records_model(enc.data, p, delims, enc.bs, cap)
        return find_pattern_model(enc.data, p, enc.bs, cap) if kind == "pattern" else find_model(enc.data, [v], enc.bs, cap)

    bufs = []
    for enc, kind, p, delims in jobs:
        want = model(enc, kind, p, delims, enc.n)
        assert int(want[-1][0]) > 0
        cap = int(want[-1][0]) + 2
        bufs.append((cap, torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda"),
                     torch.full((LEAD + cap + TAIL,), GUARD32, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    res = []
    for (enc, kind, p, delims), (cap, pbuf, lbuf) in zip(jobs, bufs):
        args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
        if kind == "records":
            res.append(codec.find_records(*args, p, delims, max_records=cap, block_counts=True,
                                          out=(pbuf[LEAD:LEAD + cap], lbuf[LEAD:LEAD + cap]))[2:])
        else:
            kw = dict(max_positions=cap, block_counts=True, out=pbuf[LEAD:LEAD + cap])
            res.append((codec.find_pattern(*args, p, **kw) if kind == "pattern" else codec.find_bytes(*args, [v], **kw))[1:])
    torch.cuda.synchronize()
    for (enc, kind, p, delims), (cap, pbuf, lbuf), (totals, errs, cnt) in zip(jobs, bufs, res):
        want = model(enc, kind, p, delims, cap)
        host = (totals.cpu().numpy(), errs.cpu().numpy(), cnt.cpu().numpy())
        if kind == "records":
            check((pbuf.cpu().numpy(), lbuf.cpu().numpy()) + host, want, cap, (kind, p))
        else:
            check((pbuf.cpu().numpy(),) + host, want, cap, (kind, p))


def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    pbuf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    _, _, totals, errs, cnt = codec.find_records(empty, 0, offsets, 0, codec.new_sub_index(0, 4096), 0, 4096, b"ERROR",
                                                 max_records=4, max_len=16, block_counts=True, out=(pbuf, lbuf))
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    assert pbuf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4


# ---- case 11: the pipeline -----------------------------------------------------------------------------------------------
def test_grep_lines_with_error(torch_mod, codec):
    """grep = find_records -> gather with no device op of the caller's in between and no host synchronisation before the
    comparison with what a splitlines filter gives: each line once, without its newline, cut at max_len"""
    torch = torch_mod
    n, bs = (1 << 20) + 1, 65536
    data = datagen.logtext(n)
    enc = encode(torch, codec, data, bs)
    lines = [ln for ln in bytes(data).split(b"\n") if b"ERROR" in ln]
    assert len(lines) > 8
    longest = max(len(ln) for ln in lines)
    for max_records, max_len in ((len(lines) + 5, 64), (len(lines), longest), (7, 200)):
        rows, raws, errs, totals, block_errs = codec.grep(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, b"ERROR",
                                                          max_records, max_len)
        torch.cuda.synchronize()
        written = min(len(lines), max_records)
        cut = sum(len(ln) > max_len for ln in lines[:written])
        assert totals.cpu().tolist() == [len(lines), written, 0, cut]
        assert not block_errs.cpu().numpy().any() and not errs.cpu().numpy().any()
        rows, raws = rows.cpu().numpy(), raws.cpu().numpy()
        assert rows.shape == (max_records, max_len) and not raws[written:].any()
        for i, ln in enumerate(lines[:written]):
            assert raws[i] == min(len(ln), max_len) and bytes(rows[i, :raws[i]]) == ln[:max_len], i

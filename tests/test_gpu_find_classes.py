"""GPU tests of hufgpu_find_classes and hufgpu_find_records_classes (the class route of GpuCodec.find_pattern /
count_pattern / find_records / count_records / grep): a pattern whose every position is a set of byte values - ignore case,
wildcards, digit classes - found straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the models of tests/find_classes_model.py (themselves checked against
Python's `re` in tests/test_find_classes_args.py).  As in tests/test_gpu_find.py every output buffer has guard words in front
and behind and is filled with the guard first: the words beyond totals[1] must still hold it.  The shapes are those of
tests/test_gpu_find_pattern.py, the smallest that reach every seam: five blocks of 4 099 bytes (tiles of 2 048, 2 048 and 3
symbols), 300 blocks of 64 bytes (two scan groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes (three chunks).
"""
import functools
import re

import numpy as np
import pytest

import find_support
from find_classes_model import find_class_records_model, find_classes_model
from find_model import find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from find_support import (ANY, CHUNK, FOUR_SHAPES, GUARD32, GUARD64, LEAD, NL, NOT_NL, OK, RW, TAIL, TILE, base_of, base_without, check,
                          codec, damaged, encode, mixed_blocks, pattern_below_255, payload_start, planted, planted_each, psearch,
                          rsearch, same_arrays, spellings, torch_mod, two_values, with_delimiters)
from libhuffman_amd import datagen
from libhuffman_amd.codec import GpuCodec

pytestmark = pytest.mark.gpu


# ---- checks ----------------------------------------------------------------------------------------------------------------
exact = functools.partial(find_support.exact_positions, find_classes_model, find_support.as_is)
exact_or_not_served = functools.partial(find_support.positions_exact_or_not_served, find_classes_model, find_support.as_is)
records_exact = functools.partial(find_support.exact_records, find_class_records_model, find_support.as_is)
records_exact_or_not_served = functools.partial(find_support.records_exact_or_not_served, find_class_records_model, find_support.as_is)


# ---- case 1: classes of one value are the literal, at every seam and at the data's end ---------------------------------------
@pytest.mark.parametrize("length", [2, 5, 33, 64])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_classes_of_one_value_are_find_pattern(torch_mod, codec, shape, length):
    bs, n, starts = FOUR_SHAPES[shape]
    pat = pattern_below_255(length, 100 + length)
    classes = [bytes([v]) for v in pat]
    enc = encode(torch_mod, codec, planted(base_of(shape), pat, starts + [n - length]), bs)
    exact(torch_mod, codec, enc, classes, must=starts + [n - length], literal=pat, what=(shape, "ends with it", length))
    enc = encode(torch_mod, codec, planted(base_of(shape), pat, starts + [n - length + 1]), bs)      # ... one byte past the data
    exact(torch_mod, codec, enc, classes, must=starts, must_not=[n - length + 1, n - length], literal=pat, what=(shape, "one short", length))
    got = psearch(torch_mod, codec, enc, list(pat), len(starts) + 7)                                # (an int a class)
    assert same_arrays(got, psearch(torch_mod, codec, enc, pat, len(starts) + 7))


# ---- case 2: ignore case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word", [b"ErRoR", b"TheQuickBrownFoxJumpsOverTheLazyDo"[:33]], ids=["5", "33"])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_ignore_case(torch_mod, codec, shape, word):
    bs, n, starts = FOUR_SHAPES[shape]
    assert word.isalpha()
    starts = starts + [n - len(word)]
    words = spellings(word, len(starts), len(word))
    data = planted_each(base_of(shape), words, starts)
    spoiled = starts[len(starts) // 2]                      # one plant with a non-letter in its middle: '[' is 'A' + 26, '5' a digit
    data[spoiled + len(word) // 2] = ord("[") if len(word) == 5 else ord("5")
    enc = encode(torch_mod, codec, data, bs)
    must = [s for s in starts if s != spoiled]
    model = GpuCodec.byte_classes(word, ignore_case=True)
    assert len(set(words)) > 2 or len(starts) <= 2
    exact(torch_mod, codec, enc, word, must=must, must_not=[spoiled], model=model, ignore_case=True, what=(shape, len(word)))
    exact(torch_mod, codec, enc, [bytes([c | 0x20, c & ~0x20]) for c in word], must=must, must_not=[spoiled], what=(shape, "as a list"))
    totals, errs = codec.count_pattern(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, word, ignore_case=True)
    assert totals.cpu().tolist() == [int(find_classes_model(data, model, bs)[2][0]), 0, 0, 0] and not errs.cpu().numpy().any()


# ---- case 3: wildcards -------------------------------------------------------------------------------------------------------
def fill_any(rng, classes, pool):
    """bytes that the classes match: the one value, or for the full class a random byte of `pool` - the values the input
    holds already: a tree of all 256 values would need HUFGPU_RELAXED_TREE"""
    return bytes(c[0] if len(c) == 1 else int(rng.choice(pool)) for c in classes)


@pytest.mark.parametrize("length", [2, 7, 64])
@pytest.mark.parametrize("where", ["middle", "first"])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_the_full_class_in_the_middle_and_in_the_first_place(torch_mod, codec, shape, where, length):
    """the first place: every start is a candidate - the dense first class"""
    bs, n, starts = FOUR_SHAPES[shape]
    rng = np.random.default_rng(length)
    classes = [bytes([v]) for v in pattern_below_255(length, 200 + length)]
    holes = [0] if where == "first" else ([1] if length == 2 else [length // 2, length // 2 + 1, length - 2])
    if where == "middle" and length == 2:
        classes = classes + classes[:1]                    # (a middle needs three positions)
    for k in holes:
        classes[k] = ANY
    m = len(classes)
    starts = starts + [n - m]
    pool = np.unique(base_of(shape))
    data = planted_each(base_of(shape), [fill_any(rng, classes, pool) for _ in starts], starts)
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, classes, must=starts, what=(shape, where, length))


@pytest.mark.parametrize("length", [2, 64])
def test_the_full_class_in_the_last_place(torch_mod, codec, length):
    """... matches at n - len and not at n - len + 1; and when the wildcard's byte is the first byte of the next block the
    match depends on that block being served"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    lit = pattern_below_255(length - 1, 300 + length)
    classes = [bytes([v]) for v in lit] + [ANY]
    seam = 2 * bs - (length - 1)                            # the literal bytes end block 1, the wildcard's byte opens block 2
    starts = [s for s in starts if abs(s - seam) > 64] + [seam]
    enc = encode(torch, codec, planted(base_of("5x4099"), lit, starts + [n - length]), bs)
    exact(torch, codec, enc, classes, must=starts + [n - length], what=("ends with it", length))
    short = encode(torch, codec, planted(base_of("5x4099"), lit, starts + [n - length + 1]), bs)
    exact(torch, codec, short, classes, must=starts, must_not=[n - length + 1, n - length], what=("one short", length))
    bad = damaged(enc, int(enc.h_offs[2]), 0x01)            # block 2's block_len: not the layout's
    res = psearch(torch, codec, bad, classes, len(starts) + 9)
    assert res[2].tolist() == [OK, OK, RW, OK, OK]
    want = find_classes_model(enc.data, classes, bs, len(starts) + 9, served=res[2] == OK)
    assert seam not in want[0].tolist() and starts[0] in want[0].tolist()
    check(res, want, len(starts) + 9, ("the next block is not served", length))


# ---- case 4: one position is find_bytes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_one_position_is_find_bytes(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    data = base_of(shape)
    enc = encode(torch, codec, data, bs)
    frequent = int(np.bincount(data).argmax())
    for values in ([frequent], [frequent, 41, 255], [int(v) for v in np.random.default_rng(8).permutation(256)[:200]]):
        want = find_model(data, values, bs, n)
        cap = int(want[2][0]) + 5
        buf = torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda")
        _, totals, errs, cnt = codec.find_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, values,
                                                max_positions=cap, block_counts=True, out=buf[LEAD:LEAD + cap])
        res = psearch(torch, codec, enc, [values], cap)
        assert same_arrays(res, (buf.cpu().numpy(), totals.cpu().numpy(), errs.cpu().numpy(), cnt.cpu().numpy())), len(values)
        check(res, find_model(data, values, bs, cap), cap, len(values))
        check(res, find_classes_model(data, [values], bs, cap), cap, len(values))


# ---- case 5: wide classes, many overlapping matches ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_sixty_four_wide_classes(torch_mod, codec, shape):
    """64 positions of [128 .. 255] over bytes below 128 with runs of 64, 65 and 200 bytes of 128 and above: 1, 2 and 137
    matches a run, each run across a tile or a block seam"""
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(11)
    data = base_of(shape) & 0x7F
    at = {"5x4099": [2048 - 30, 4099 - 64, 2 * 4099 + 2048 - 100], "300x64": [64 * 7 + 10, 64 * 255 + 1, 64 * 100 - 5],
          "3chunks": [CHUNK - 1, TILE - 63, 2 * CHUNK - 150]}[shape]
    for s, run in zip(at, (64, 65, 200)):
        data[s:s + run] = rng.integers(128, 256, run)
    enc = encode(torch_mod, codec, data, bs)
    classes = [bytes(range(128, 256))] * 64
    total, _ = exact(torch_mod, codec, enc, classes, must=[at[0], at[1], at[1] + 1, at[2], at[2] + 136],
                  must_not=[at[0] + 1, at[1] + 2, at[2] + 137], what=shape)
    assert total == 1 + 2 + 137


# ---- case 6: one-symbol blocks -------------------------------------------------------------------------------------------------
def test_one_symbol_blocks(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    for m in (1, 7, 33, 64):
        classes = [bytes([41, 40 + 3 * (k % 5)]) for k in range(m)]            # the leaf in every class
        want = find_classes_model(enc.data, classes, bs, n + 3)
        assert np.array_equal(want[0], np.arange(n - m + 1)) and want[1].tolist() == [bs] * 4 + [bs - m + 1]
        res = psearch(torch, codec, enc, classes, n + 3)
        assert not res[2].any()
        check(res, want, n + 3, m)
        for k in sorted({0, m // 2, m - 1}):                                    # ... in all classes but one
            res = psearch(torch, codec, enc, classes[:k] + [b"(*"] + classes[k + 1:], 4)
            assert not res[2].any() and res[1].tolist() == [0, 0, 0, 0], (m, k)
            check(res, find_classes_model(enc.data, classes[:k] + [b"(*"] + classes[k + 1:], bs, 4), 4, (m, k))


@pytest.mark.parametrize("bs", [4096, 4099])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs):
    torch = torch_mod
    data = mixed_blocks(bs, 6, 26)
    tail, head = pattern_below_255(6, 1), pattern_below_255(5, 2)
    out_of, into = b")" * 4 + tail, head + b")" * 3
    s_out, s_in = [bs - 4, 3 * bs - 4], [2 * bs - 5, 4 * bs - 5]
    data = planted(planted(data, out_of, s_out), into, s_in)
    data[3 * bs - 4 + 6] ^= 1                               # one plant in the class's other value
    enc = encode(torch, codec, data, bs)
    assert [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)] == [True, False] * 3
    paren = [b")("]
    exact(torch, codec, enc, paren * 4 + [bytes([c, c ^ 1]) for c in tail], must=s_out, what="out of a one-symbol block")
    exact(torch, codec, enc, [bytes([c, c ^ 1]) for c in head] + paren * 3, must=s_in, what="into a one-symbol block")
    exact(torch, codec, enc, paren * 3 + [ANY] * 2 + [bytes([c, c ^ 1]) for c in tail[1:]], must=s_out, what="a wildcard on the seam")
    exact(torch, codec, enc, paren * 64, must=[bs - 64, 2 * bs], must_not=[bs - 63], what="sixty-four")
    for p in (paren * 4 + [bytes([c, c ^ 1]) for c in tail], paren * 64):
        exact_or_not_served(torch, codec, enc, p, 50, sub=torch.zeros_like(enc.sub), what="zeros")


# ---- case 7: blocks that are not served ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(30)
    lit = bytes((rng.integers(0, 2, 33) * 200 + 7).astype(np.uint8))
    classes = [bytes([v]) for v in lit]
    for k in (3, 17, 32):
        classes[k] = b"\x07\xcf"                           # either value
    starts = [0, 500, bs - 43, bs - 10, bs + 1000, bs + 2040, 2 * bs - 1, 2 * bs + 40, 2 * bs + 2030, 3 * bs - 33, 4 * bs - 5, n - 33]
    enc = encode(torch, codec, planted(two_values(n, 31), lit, starts), bs)
    exact(torch, codec, enc, classes, must=starts, what="undamaged")
    assert not (enc.data == NL).any()
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for p, cap in ((classes, 40), (classes[:3], n), ([ANY, classes[0]], n)):
            errs = exact_or_not_served(torch, codec, bad, p, cap, what=(damage, b, len(p)))
            assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
        # ONE record (no delimiter occurs): any block that is not served leaves its extent unknown
        res = rsearch(torch, codec, bad, classes, b"\n", 3)
        assert res[2].tolist() == [0, 0, 1, 0]
        check(res, find_class_records_model(enc.data, classes, b"\n", bs, 3, served=res[3] == OK), 3, (damage, b))


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    word = b"needle"
    nl = [50, 4000, bs + 7, 2 * bs - 1, 3 * bs, 4 * bs + 2047, 5 * bs + 100]
    at = [100, bs - 3, 2 * bs + 2045, 3 * bs + 1, 5 * bs + 1494]
    data = planted_each(with_delimiters(base_without(5 * bs + 1500, 31), nl), spellings(word, len(at), 3), at)
    enc = encode(torch, codec, data, bs)
    classes = [bytes([c, c ^ 0x20]) for c in word]
    rng = np.random.default_rng(33)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    for p in (classes, classes[:2], [NOT_NL] + classes[1:]):
        cap = int(find_classes_model(data, p, bs)[2][0]) + 3
        assert not exact_or_not_served(torch, codec, enc, p, cap, what="own").any()
        errs = exact_or_not_served(torch, codec, enc, p, cap, sub=other, what=sub)
        assert sub == "random" or errs.all()                # (a bit count of 0 cannot be that of 32 codewords)
        assert not records_exact_or_not_served(torch, codec, enc, p, b"\n", cap, what="own").any()
        records_exact_or_not_served(torch, codec, enc, p, b"\n", cap, sub=other, max_len=9, what=sub)


# ---- case 8: the caps ----------------------------------------------------------------------------------------------------------
def test_caps(torch_mod, codec):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    word = b"Warning"
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000]
    starts = starts + [starts[1] + 20, n - len(word)]      # (two matches in one record)
    data = planted_each(with_delimiters(base_without(n, 71), nl), spellings(word, len(starts), 4), starts)
    enc = encode(torch, codec, data, bs)
    classes = GpuCodec.byte_classes(word, ignore_case=True)
    total = int(find_classes_model(data, classes, bs)[2][0])
    rtotal = int(find_class_records_model(data, classes, b"\n", bs)[3][0])
    assert total == len(starts) and 2 < rtotal < total
    for cap in (0, 1, total - 1, total):
        for counts in (True, False):
            res = psearch(torch, codec, enc, word, cap, counts=counts, ignore_case=True)        # (cap 0: d_pos is NULL)
            assert not res[2].any() and int(res[1][0]) == total
            check(res, find_classes_model(data, classes, bs, cap), cap, (cap, counts))
    for cap in (0, 1, rtotal - 1, rtotal):
        for counts in (True, False):
            res = rsearch(torch, codec, enc, word, b"\n", cap, counts=counts, ignore_case=True)
            assert not res[3].any() and int(res[2][0]) == rtotal
            check(res, find_class_records_model(data, classes, b"\n", bs, cap), cap, (cap, counts))
    totals, errs = codec.count_records(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, word, ignore_case=True)
    assert totals.cpu().tolist() == [rtotal, 0, 0, 0] and not errs.cpu().numpy().any()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    for bad in ([], [1] * 65, [1, b""]):
        with pytest.raises(ValueError):
            codec.find_pattern(*args, bad)
        with pytest.raises(ValueError):
            codec.find_records(*args, bad)
    with pytest.raises(ValueError, match="class 2 of the pattern holds a delimiter"):
        codec.find_records(*args, [b"a", b"b", ANY, b"c"])
    with pytest.raises(ValueError, match="class 0 "):
        codec.find_records(*args, b",x", delimiters=b";,", ignore_case=True)
    codec.find_records(*args, [b"a", ANY], delimiters=b"")  # the empty delimiter set: valid


# ---- case 9: records -------------------------------------------------------------------------------------------------------------
def test_records_ignore_case_at_the_seams(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    word = b"error"
    base = base_without(n, 41)
    # delimiters: a lane seam's two sides, a tile seam's two sides, two in a row, a block's last and its first byte, a 3-byte
    # tile's last two bytes, another block's first byte alone (tests/test_gpu_find_records.py)
    nl = [31, 32, 300, 2047, 2048, 2500, 2501, 3000, bs - 1, bs, 2 * bs + 100, 2 * bs + 4097, 3 * bs - 1, 3 * bs + 1500, 4 * bs, 4 * bs + 200]
    starts = [0, 301, 2047 - 5, bs + 2048 - 3, 2 * bs - 3, 3 * bs + 1500 - 5, 4 * bs + 1, n - 5]
    data = planted_each(with_delimiters(base, nl), spellings(word, len(starts), 6), starts)
    classes = GpuCodec.byte_classes(word, ignore_case=True)
    enc = encode(torch, codec, data, bs)
    pos, lens, _ = records_exact(torch, codec, enc, word, must=[0, 301, bs + 1, 3 * bs, 4 * bs + 1, 4 * bs + 201], model=classes,
                              ignore_case=True, what="no end")
    assert pos[-1] + lens[-1] == n and lens[0] == 31
    records_exact(torch, codec, enc, [NOT_NL] + [bytes([c, c ^ 0x20]) for c in word[1:]], must=[301, bs + 1], must_not=[2502],
                  what="a wide first class")
    for max_len in (1, 30, 31, 32, 5000):                  # below, at and above the lengths: totals[3]
        records_exact(torch, codec, enc, word, model=classes, max_len=max_len, ignore_case=True, what=max_len)
    cut = [int(find_class_records_model(data, classes, b"\n", bs, n, m)[3][3]) for m in (1, 31, 5000)]
    assert cut[0] > cut[1] >= cut[2] == 0
    data[n - 1] = NL                                       # a delimiter as the data's last byte, and one as its first
    data[n - 6:n - 1] = np.frombuffer(b"eRRoR", np.uint8)
    data[0] = NL
    data[1:6] = np.frombuffer(b"ERROr", np.uint8)
    enc = encode(torch, codec, data, bs)
    pos, lens, _ = records_exact(torch, codec, enc, word, must=[1, 4 * bs + 201], must_not=[0], model=classes, ignore_case=True, what="an end")
    assert pos[-1] + lens[-1] == n - 1


@pytest.mark.parametrize("shape", ["300x64", "200x3"])
def test_one_record_over_all_blocks(torch_mod, codec, shape):
    """a match in every tile; the empty delimiter set and a delimiter that never occurs both give ONE entry, (0, n)"""
    bs, n, _ = FOUR_SHAPES[shape]
    base = base_without(n, 42)
    nb = (n + bs - 1) // bs
    two = [b"Qq", b"Zz"]
    data = planted_each(base, [b"qZ", b"Qz"] * nb, [b * bs for b in range(nb)])
    enc = encode(torch_mod, codec, data, bs)
    for delims in (b"", b"\n"):
        res = rsearch(torch_mod, codec, enc, two, delims, 3)
        assert res[2].tolist() == [1, 1, 0, 0] and not res[3].any(), (delims, res[2])
        assert res[0][LEAD] == 0 and int(res[1].view(np.uint32)[LEAD]) == n, delims
        check(res, find_class_records_model(data, two, delims, bs, 3), 3, delims)
        assert res[4].tolist() == [1] + [0] * (nb - 1)
    res = rsearch(torch_mod, codec, enc, [ANY, b"Zz"], b"", 3)                  # the full class with the empty delimiter set
    check(res, find_class_records_model(data, [ANY, b"Zz"], b"", bs, 3), 3, "any")


def test_grep_ignore_case(torch_mod, codec):
    """grep(..., ignore_case=True) without a synchronisation, against an `re` filter over the split lines"""
    torch = torch_mod
    n, bs = (1 << 18) + 1, 65536
    data = datagen.logtext(n).copy()
    lines = bytes(data).split(b"\n")
    at = 0
    for i, line in enumerate(lines):                        # other spellings of the word in some of the lines that hold it
        k = line.find(b"ERROR")
        if k >= 0 and i % 3:
            data[at + k:at + k + 5] = np.frombuffer([b"error", b"Error"][i % 2], np.uint8)
        at += len(line) + 1
    lines = bytes(data).split(b"\n")
    want = [l for l in lines if re.search(rb"error", l, re.IGNORECASE)]
    exact_case = [l for l in lines if b"ERROR" in l]
    assert 0 < len(exact_case) < len(want) < n // 40
    enc = encode(torch, codec, data, bs)
    cap, width = len(want) + 5, 256
    rows, raws, gerrs, totals, block_errs = codec.grep(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, b"error", cap, width,
                                                       ignore_case=True)
    rows, raws, gerrs, totals, block_errs = (x.cpu().numpy() for x in (rows, raws, gerrs, totals, block_errs))
    assert totals.tolist() == [len(want), len(want), 0, sum(len(l) > width for l in want)] and not block_errs.any() and not gerrs.any()
    assert not raws[len(want):].any()
    for i, line in enumerate(want):
        assert raws[i] == min(len(line), width) and bytes(rows[i, :raws[i]]) == line[:width], i


# ---- case 10: one context, call after call -------------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """find_pattern, a class call, find_records with classes, find_bytes, a literal find_records - and the two literal calls once
    more - without a synchronise in between: each gives its own model's answer, and the literal calls the same after a class
    call as before it"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    word = b"Segfault"
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000]
    data = planted_each(with_delimiters(base_without(n, 72), nl), spellings(word, len(starts), 5), starts)
    enc = encode(torch, codec, data, bs)
    lower = word.lower()
    classes = GpuCodec.byte_classes(word, ignore_case=True)
    v = int(np.bincount(data).argmax())
    jobs = [("pattern", lower), ("classes", word), ("class records", word), ("bytes", [v]), ("records", lower), ("pattern", lower),
            ("records", lower)]

    def model(kind, cap):
        if kind == "pattern":
            return find_pattern_model(data, lower, bs, cap)
        if kind == "classes":
            return find_classes_model(data, classes, bs, cap)
        if kind == "bytes":
            return find_model(data, [v], bs, cap)
        return (find_records_model(data, lower, b"\n", bs, cap) if kind == "records" else find_class_records_model(data, classes, b"\n", bs, cap))

    bufs = []
    for kind, _ in jobs:
        want = model(kind, n)
        cap = int(want[-1][0]) + 2
        assert int(want[-1][0]) > 0, kind
        bufs.append((cap, torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda"),
                     torch.full((LEAD + cap + TAIL,), GUARD32, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    res = []
    for (kind, key), (cap, pbuf, lbuf) in zip(jobs, bufs):
        if "records" in kind:
            res.append(codec.find_records(*args, key, b"\n", max_records=cap, block_counts=True, out=(pbuf[LEAD:LEAD + cap], lbuf[LEAD:LEAD + cap]),
                                          ignore_case=kind == "class records"))
        elif kind == "bytes":
            res.append(codec.find_bytes(*args, key, max_positions=cap, block_counts=True, out=pbuf[LEAD:LEAD + cap]))
        else:
            res.append(codec.find_pattern(*args, key, max_positions=cap, block_counts=True, out=pbuf[LEAD:LEAD + cap], ignore_case=kind == "classes"))
    torch.cuda.synchronize()
    host = []
    for (kind, key), (cap, pbuf, lbuf), r in zip(jobs, bufs, res):
        if "records" in kind:
            got = (pbuf.cpu().numpy(), lbuf.cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy(), r[4].cpu().numpy())
            check(got, model(kind, cap), cap, kind)
        else:
            got = (pbuf.cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy())
            check(got, model(kind, cap), cap, kind)
        host.append(got)
    assert same_arrays(host[0], host[5]) and same_arrays(host[4], host[6])
    assert int(host[1][1][0]) > int(host[0][1][0]) > 0      # the class call sees the spellings that the literal does not


def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    pos, totals, errs, cnt = codec.find_pattern(empty, 0, offsets, 0, sub, 0, 4096, b"error", max_positions=4, block_counts=True, out=buf,
                                                ignore_case=True)
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    _, _, totals, errs, cnt = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, [b"eE", b"rR"], max_records=4, block_counts=True,
                                                 out=(buf, lbuf))
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4

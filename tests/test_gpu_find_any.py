"""GPU tests of hufgpu_find_any and hufgpu_find_records_any (GpuCodec.AnyOf as the `pattern` of find_pattern / count_pattern /
find_records / count_records / grep): ANY of several class patterns - grep -e A -e B - found in one walk of the stream,
straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the models of tests/find_any_model.py (themselves checked against
Python's `re` in tests/test_find_any_args.py).  As in tests/test_gpu_find.py every output buffer has guard words in front and
behind and is filled with the guard first: the words beyond totals[1] must still hold it.  Helpers and the four shapes are
those of tests/test_gpu_find_classes.py: five blocks of 4 099 bytes (tiles of 2 048, 2 048 and 3 symbols), 300 blocks of 64
bytes (two scan groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes (three chunks).
"""
import functools
import re

import numpy as np
import pytest

import find_support
from find_any_model import find_any_model, find_any_records_model
from find_classes_model import find_class_records_model, find_classes_model
from find_model import find_model
from find_pattern_model import find_pattern_model
from find_support import (ANY, FOUR_SHAPES, GUARD32, GUARD64, LEAD, NOT_NL, OK, RW, TAIL, TILE, TILE_END, AnyOf, base_of, base_without,
                          check, codec, damaged, encode, mixed_blocks, pattern_below_255, payload_start, planted, planted_each,
                          psearch, rsearch, same_arrays, spellings, torch_mod, two_values, with_delimiters)
from libhuffman_amd import datagen
from libhuffman_amd.codec import GpuCodec

pytestmark = pytest.mark.gpu

MIXES = [(2, 5, 33), (31, 33), (32, 32), (1, 63)]
MIX_IDS = ["x".join(map(str, m)) for m in MIXES]


# ---- checks ----------------------------------------------------------------------------------------------------------------
exact = functools.partial(find_support.exact_positions, find_any_model, find_support.any_of)
exact_or_not_served = functools.partial(find_support.positions_exact_or_not_served, find_any_model, find_support.any_of)
records_exact = functools.partial(find_support.exact_records, find_any_records_model, find_support.any_of)
records_exact_or_not_served = functools.partial(find_support.records_exact_or_not_served, find_any_records_model, find_support.any_of)


def widened(pat, every=3):
    """the literal as classes, every third position with a second value (no newline, not 255)"""
    return [bytes([v]) if k % every else bytes([v, 128 + (v + 7) % 120]) for k, v in enumerate(pat)]


# ---- identities, in the same process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 5, 33, 64])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_one_alternative_is_the_class_call(torch_mod, codec, shape, length):
    """positions and records, word for word, with the pattern at every seam, at the data's end and one byte past it"""
    bs, n, starts = FOUR_SHAPES[shape]
    pat = pattern_below_255(length, 100 + length)
    classes = widened(pat)
    for last in (n - length, n - length + 1):
        data = planted(base_of(shape), pat, starts + [last])
        data[data == 10] = 11                               # one record: the delimiter that follows is the only one
        data[next(p for p in range(n // 2, n) if all(not s <= p < s + length for s in starts + [last]))] = 10
        enc = encode(torch_mod, codec, data, bs)
        total, res = exact(torch_mod, codec, enc, [classes], must=starts + ([last] if last == n - length else []),
                           must_not=[last] if last != n - length and length > 1 else [], what=(shape, length, last))
        assert same_arrays(res, psearch(torch_mod, codec, enc, classes, total + 7)), (shape, length, "differs from find_classes")
        got = rsearch(torch_mod, codec, enc, AnyOf(classes), b"\n", 5, max_len=100)
        assert same_arrays(got, rsearch(torch_mod, codec, enc, classes, b"\n", 5, max_len=100)), (shape, length, "records differ")
        check(got, find_class_records_model(data, classes, b"\n", bs, 5, 100), 5, (shape, length))


@pytest.mark.parametrize("count", [1, 3, 64])
@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_alternatives_of_one_position_are_find_bytes(torch_mod, codec, shape, count):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    data = base_of(shape)
    enc = encode(torch, codec, data, bs)
    rng = np.random.default_rng(count)
    frequent = int(np.bincount(data).argmax())
    sets = [[frequent]] + [[int(v) for v in rng.permutation(255)[:int(rng.integers(1, 4))]] for _ in range(count - 1)]
    union = sorted(set(v for s in sets for v in s))
    want = find_model(data, union, bs, n)
    cap = int(want[2][0]) + 5
    buf = torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda")
    _, totals, errs, cnt = codec.find_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, union, max_positions=cap,
                                            block_counts=True, out=buf[LEAD:LEAD + cap])
    res = psearch(torch, codec, enc, AnyOf(*[[s] for s in sets]), cap)
    assert same_arrays(res, (buf.cpu().numpy(), totals.cpu().numpy(), errs.cpu().numpy(), cnt.cpu().numpy())), count
    check(res, find_model(data, union, bs, cap), cap, count)
    check(res, find_any_model(data, [[s] for s in sets], bs, cap), cap, count)


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_alternatives_are_the_union_of_their_class_calls(torch_mod, codec, shape):
    bs, n, starts = FOUR_SHAPES[shape]
    words = [b"ERROR", b"Fatal", b"panic:", b"ERR"]         # (ERR lies wherever ERROR does: those starts count once)
    data = planted_each(base_of(shape), [words[i % 3] for i in range(len(starts))], starts)
    enc = encode(torch_mod, codec, data, bs)
    alts = [list(GpuCodec.byte_classes(w, ignore_case=True)) for w in words]
    alts = [[np.flatnonzero(np.unpackbits(c, bitorder="little")).tolist() for c in a] for a in alts]
    total, res = exact(torch_mod, codec, enc, alts, must=starts, what=shape)
    each = [psearch(torch_mod, codec, enc, a, total + 7) for a in alts]
    union = np.unique(np.concatenate([r[0][LEAD:LEAD + int(r[1][1])] for r in each]))
    assert sum(int(r[1][0]) for r in each) > total == union.size
    assert np.array_equal(res[0][LEAD:LEAD + total], union)
    _, res = exact(torch_mod, codec, enc, words, must=starts, model=alts, ignore_case=True, what=(shape, "literals, ignore_case"))
    assert np.array_equal(res[0][LEAD:LEAD + total], union)
    totals, errs = codec.count_pattern(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, AnyOf(*words), ignore_case=True)
    assert totals.cpu().tolist() == [total, 0, 0, 0] and not errs.cpu().numpy().any()


# ---- mixed lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", MIXES, ids=MIX_IDS)
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_mixed_lengths(torch_mod, codec, shape, mix):
    """every alternative at every lane, tile, chunk and block seam of the shape (the plants rotate through the starts); the
    shortest one right in front of a tile's end, where the longest does not fit - found once, by the seam kernel -; at
    n - len_short, where the longest would pass raw_size; and at n - len_short + 1, where nothing lies"""
    bs, n, starts = FOUR_SHAPES[shape]
    lits = [pattern_below_255(m, 500 + 70 * j + m) for j, m in enumerate(mix)]
    alts = [widened(p) for p in lits]
    short = min(lits, key=len)
    tsym = min(bs or TILE, TILE)
    extra = [TILE_END[shape] - len(short)] if len(short) <= tsym else []
    for rot in range(len(mix)):
        data = planted_each(base_of(shape), [lits[(i + rot) % len(mix)] for i in range(len(starts))], starts)
        data = planted(data, short, extra + [n - len(short)])
        enc = encode(torch_mod, codec, data, bs)
        exact(torch_mod, codec, enc, alts, must=starts + extra + [n - len(short)], what=(shape, mix, rot))
    data = planted(data, bytes(255 - v for v in short), [n - len(short)])       # (values of 1 to 127: not the alternative's)
    data = planted(data, short, [n - len(short) + 1])
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, alts, must=starts + extra, must_not=[n - len(short)] + ([n - len(short) + 1] if len(short) > 1 else []),
          what=(shape, mix, "one short"))


# ---- the same start, and what one alternative must not do to another ---------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_two_alternatives_at_one_start_count_once(torch_mod, codec, shape):
    bs, n, starts = FOUR_SHAPES[shape]
    base = base_of(shape).copy()
    base[base == ord("a")] = ord("e")                       # no `a` but the planted ones
    data = planted_each(base, [b"abc", b"abd"] * len(starts), starts)
    enc = encode(torch_mod, codec, data, bs)
    total, _ = exact(torch_mod, codec, enc, [b"ab", b"abc"], must=starts, what=shape)
    assert total == len(starts)
    total, _ = exact(torch_mod, codec, enc, [b"abc", b"ab", [b"a", ANY, b"cd"]], must=starts, what=(shape, "three"))
    assert total == len(starts)


@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_no_cross_talk_between_alternatives(torch_mod, codec, shape):
    """`ab` and `cd` lie next to each other in the state: `ad`, `cb` and `bc` are no match, `abcd` is two"""
    bs, n, starts = FOUR_SHAPES[shape]
    base = base_of(shape).copy()
    base[np.isin(base, list(b"abcd"))] = ord("e")
    plants = [b"ad", b"cb", b"bc", b"abcd"]
    data = planted_each(base, [plants[i % 4] for i in range(len(starts))], starts)
    data = planted(data, b"abcd", [n - 4])
    enc = encode(torch_mod, codec, data, bs)
    hits = [s for i, s in enumerate(starts) if i % 4 == 3] + [n - 4]
    total, _ = exact(torch_mod, codec, enc, [b"ab", b"cd"], must=hits + [s + 2 for s in hits], what=shape)
    assert total == 2 * len(hits)
    total, _ = exact(torch_mod, codec, enc, [b"cd", b"ab"], must=hits + [s + 2 for s in hits], what=(shape, "the other order"))
    assert total == 2 * len(hits)


@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_dense_random_data_over_four_letters(torch_mod, codec, shape):
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b"abcd", np.uint8)
    enc = encode(torch_mod, codec, rng.choice(letters, n).astype(np.uint8), bs)
    for trial in range(6):
        alts = [[bytes(rng.choice(letters, int(rng.integers(1, 3)), replace=False).astype(np.uint8)) for _ in range(int(rng.integers(1, 7)))]
                for _ in range(int(rng.integers(1, 7)))]
        exact(torch_mod, codec, enc, alts, what=(shape, trial, alts))


def test_the_longer_alternative_reaches_a_block_that_is_not_served(torch_mod, codec):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    base = base_of("5x4099").copy()
    base[base == ord("a")] = ord("e")
    only_long, both = 2 * bs - 3, 3 * bs - 1                # `ab` ends inside block 1 / `ab` itself crosses into block 3
    data = planted(base, b"abcXY", [starts[1], only_long, both, 3 * bs + 100])
    enc = encode(torch, codec, data, bs)
    alts = [b"ab", b"abcXY"]
    total, _ = exact(torch, codec, enc, alts, must=[starts[1], only_long, both, 3 * bs + 100], what="all served")
    assert total == 4
    bad = damaged(enc, int(enc.h_offs[2]), 0x01)            # block 2's block_len: not the layout's
    res = psearch(torch, codec, bad, AnyOf(*alts), 9)
    assert res[2].tolist() == [OK, OK, RW, OK, OK]
    check(res, find_any_model(data, alts, bs, 9, served=res[2] == OK), 9, "block 2 is not served")
    assert res[0][LEAD:LEAD + 3].tolist() == [starts[1], only_long, 3 * bs + 100]      # the short one alone lies in served blocks
    res = psearch(torch, codec, bad, AnyOf(b"abcXY", b"ab"), 9)                          # ... in either order
    assert res[0][LEAD:LEAD + 3].tolist() == [starts[1], only_long, 3 * bs + 100] and int(res[1][0]) == 3
    bad = damaged(enc, int(enc.h_offs[3]), 0x01)            # block 3: at 3 bs - 1 BOTH alternatives reach it, the start is dropped
    res = psearch(torch, codec, bad, AnyOf(*alts), 9)
    assert res[2].tolist() == [OK, OK, OK, RW, OK]
    check(res, find_any_model(data, alts, bs, 9, served=res[2] == OK), 9, "block 3 is not served")
    assert res[0][LEAD:LEAD + 2].tolist() == [starts[1], only_long] and int(res[1][0]) == 2


# ---- one-symbol blocks -----------------------------------------------------------------------------------------------------
def test_one_symbol_blocks(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    for m0, m1 in ((5, 1), (5, 3), (2, 33), (33, 2), (1, 63), (31, 33)):
        without = [b"(*"] * m0                                                  # the leaf in no class of the first alternative
        with_leaf = [bytes([41, 40 + 3 * (k % 5)]) for k in range(m1)]          # ... and in every class of the second
        want = find_any_model(enc.data, [without, with_leaf], bs, n + 3)
        assert np.array_equal(want[0], np.arange(n - m1 + 1)) and want[1].tolist() == [bs] * 4 + [bs - m1 + 1]
        res = psearch(torch, codec, enc, AnyOf(without, with_leaf), n + 3)
        assert not res[2].any()
        check(res, want, n + 3, (m0, m1))
        for k in sorted({0, m1 // 2, m1 - 1}):                                  # ... in no alternative: one class of the second lacks it
            alts = [without, with_leaf[:k] + [b"(*"] + with_leaf[k + 1:]]
            res = psearch(torch, codec, enc, AnyOf(*alts), 4)
            assert not res[2].any() and res[1].tolist() == [0, 0, 0, 0], (m0, m1, k)
            check(res, find_any_model(enc.data, alts, bs, 4), 4, (m0, m1, k))


@pytest.mark.parametrize("bs", [4096, 4099])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs):
    torch = torch_mod
    data = mixed_blocks(bs, 6, 26)
    tail, head = pattern_below_255(6, 1), pattern_below_255(5, 2)
    out_of, into = b")" * 4 + tail, head + b")" * 3
    s_out, s_in = [bs - 4, 3 * bs - 4], [2 * bs - 5, 4 * bs - 5]
    data = planted(planted(data, out_of, s_out), into, s_in)
    enc = encode(torch, codec, data, bs)
    assert [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)] == [True, False] * 3
    paren = [b")("]
    alts = [paren * 4 + [bytes([c, c ^ 1]) for c in tail], [bytes([c, c ^ 1]) for c in head] + paren * 3, paren * 40]
    exact(torch, codec, enc, alts, must=s_out + s_in + [0, bs - 40, 2 * bs], must_not=[bs - 39], what="into, out of, inside")
    exact(torch, codec, enc, alts[:2], must=s_out + s_in, must_not=[0], what="into and out of")
    exact_or_not_served(torch, codec, enc, alts, 3 * bs, sub=torch.zeros_like(enc.sub), what="zeros")


# ---- damage ----------------------------------------------------------------------------------------------------------------
def damage_input(torch, codec):
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(30)
    lit = bytes((rng.integers(0, 2, 33) * 200 + 7).astype(np.uint8))
    classes = [bytes([v]) for v in lit]
    for k in (3, 17, 32):
        classes[k] = b"\x07\xcf"                           # either value
    starts = [0, 500, bs - 43, bs - 10, bs + 1000, bs + 2040, 2 * bs - 1, 2 * bs + 40, 2 * bs + 2030, 3 * bs - 33, 4 * bs - 5, n - 33]
    enc = encode(torch, codec, planted(two_values(n, 31), lit, starts), bs)
    return enc, [classes, classes[5:12], [ANY, classes[0], classes[1]]], starts


@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    torch = torch_mod
    enc, alts, starts = damage_input(torch, codec)
    bs, n = enc.bs, enc.n
    exact(torch, codec, enc, alts[:1] + alts[2:], must=starts, room=3, what="undamaged")
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for a, cap in ((alts, n), (alts[:1], 40), (alts[1:], n)):
            errs = exact_or_not_served(torch, codec, bad, a, cap, what=(damage, b, len(a)))
            assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
        # ONE record (no delimiter occurs): any block that is not served leaves its extent unknown
        errs = records_exact_or_not_served(torch, codec, bad, alts[:2] + [[NOT_NL] + alts[2][1:]], b"\n", 3, what=(damage, b, "records"))
        assert errs.tolist() == [RW if j == b else OK for j in range(5)]


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    words = [b"needle", b"pin", b"haystack"]
    nl = [50, 4000, bs + 7, 2 * bs - 1, 3 * bs, 4 * bs + 2047, 5 * bs + 100]
    at = [100, bs - 3, 2 * bs + 2045, 3 * bs + 1, 5 * bs + 1494]
    data = planted_each(with_delimiters(base_without(5 * bs + 1500, 31), nl), [words[i % 3] for i in range(len(at))], at)
    enc = encode(torch, codec, data, bs)
    alts = [[bytes([c, c ^ 0x20]) for c in w] for w in words]
    rng = np.random.default_rng(33)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    for a in (alts, alts[:2], [[NOT_NL] + alts[0][1:], alts[1]]):
        cap = int(find_any_model(data, a, bs)[2][0]) + 3
        assert not exact_or_not_served(torch, codec, enc, a, cap, what="own").any()
        errs = exact_or_not_served(torch, codec, enc, a, cap, sub=other, what=sub)
        assert sub == "random" or errs.all()                # (a bit count of 0 cannot be that of 32 codewords)
        assert not records_exact_or_not_served(torch, codec, enc, a, b"\n", cap, what="own").any()
        records_exact_or_not_served(torch, codec, enc, a, b"\n", cap, sub=other, max_len=9, what=sub)
    bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    exact_or_not_served(torch, codec, bad, alts, cap, sub=other, what=(sub, "and a damaged block"))
    records_exact_or_not_served(torch, codec, bad, alts, b"\n", cap, sub=other, what=(sub, "and a damaged block"))


# ---- the caps --------------------------------------------------------------------------------------------------------------
def test_caps(torch_mod, codec):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    words = [b"Warning", b"Oops"]
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000]
    starts = starts + [starts[1] + 20, n - 7]               # (two matches in one record)
    plants = [s for i in range(len(starts)) for s in spellings(words[i % 2], 1 + i, 4 + i)[-1:]]
    data = planted_each(with_delimiters(base_without(n, 71), nl), plants, starts)
    enc = encode(torch, codec, data, bs)
    model = [GpuCodec.byte_classes(w, ignore_case=True) for w in words]
    total = int(find_any_model(data, model, bs)[2][0])
    rtotal = int(find_any_records_model(data, model, b"\n", bs)[3][0])
    assert total == len(starts) and 2 < rtotal < total
    for cap in (0, 1, total - 1, total):
        for counts in (True, False):
            res = psearch(torch, codec, enc, AnyOf(*words), cap, counts=counts, ignore_case=True)        # (cap 0: d_pos is NULL)
            assert not res[2].any() and int(res[1][0]) == total
            check(res, find_any_model(data, model, bs, cap), cap, (cap, counts))
    for cap in (0, 1, rtotal - 1, rtotal):
        for counts in (True, False):
            res = rsearch(torch, codec, enc, AnyOf(*words), b"\n", cap, counts=counts, ignore_case=True)
            assert not res[3].any() and int(res[2][0]) == rtotal
            check(res, find_any_records_model(data, model, b"\n", bs, cap), cap, (cap, counts))
    totals, errs = codec.count_records(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, AnyOf(*words), ignore_case=True)
    assert totals.cpu().tolist() == [rtotal, 0, 0, 0] and not errs.cpu().numpy().any()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    for bad in (AnyOf(), AnyOf(*[b"x"] * 65), AnyOf(b"x" * 32, b"y" * 33), AnyOf(b"x", b""), AnyOf([1, b""])):
        with pytest.raises(ValueError):
            codec.find_pattern(*args, bad)
        with pytest.raises(ValueError):
            codec.find_records(*args, bad)
    with pytest.raises(ValueError, match="class 2 of alternative 1 holds a delimiter"):
        codec.find_records(*args, AnyOf(b"x", [b"a", b"b", ANY, b"c"]))
    with pytest.raises(ValueError, match="class 0 of alternative 0 "):
        codec.find_records(*args, AnyOf(b",x", b"y"), delimiters=b";,", ignore_case=True)
    codec.find_records(*args, AnyOf([b"a", ANY], b"b"), delimiters=b"")      # the empty delimiter set: valid


# ---- records ---------------------------------------------------------------------------------------------------------------
def test_records_at_the_seams(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    words = [b"error", b"fatal", b"panic!"]
    base = base_without(n, 41)
    # delimiters: a lane seam's two sides, a tile seam's two sides, two in a row, a block's last and its first byte, a 3-byte
    # tile's last two bytes, another block's first byte alone (tests/test_gpu_find_records.py)
    nl = [31, 32, 300, 2047, 2048, 2500, 2501, 3000, bs - 1, bs, 2 * bs + 100, 2 * bs + 4097, 3 * bs - 1, 3 * bs + 1500, 4 * bs, 4 * bs + 200]
    # record 0 holds error AND fatal, record 301 error twice and panic!, the others one alternative each
    plants = [(0, b"ERROR"), (12, b"fatal"), (301, b"Error"), (320, b"eRRor"), (350, b"PANIC!"), (2047 - 5, b"Fatal"), (bs + 2048 - 3, b"panic!"),
              (2 * bs - 3, b"FATAL"), (3 * bs + 1500 - 6, b"Panic!"), (4 * bs + 1, b"error"), (n - 5, b"fAtAl")]
    data = planted_each(with_delimiters(base, nl), [p for _, p in plants], [s for s, _ in plants])
    model = [GpuCodec.byte_classes(w, ignore_case=True) for w in words]
    enc = encode(torch, codec, data, bs)
    must = [0, 301, bs + 1, 3 * bs, 4 * bs + 1, 4 * bs + 201]
    pos, lens, _ = records_exact(torch, codec, enc, words, must=must, must_not=[33, 2 * bs + 101], model=model, ignore_case=True, what="no end")
    assert pos[-1] + lens[-1] == n and lens[0] == 31 and pos.tolist().count(0) == 1 and pos.tolist().count(301) == 1
    assert find_any_model(data, model, bs)[2][0] == len(plants) > pos.size
    wide = [[NOT_NL] + [bytes([c, c ^ 0x20]) for c in w[1:]] for w in words[:2]]
    records_exact(torch, codec, enc, wide, must=[301, bs + 1], must_not=[2502], what="a wide first class")
    for max_len in (1, 30, 31, 32, 5000):                  # below, at and above the lengths: totals[3]
        records_exact(torch, codec, enc, words, model=model, max_len=max_len, ignore_case=True, what=max_len)
    cut = [int(find_any_records_model(data, model, b"\n", bs, n, m)[3][3]) for m in (1, 31, 5000)]
    assert cut[0] > cut[1] >= cut[2] == 0
    data[n - 1] = 10                                       # a delimiter as the data's last byte, and one as its first
    data[n - 6:n - 1] = np.frombuffer(b"fAtAl", np.uint8)
    data[0] = 10
    data[1:6] = np.frombuffer(b"ERROr", np.uint8)
    enc = encode(torch, codec, data, bs)
    pos, lens, _ = records_exact(torch, codec, enc, words, must=[1, 4 * bs + 201], must_not=[0], model=model, ignore_case=True, what="an end")
    assert pos[-1] + lens[-1] == n - 1


@pytest.mark.parametrize("shape", ["300x64", "200x3"])
def test_one_record_over_all_blocks(torch_mod, codec, shape):
    """a match of one alternative or the other in every tile; the empty delimiter set and a delimiter that never occurs both
    give ONE entry, (0, n)"""
    bs, n, _ = FOUR_SHAPES[shape]
    base = base_without(n, 42)
    nb = (n + bs - 1) // bs
    alts = [[b"Qq", b"Zz"], [b"Xx", b"Yy"], [b"Q", b"Y", b"Z"]]
    data = planted_each(base, [b"qZ", b"Xy"] * nb, [b * bs for b in range(nb)])
    enc = encode(torch_mod, codec, data, bs)
    for delims in (b"", b"\n"):
        res = rsearch(torch_mod, codec, enc, AnyOf(*alts), delims, 3)
        assert res[2].tolist() == [1, 1, 0, 0] and not res[3].any(), (delims, res[2])
        assert res[0][LEAD] == 0 and int(res[1].view(np.uint32)[LEAD]) == n, delims
        check(res, find_any_records_model(data, alts, delims, bs, 3), 3, delims)
        assert res[4].tolist() == [1] + [0] * (nb - 1)
    res = rsearch(torch_mod, codec, enc, AnyOf([ANY, b"Zz"], [b"y"]), b"", 3)   # the full class with the empty delimiter set
    check(res, find_any_records_model(data, [[ANY, b"Zz"], [b"y"]], b"", bs, 3), 3, "any")


def test_grep_any_of_ignore_case(torch_mod, codec):
    """grep(AnyOf(...), ignore_case=True) without a synchronisation, against an `re` filter over the split lines"""
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
    want = [l for l in lines if re.search(rb"error|heartbeat|timed out", l, re.IGNORECASE)]
    one = [l for l in lines if re.search(rb"error", l, re.IGNORECASE)]
    assert 0 < len(one) < len(want) < n // 20
    enc = encode(torch, codec, data, bs)
    cap, width = len(want) + 5, 256
    rows, raws, gerrs, totals, block_errs = codec.grep(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs,
                                                       AnyOf(b"error", b"HeartBeat", b"Timed Out"), cap, width, ignore_case=True)
    rows, raws, gerrs, totals, block_errs = (x.cpu().numpy() for x in (rows, raws, gerrs, totals, block_errs))
    assert totals.tolist() == [len(want), len(want), 0, sum(len(l) > width for l in want)] and not block_errs.any() and not gerrs.any()
    assert not raws[len(want):].any()
    for i, line in enumerate(want):
        assert raws[i] == min(len(line), width) and bytes(rows[i, :raws[i]]) == line[:width], i


# ---- one context, call after call --------------------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """find_pattern, a class call, an any-of call, find_records with an AnyOf, find_bytes - and the first two once more -
    without a synchronise in between: each gives its own model's answer, and the older calls the same after an any-of call
    as before it"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    words = [b"Segfault", b"abort"]
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000]
    plants = [spellings(words[i % 2], 2 + i, 5 + i)[-1] for i in range(len(starts))]
    plants[0], plants[2] = b"segfault", b"segfault"
    data = planted_each(with_delimiters(base_without(n, 72), nl), plants, starts)
    enc = encode(torch, codec, data, bs)
    lower = words[0].lower()
    classes = GpuCodec.byte_classes(words[0], ignore_case=True)
    alts = [GpuCodec.byte_classes(w, ignore_case=True) for w in words]
    v = int(np.bincount(data).argmax())
    jobs = [("pattern", lower), ("classes", words[0]), ("any", AnyOf(*words)), ("any records", AnyOf(*words)), ("bytes", [v]),
            ("pattern", lower), ("classes", words[0])]

    def model(kind, cap):
        if kind == "pattern":
            return find_pattern_model(data, lower, bs, cap)
        if kind == "classes":
            return find_classes_model(data, classes, bs, cap)
        if kind == "any":
            return find_any_model(data, alts, bs, cap)
        if kind == "bytes":
            return find_model(data, [v], bs, cap)
        return find_any_records_model(data, alts, b"\n", bs, cap)

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
                                          ignore_case=True))
        elif kind == "bytes":
            res.append(codec.find_bytes(*args, key, max_positions=cap, block_counts=True, out=pbuf[LEAD:LEAD + cap]))
        else:
            res.append(codec.find_pattern(*args, key, max_positions=cap, block_counts=True, out=pbuf[LEAD:LEAD + cap], ignore_case=kind != "pattern"))
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
    assert same_arrays(host[0], host[5]) and same_arrays(host[1], host[6])
    assert int(host[2][1][0]) > int(host[1][1][0]) > int(host[0][1][0]) > 0     # any-of sees both words, the class call all spellings of one


def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    pos, totals, errs, cnt = codec.find_pattern(empty, 0, offsets, 0, sub, 0, 4096, AnyOf(b"error", b"fatal"), max_positions=4,
                                                block_counts=True, out=buf, ignore_case=True)
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    _, _, totals, errs, cnt = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, AnyOf([b"eE", b"rR"], b"x"), max_records=4,
                                                 block_counts=True, out=(buf, lbuf))
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4

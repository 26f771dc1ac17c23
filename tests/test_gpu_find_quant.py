"""GPU tests of hufgpu_find_any_quant and hufgpu_find_records_quant (GpuCodec.Opt / Rep / regex as the `pattern` of
find_pattern / find_records / grep): patterns with OPTIONAL positions - grep -E 'colou?r', '[0-9]{1,3}' - found in one walk of
the stream, straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the models of tests/find_quant_model.py (themselves checked against
Python's `re` in tests/test_find_quant_args.py).  As in tests/test_gpu_find.py every output buffer has guard words in front and
behind and is filled with the guard first: the words beyond totals[1] must still hold it.  The four shapes are those of
tests/test_gpu_find_classes.py: five blocks of 4 099 bytes (tiles of 2 048, 2 048 and 3 symbols), 300 blocks of 64 bytes (two
scan groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes (three chunks).
"""
import re

import numpy as np
import pytest

from find_any_model import find_any_model
from find_classes_model import find_classes_model
from find_context_model import find_context_model
from find_model import find_model
from find_pattern_model import find_pattern_model
from find_quant_model import find_quant_model, find_quant_records_model
from find_quant_support import POS_NAME, REC_NAME, O, forms, lit, quant_call, rep
from find_support import (FOUR_SHAPES, LEAD, OK, RW, TILE_END, answer_or_not_served, base_of, base_without, check, codec, context,  # noqa: F401
                          damaged, encode, exact_answer, find, find_call, mixed_blocks, payload_start, planted, planted_each, positions_of,
                          psearch, same_arrays, torch_mod, two_values, with_delimiters)
from libhuffman_amd.codec import GpuCodec

pytestmark = pytest.mark.gpu

Opt, Rep = GpuCodec.Opt, GpuCodec.Rep
LETTERS = b"abcdex"


# ---- checks ----------------------------------------------------------------------------------------------------------------
def pos_call(torch, codec, enc, alts, cap, **kw):
    return positions_of(quant_call(torch, codec, enc, POS_NAME, alts, cap, **kw))


def rec_call(torch, codec, enc, alts, cap, **kw):
    return quant_call(torch, codec, enc, REC_NAME, alts, cap, **kw)


def exact(torch, codec, enc, alts, must=(), must_not=(), room=7, what=""):
    """all blocks served and everything equal to the model; returns (the total, the call's host arrays)"""
    full, res, _ = exact_answer(lambda cap: pos_call(torch, codec, enc, alts, cap),
                                lambda cap, served: find_quant_model(enc.data, alts, enc.bs, cap, served), enc.n, must, must_not, room, what,
                                total_in=(1, enc.n - 1))
    return int(full[2][0]), res


def exact_or_not_served(torch, codec, enc, alts, cap, sub=None, what=""):
    return answer_or_not_served(lambda cap: pos_call(torch, codec, enc, alts, cap, sub=sub),
                                lambda cap, served: find_quant_model(enc.data, alts, enc.bs, cap, served), cap, what)


def records_exact_or_not_served(torch, codec, enc, alts, delims, cap, sub=None, what="", **kw):
    return answer_or_not_served(lambda cap: rec_call(torch, codec, enc, alts, cap, delims=delims, sub=sub, **kw),
                                lambda cap, served: find_quant_records_model(enc.data, alts, delims, enc.bs, cap, 0, served, **kw), cap, what)


def scrubbed(shape, letters=LETTERS):
    """the shape's base without the letters that the patterns are made of: only what is planted matches"""
    data = base_of(shape).copy()
    data[np.isin(data, list(letters))] = ord("z")
    return data


# ---- identities, in the same process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_without_an_optional_position_the_calls_are_the_older_ones(torch_mod, codec, shape):
    """`optional` NULL and all zeros: hufgpu_find_any and hufgpu_find_records_context, word for word"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    words = [b"abc", b"dexab", b"x"]
    data = planted_each(scrubbed(shape), [words[i % 3] for i in range(len(starts))], starts)
    data[data == 10] = 11
    data[[s + 9 for s in starts[::2]]] = 10
    enc = encode(torch, codec, data, bs)
    alts = [lit(w) for w in words]
    want = find_any_model(data, alts, bs, n)
    cap = int(want[2][0]) + 5
    older = positions_of(find_call(torch, codec, enc, "find_any", alts, cap))
    check(older, find_any_model(data, alts, bs, cap), cap, shape)
    for optional in (None, bytes(9)):
        assert same_arrays(pos_call(torch, codec, enc, alts, cap, optional=optional), older), (shape, optional)
    for kw in (dict(), dict(invert=True), dict(before=1, after=2), dict(before=0, after=0, numbers=False, flags=False)):
        older = context(torch, codec, enc, alts, b"\n", 9, max_len=7, **kw)
        check(older, find_context_model(data, alts, b"\n", bs, 9, 7, **{k: v for k, v in kw.items() if k in ("invert", "before", "after")}), 9, kw)
        for optional in (None, bytes(9)):
            assert same_arrays(rec_call(torch, codec, enc, alts, 9, max_len=7, optional=optional, **kw), older), (shape, kw, optional)


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_optional_letters_are_the_any_of_call_over_the_written_out_forms(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    alts = [lit(b"colour", (4,)), lit(b"https://", (4,)), lit(b"gray", (2,)) + lit(b"sh", (0, 1))]
    words = [b"color", b"colour", b"http://", b"https://", b"gry", b"grays", b"grysh", b"colouur"]
    for rot in range(3):
        at = [max(s - (i + rot) % 4, 0) for i, s in enumerate(starts)]
        data = planted_each(base_of(shape), [words[(i + rot) % len(words)] for i in range(len(starts))], at)
        enc = encode(torch, codec, data, bs)
        total, res = exact(torch, codec, enc, alts, must=[a for i, a in enumerate(at) if (i + rot) % len(words) != 7], what=(shape, rot))
        written = forms(alts)
        assert len(written) == 2 + 2 + 8 and sum(len(f) for f in written) <= 64
        assert same_arrays(res, positions_of(find_call(torch, codec, enc, "find_any", written, total + 7))), (shape, rot)


# ---- every seam ------------------------------------------------------------------------------------------------------------
SEAM_PATTERNS = {"ab?c": ([lit(b"abc", (1,))], [b"abc", b"ac", b"abbc", b"ab"]),
                 "a?b": ([lit(b"ab", (0,))], [b"ab", b"b", b"aab", b"a"]),
                 "ab?": ([lit(b"ab", (1,))], [b"ab", b"a", b"abb", b"b"]),
                 "ab?c?d?e": ([lit(b"abcde", (1, 2, 3))], [b"abcde", b"ae", b"abe", b"ace", b"ade", b"abde", b"acde", b"abce", b"abcd", b"aee"]),
                 "x{2,5}": ([rep(b"x", 2, 5)], [b"x" * r for r in range(1, 8)])}


@pytest.mark.parametrize("name", list(SEAM_PATTERNS))
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_every_seam(torch_mod, codec, shape, name):
    """every form, and strings that are none, across every lane, tile, chunk and block seam of the shape at every split: the
    plants rotate through the starts and move back byte by byte; the shortest form right in front of a tile's end, where the
    longest does not fit; at n - len_short, where the longest would pass raw_size; nothing at n - len_min + 1"""
    bs, n, starts = FOUR_SHAPES[shape]
    alts, plants = SEAM_PATTERNS[name]
    short = min(forms(alts), key=len)
    short = b"".join(short)
    longest = max(len(a) for a in alts)
    for rot in range(max(longest, 4)):
        at = [max(s + 1 - (i + rot) % (longest + 1), 0) for i, s in enumerate(starts)]
        data = planted_each(scrubbed(shape), [plants[(i + rot) % len(plants)] for i in range(len(starts))], at)
        data = planted(data, short, [TILE_END[shape] - len(short), n - len(short)])
        enc = encode(torch_mod, codec, data, bs)
        exact(torch_mod, codec, enc, alts, must=[TILE_END[shape] - len(short), n - len(short)], what=(shape, name, rot))
    data = planted(scrubbed(shape), b"z" * longest + short, [n - longest - len(short) + 1])     # cut: its last byte is not there
    enc = encode(torch_mod, codec, planted(data, short, starts[:1]), bs)
    exact(torch_mod, codec, enc, alts, must=starts[:1], must_not=[n - len(short) + 1] if name != "x{2,5}" and len(short) > 1 else [],
          what=(shape, name, "cut"))


@pytest.mark.parametrize("required", [0, 31, 63])
def test_64_positions_and_one_required_over_blocks_of_3_bytes(torch_mod, codec, required):
    bs, n, _ = FOUR_SHAPES["200x3"]
    data = base_of("200x3")
    top = np.argsort(np.bincount(data, minlength=256))[::-1]
    wide = bytes(sorted(int(v) for v in top[1:40]))
    alt = [bytes([int(top[0])]) if k == required else O(wide) for k in range(64)]
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, [alt], must=np.flatnonzero(data == top[0]).tolist(), what=required)


# ---- the layout of the state -------------------------------------------------------------------------------------------------
def four_letters(torch, codec, shape, seed):
    bs, n, _ = FOUR_SHAPES[shape]
    return encode(torch, codec, np.random.default_rng(seed).choice(np.frombuffer(b"abcd", np.uint8), n).astype(np.uint8), bs)


def narrow(rng, m, flags):
    """classes of two or three of the four letters; in a long alternative, so that it occurs, three of them at every fourth
    position and at the optional ones, and all four elsewhere"""
    letters = np.frombuffer(b"abcd", np.uint8)
    sizes = [int(rng.integers(2, 4)) if m <= 8 else 3 if k % 4 == 0 or flags[k] else 4 for k in range(m)]
    return [O(c) if f else c for c, f in zip([bytes(rng.choice(letters, size, replace=False)) for size in sizes], flags)]


@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_the_layout_of_the_state(torch_mod, codec, shape):
    enc = four_letters(torch_mod, codec, shape, 81)
    rng = np.random.default_rng(82)
    run = lambda m, lo, hi: [lo <= k < hi for k in range(m)]             # noqa: E731
    cases = {
        "an alternative across bits 31 / 32, an optional run over that edge": [narrow(rng, 28, run(28, 0, 0)), narrow(rng, 10, run(10, 2, 7))],
        "one alternative across the edge, the run on it": [narrow(rng, 40, run(40, 29, 35))],
        "a run at the low end of alternative 0 right above alternative 1's start": [narrow(rng, 6, run(6, 3, 6)), narrow(rng, 5, run(5, 1, 2))],
        "... and alternative 1 starting with a run": [narrow(rng, 6, run(6, 3, 6)), narrow(rng, 5, run(5, 0, 3))],
        "the reverse order": [narrow(rng, 5, run(5, 0, 3)), narrow(rng, 6, run(6, 3, 6))],
        "a total of exactly 64, runs at bit 63 and at bit 0": [narrow(rng, 30, run(30, 0, 4)), narrow(rng, 4, run(4, 1, 2)), narrow(rng, 30, run(30, 25, 30))],
        "64 alternatives of one position": [[bytes([v])] for v in b"ab"] * 32,
        "32 of two, each with a flag": [[O(b"c"), b"a"], [b"b", O(b"d")]] * 16,
    }
    for what, alts in cases.items():
        assert sum(len(a) for a in alts) <= 64
        exact(torch_mod, codec, enc, alts, what=(shape, what))


@pytest.mark.parametrize("shape", ["5x4099", "300x64", "200x3"])
def test_dense_random_data_over_four_letters(torch_mod, codec, shape):
    enc = four_letters(torch_mod, codec, shape, 77)
    rng = np.random.default_rng(78)
    for trial in range(8):
        alts = []
        for _ in range(int(rng.integers(1, 7))):
            m = int(rng.integers(2, 9))
            flags = [bool(rng.integers(0, 2)) for _ in range(m)]
            for k in rng.choice(m, 2, replace=False):       # two required positions at least: no set of alternatives lies everywhere
                flags[k] = False
            classes = [bytes(rng.choice(np.frombuffer(b"abcd", np.uint8), int(rng.integers(1, 3)), replace=False)) for _ in range(m)]
            alts.append([O(c) if f else c for c, f in zip(classes, flags)])
        exact(torch_mod, codec, enc, alts, what=(shape, trial, alts))


# ---- blocks that are not served ------------------------------------------------------------------------------------------------
def test_the_longer_form_reaches_a_block_that_is_not_served(torch_mod, codec):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    only_long, both = 2 * bs - 3, 3 * bs - 1                # `ab` ends inside block 1 / `ab` itself crosses into block 3
    data = planted(scrubbed("5x4099"), b"abcde", [starts[1], only_long, both, 3 * bs + 100])
    enc = encode(torch, codec, data, bs)
    alts = [lit(b"abcde", (2, 3, 4))]
    total, _ = exact(torch, codec, enc, alts, must=[starts[1], only_long, both, 3 * bs + 100], what="all served")
    assert total == 4
    bad = damaged(enc, int(enc.h_offs[2]), 0x01)            # block 2's block_len: not the layout's
    res = pos_call(torch, codec, bad, alts, 9)
    assert res[2].tolist() == [OK, OK, RW, OK, OK]
    check(res, find_quant_model(data, alts, bs, 9, served=res[2] == OK), 9, "block 2 is not served")
    assert res[0][LEAD:LEAD + 3].tolist() == [starts[1], only_long, 3 * bs + 100]      # the short form alone lies in served blocks
    bad = damaged(enc, int(enc.h_offs[3]), 0x01)            # block 3: at 3 bs - 1 every form reaches it, the start is dropped
    res = pos_call(torch, codec, bad, alts, 9)
    assert res[2].tolist() == [OK, OK, OK, RW, OK]
    check(res, find_quant_model(data, alts, bs, 9, served=res[2] == OK), 9, "block 3 is not served")
    assert res[0][LEAD:LEAD + 2].tolist() == [starts[1], only_long] and int(res[1][0]) == 2


def damage_input(torch, codec):
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(30)
    word = bytes((rng.integers(0, 2, 33) * 200 + 7).astype(np.uint8))
    alt = lit(word, (1, 2, 16, 30, 31, 32))
    for k in (3, 17):
        alt[k] = b"\x07\xcf"                                # either value
    starts = [0, 500, bs - 43, bs - 10, bs + 1000, bs + 2040, 2 * bs - 1, 2 * bs + 40, 2 * bs + 2030, 3 * bs - 33, 4 * bs - 5, n - 33]
    enc = encode(torch, codec, planted(two_values(n, 31), word, starts), bs)
    return enc, [alt, lit(word[5:12], (0, 6)), [O(b"\x07"), alt[0], O(b"\xcf"), alt[1][0]]], starts


@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    torch = torch_mod
    enc, alts, starts = damage_input(torch, codec)
    bs, n = enc.bs, enc.n
    exact(torch, codec, enc, alts[:1], must=starts, room=3, what="undamaged")
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for a, cap in ((alts, n), (alts[:1], 40), (alts[1:], n)):
            errs = exact_or_not_served(torch, codec, bad, a, cap, what=(damage, b, len(a)))
            assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
        errs = records_exact_or_not_served(torch, codec, bad, alts, b"\n", 3, what=(damage, b, "records"))     # ONE record
        assert errs.tolist() == [RW if j == b else OK for j in range(5)]


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    words = [b"needle", b"pin", b"haystack", b"nedle", b"hastck"]
    nl = [50, 4000, bs + 7, 2 * bs - 1, 3 * bs, 4 * bs + 2047, 5 * bs + 100]
    at = [100, bs - 3, 2 * bs + 2045, 3 * bs + 1, 5 * bs + 1494, 4 * bs - 2, 4 * bs + 2046]
    data = planted_each(with_delimiters(base_without(5 * bs + 1500, 31), nl), [words[i % 5] for i in range(len(at))], at)
    enc = encode(torch, codec, data, bs)
    alts = [lit(b"needle", (2,)), lit(b"pin", (2,)), lit(b"haystack", (2, 5))]
    rng = np.random.default_rng(33)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    cap = int(find_quant_model(data, alts, bs)[2][0]) + 3
    assert not exact_or_not_served(torch, codec, enc, alts, cap, what="own").any()
    errs = exact_or_not_served(torch, codec, enc, alts, cap, sub=other, what=sub)
    assert sub == "random" or errs.all()                    # (a bit count of 0 cannot be that of 32 codewords)
    assert not records_exact_or_not_served(torch, codec, enc, alts, b"\n", cap, what="own").any()
    records_exact_or_not_served(torch, codec, enc, alts, b"\n", cap, sub=other, what=sub)
    bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    exact_or_not_served(torch, codec, bad, alts, cap, sub=other, what=(sub, "and a damaged block"))
    records_exact_or_not_served(torch, codec, bad, alts, b"\n", cap, sub=other, what=(sub, "and a damaged block"), before=1, after=1)


# ---- one-symbol blocks -----------------------------------------------------------------------------------------------------
def test_one_symbol_blocks(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    leaf, other = b")(", b"(*"
    for m, optional in ((1, ()), (5, (1, 3)), (33, (0, 1, 2, 30, 31, 32)), (64, tuple(range(1, 64))), (64, tuple(range(63)))):
        with_leaf = [O(leaf) if k in optional else leaf for k in range(m)]                  # the leaf in every class
        shortest = m - len(optional)
        both = ([[other] * 3] if m < 64 else []) + [with_leaf]                             # the leaf in no class of the first alternative
        want = find_quant_model(enc.data, both, bs, n + 3)
        assert np.array_equal(want[0], np.arange(n - shortest + 1))
        res = pos_call(torch, codec, enc, both, n + 3)
        assert not res[2].any()
        check(res, want, n + 3, (m, optional))
        required = [k for k in range(m) if k not in optional]
        for k in sorted({required[0], required[-1]}):                                       # ... but in one required class: no start
            alts = [with_leaf[:k] + [other] + with_leaf[k + 1:]]
            res = pos_call(torch, codec, enc, alts, 4)
            assert not res[2].any() and res[1].tolist() == [0, 0, 0, 0], (m, optional, k)
        for k in optional[:1]:                                                              # ... but in one optional class: still every start
            alts = [with_leaf[:k] + [O(other)] + with_leaf[k + 1:]]
            check(pos_call(torch, codec, enc, alts, 4), find_quant_model(enc.data, alts, bs, 4), 4, (m, optional, k, "optional"))
    only_optional = [other, O(leaf), O(leaf)]                                               # the leaf in optional classes only
    res = pos_call(torch, codec, enc, [only_optional], 4)
    assert not res[2].any() and res[1].tolist() == [0, 0, 0, 0]
    check(pos_call(torch, codec, enc, [[O(other), leaf, O(other)]], n + 3), find_quant_model(enc.data, [[leaf]], bs, n + 3), n + 3, "skipped")


@pytest.mark.parametrize("bs", [4096, 4099])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs):
    torch = torch_mod
    data = mixed_blocks(bs, 6, 26)
    data[np.isin(data, list(b"abcdef"))] = ord("z")
    out_of, into = b"))))abdef", b"abcf)))"                   # forms of the two alternatives below
    s_out, s_in = [bs - 4, 3 * bs - 4], [2 * bs - 4, 4 * bs - 5]
    data = planted(planted(data, out_of, s_out), into, s_in)
    enc = encode(torch, codec, data, bs)
    assert [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)] == [True, False] * 3
    paren = b")("
    alts = [[paren, O(paren), paren, paren] + lit(b"abcdef", (2, 4)), lit(b"abcdf", (2, 3)) + [paren, paren, O(paren), O(paren)],
            [paren] * 38 + [O(paren)] * 2]
    exact(torch, codec, enc, alts, must=s_out + s_in + [0, bs - 38, 2 * bs, bs - 3], must_not=[bs - 37, bs - 2],
          what="into, out of, inside")
    exact(torch, codec, enc, alts[:2], must=s_out + s_in, must_not=[0], what="into and out of")
    exact_or_not_served(torch, codec, enc, alts, 3 * bs, sub=torch.zeros_like(enc.sub), what="zeros")


# ---- the caps and the records ------------------------------------------------------------------------------------------------
def log_input(torch, codec):
    bs, n, starts = FOUR_SHAPES["5x4099"]
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000, 3 * bs + 3001, 4 * bs + 9]
    starts = starts + [starts[1] + 20, n - 10]              # (two forms in one record)
    words = [b"took 5ms", b"took 12345ms", b"color", b"colour", b"took 123456ms", b"took ms"]
    data = planted_each(with_delimiters(base_without(n, 71), nl), [words[i % len(words)] for i in range(len(starts))], starts)
    return encode(torch, codec, data, bs), [lit(b"took ") + rep(b"0123456789", 1, 5) + lit(b"ms"), lit(b"colour", (4,))], starts


def test_caps(torch_mod, codec):
    torch = torch_mod
    enc, alts, starts = log_input(torch, codec)
    total = int(find_quant_model(enc.data, alts, enc.bs)[2][0])
    rtotal = int(find_quant_records_model(enc.data, alts, b"\n", enc.bs)[3][0])
    assert total == sum(i % 6 < 4 for i in range(len(starts))) and 2 < rtotal < total     # a line with two forms: once
    for cap in (0, 1, total - 1, total):
        for counts in (True, False):
            res = pos_call(torch, codec, enc, alts, cap, counts=counts)                     # (cap 0: d_pos is NULL)
            assert not res[2].any() and int(res[1][0]) == total
            check(res, find_quant_model(enc.data, alts, enc.bs, cap), cap, (cap, counts))
    for cap in (0, 1, rtotal - 1, rtotal):
        for counts in (True, False):
            res = rec_call(torch, codec, enc, alts, cap, counts=counts, numbers=bool(cap % 2), flags=False)
            assert not res[3].any() and int(res[2][0]) == rtotal
            want = find_quant_records_model(enc.data, alts, b"\n", enc.bs, cap)
            check(res, want[:5] if cap % 2 else want[:4], cap, (cap, counts))


@pytest.mark.parametrize("kw", [dict(), dict(invert=True), dict(before=2, after=2), dict(invert=True, before=2, after=2), dict(before=0, after=2),
                                dict(max_len=6)], ids=str)
def test_records_invert_numbers_and_context(torch_mod, codec, kw):
    torch = torch_mod
    enc, alts, _ = log_input(torch, codec)
    max_len = kw.pop("max_len", 0)
    full = find_quant_records_model(enc.data, alts, b"\n", enc.bs, enc.n, max_len, **kw)
    total = int(full[3][0])
    assert total > 2
    for cap in (total + 3, total - 1):
        res = rec_call(torch, codec, enc, alts, cap, max_len=max_len, **kw)
        assert not res[3].any()
        check(res, find_quant_records_model(enc.data, alts, b"\n", enc.bs, cap, max_len, **kw), cap, (kw, cap))


def test_the_python_layer(torch_mod, codec):
    """Opt / Rep / regex through find_pattern, count_pattern, find_records, count_records and grep - the last without a
    synchronisation, against an `re` filter of the lines"""
    torch = torch_mod
    enc, alts, _ = log_input(torch, codec)
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
    expr = rb"took [0-9]{1,5}ms|colou?r"
    pattern = GpuCodec.regex(expr)
    by_hand = GpuCodec.AnyOf(list(b"took ") + [Rep(b"0123456789", 1, 5), ord("m"), ord("s")], list(b"colo") + [Opt(b"u"), ord("r")])
    want = find_quant_model(enc.data, alts, enc.bs, enc.n)
    total = int(want[2][0])
    assert want[0].tolist() == [m.start() for m in re.finditer(b"(?=(?:" + expr + b"))", bytes(enc.data))]
    for p in (pattern, by_hand):
        check(psearch(torch, codec, enc, p, total + 2), find_quant_model(enc.data, alts, enc.bs, total + 2), total + 2, "find_pattern")
        totals, errs = codec.count_pattern(*args, p)
        assert totals.cpu().tolist() == [total, 0, 0, 0] and not errs.cpu().numpy().any()
    lines = bytes(enc.data).split(b"\n")
    keep = [ln for ln in lines if re.search(expr, ln)]
    totals, errs = codec.count_records(*args, pattern)
    assert totals.cpu().tolist() == [len(keep), 0, 0, 0]
    rows, width = len(keep) + 2, 300
    out = codec.grep(*args, pattern, rows, width, line_numbers=True)                         # enqueue-only: read back below
    got, raw_lens, gerrs, totals, berrs, numbers = [t.cpu().numpy() for t in out]
    assert totals.tolist()[:3] == [len(keep), len(keep), 0] and not berrs.any() and not gerrs.any()
    assert [bytes(got[i, :raw_lens[i]]) for i in range(len(keep))] == [ln[:width] for ln in keep]
    assert numbers[:len(keep)].tolist() == [i for i, ln in enumerate(lines) if re.search(expr, ln)]
    out = codec.grep(*args, pattern, rows + 40, width, invert=True, context=1)
    want = find_quant_records_model(enc.data, alts, b"\n", enc.bs, rows + 40, width, invert=True, before=1, after=1)
    assert out[3].cpu().tolist() == want[3].tolist() and out[5].cpu().numpy()[:want[5].size].tolist() == want[5].tolist()
    for bad in (dict(bol=True), dict(word=True), dict(whole_line=True)):
        with pytest.raises(ValueError, match="do not go with Opt / Rep"):
            codec.find_records(*args, pattern, **bad)
        with pytest.raises(ValueError, match="do not go with Opt / Rep"):
            codec.find_pattern(*args, pattern, **bad)
    with pytest.raises(ValueError, match="holds an Opt or a Rep"):
        codec.find_records(*args, GpuCodec.AllOf(b"took", pattern))


# ---- one context -----------------------------------------------------------------------------------------------------------
def test_calls_back_to_back_on_one_context(torch_mod, codec):
    """a quant call between a literal call, a class call, an any-of call, a context call and find_bytes: each gives its own
    model's answer, and the older ones give the same after as before"""
    torch = torch_mod
    enc, alts, _ = log_input(torch, codec)
    data, bs, n = enc.data, enc.bs, enc.n
    classes = [b"cC", b"o", b"l", b"o"]
    anyof = [lit(b"took"), lit(b"color")]

    def older():
        return [psearch(torch, codec, enc, b"took ", 40), psearch(torch, codec, enc, classes, 40),
                positions_of(find_call(torch, codec, enc, "find_any", anyof, 40)),
                context(torch, codec, enc, anyof, b"\n", 40, before=1, after=1), find(torch, codec, enc, b"\n", 40)]

    def quant():
        res = pos_call(torch, codec, enc, alts, 40)
        check(res, find_quant_model(data, alts, bs, 40), 40, "quant")
        res = rec_call(torch, codec, enc, alts, 40, before=1)
        check(res, find_quant_records_model(data, alts, b"\n", bs, 40, before=1), 40, "quant records")

    quant()
    before = older()
    for res, want in zip(before, (find_pattern_model(data, b"took ", bs, 40), find_classes_model(data, classes, bs, 40),
                                  find_any_model(data, anyof, bs, 40), find_context_model(data, anyof, b"\n", bs, 40, before=1, after=1),
                                  find_model(data, b"\n", bs, 40))):
        check(res, want, 40, "older")
    quant()
    for a, b in zip(before, older()):
        assert same_arrays(a, b)
    quant()

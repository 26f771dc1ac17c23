"""GPU tests of hufgpu_find_any_expr and hufgpu_find_records_expr (GpuCodec.Expr / egrep as the `pattern` of find_pattern /
find_records / grep): anchors, terms and optional positions TOGETHER - '^[0-9]{1,3}\\.', grep -w 'colou?r', '^A.*B{1,5}$' - in one
call, straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values come from the models of tests/find_expr_model.py (themselves checked against
Python's `re` in tests/test_find_expr_args.py).  As in tests/test_gpu_find.py every output buffer has guard words in front and
behind and is filled with the guard first: the words beyond totals[1] must still hold it.  The four shapes are those of
tests/find_support.py: five blocks of 4 099 bytes (tiles of 2 048, 2 048 and 3 symbols), 300 blocks of 64 bytes (two scan
groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes (three chunks).  On an undamaged stream with its own
sub-index every block must be served: totals[2] == 0 is part of every exact check.
"""
import re

import numpy as np
import pytest

from find_any_model import find_any_model
from find_context_model import find_context_model
from find_expr_model import ALL, BOL, EOL, ORDERED, WORD, find_any_expr_model, find_records_expr_model
from find_expr_support import POS_NAME, REC_NAME, O, expr_call, lit, rep
from find_quant_support import forms, quant_call
from find_support import (FOUR_SHAPES, LEAD, OK, RW, SEAMS, TILE, TILE_END, W, answer_or_not_served, base_of, check, codec, context,  # noqa: F401
                          damaged, encode, exact_answer, find, find_call, payload_start, planted, planted_each, positions, positions_of,
                          psearch, records, same_arrays, seven, torch_mod)
from find_terms_support import terms_call
from libhuffman_amd.codec import GpuCodec

pytestmark = pytest.mark.gpu

Opt, Rep, Expr = GpuCodec.Opt, GpuCodec.Rep, GpuCodec.Expr
NL = b"\n"
EACH_ANCHOR = [BOL, EOL, BOL | EOL, WORD]
NAMES = {BOL: "bol", EOL: "eol", BOL | EOL: "x", WORD: "word"}


# ---- checks ----------------------------------------------------------------------------------------------------------------
def pos_call(torch, codec, enc, alts, anchors, cap, **kw):
    return positions_of(expr_call(torch, codec, enc, POS_NAME, [alts], cap, anchors=anchors, **kw))


def rec_call(torch, codec, enc, terms, anchors, mode, cap, **kw):
    return expr_call(torch, codec, enc, REC_NAME, terms, cap, anchors=anchors, mode=mode, **kw)


def exact(torch, codec, enc, alts, anchors, must=(), must_not=(), at_least=1, what=""):
    """the positions call and the one-term records call: all blocks served and everything equal to the models"""
    full, res, _ = exact_answer(lambda cap: pos_call(torch, codec, enc, alts, anchors, cap),
                                lambda cap, served: find_any_expr_model(enc.data, alts, NL, W, anchors, enc.bs, cap, served), enc.n, must,
                                must_not, 7, what)
    assert int(full[2][0]) >= at_least and int(res[1][2]) == 0, (what, full[2])
    exact_records(torch, codec, enc, [alts], anchors, ORDERED, what=what)
    return int(full[2][0]), res


def exact_records(torch, codec, enc, terms, anchors, mode, must=(), must_not=(), at_least=0, what="", **kw):
    full, res, _ = exact_answer(lambda cap: rec_call(torch, codec, enc, terms, anchors, mode, cap, **kw),
                                lambda cap, served: find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, cap, 0, served, **kw),
                                enc.n, must, must_not, 7, what)
    assert int(full[3][0]) >= at_least and int(res[2][2]) == 0, (what, full[3])
    return full, res


def pos_or_not_served(torch, codec, enc, alts, anchors, cap, sub=None, what=""):
    return answer_or_not_served(lambda cap: pos_call(torch, codec, enc, alts, anchors, cap, sub=sub),
                                lambda cap, served: find_any_expr_model(enc.data, alts, NL, W, anchors, enc.bs, cap, served), cap, what)


def rec_or_not_served(torch, codec, enc, terms, anchors, mode, cap, sub=None, what="", **kw):
    return answer_or_not_served(lambda cap: rec_call(torch, codec, enc, terms, anchors, mode, cap, sub=sub, **kw),
                                lambda cap, served: find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, cap, 0, served, **kw),
                                cap, what)


def scrubbed(shape, letters=b"abcdex"):
    """the shape's base without the letters that the patterns are made of: only what is planted matches"""
    data = base_of(shape).copy()
    data[np.isin(data, list(letters))] = ord("z")
    return data


def dense(n, seed):
    """four letters, a byte that is no word byte, and lines"""
    return np.random.default_rng(seed).choice(np.frombuffer(b"abcd \n", np.uint8), n, p=[0.22, 0.22, 0.2, 0.16, 0.1, 0.1]).astype(np.uint8)


def all_starts(shape):
    return sorted(set(FOUR_SHAPES[shape][2] + SEAMS[shape] + [TILE_END[shape]]))


# ---- identities, in the same process ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_the_three_identities(torch_mod, codec, shape):
    """one dimension at a time the calls give what the older calls give, word for word, every output and guard word"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    words = [b"\nabc ", b" dexab\n", b" x ", b"zabc\n", b"\nabd"]
    data = planted_each(scrubbed(shape), [words[i % 5] for i in range(len(starts))], [max(s - 1, 0) for s in starts])
    enc = encode(torch, codec, data, bs)
    fixed = [lit(w) for w in (b"abc", b"dexab", b"x")]
    ctx_kw = (dict(), dict(invert=True), dict(before=1, after=2), dict(numbers=False, flags=False))
    # no optional position, one term: the anchored calls
    for anchors in [0] + EACH_ANCHOR:
        older = positions(torch, codec, enc, fixed, anchors, 40)
        check(older, find_any_expr_model(data, fixed, NL, W, anchors, bs, 40), 40, (shape, anchors))
        for optional in (None, bytes(9)):
            assert same_arrays(pos_call(torch, codec, enc, fixed, anchors, 40, optional=optional), older), (shape, anchors, optional)
        for kw in ctx_kw:
            older = records(torch, codec, enc, fixed, anchors, 9, max_len=7, **kw)
            for mode in (ALL, ORDERED):
                assert same_arrays(rec_call(torch, codec, enc, [fixed], anchors, mode, 9, max_len=7, optional=None, **kw), older), (shape, anchors, kw)
    # no anchor, one term: the quant calls
    quant = [lit(b"abc", (2,)), lit(b"dexab", (1, 2)), rep(b"x", 1, 3)]
    older = positions_of(quant_call(torch, codec, enc, "find_any_quant", quant, 40))
    check(older, find_any_expr_model(data, quant, NL, W, 0, bs, 40), 40, (shape, "quant"))
    assert same_arrays(pos_call(torch, codec, enc, quant, 0, 40, delims=None), older), shape
    for kw in ctx_kw:
        older = quant_call(torch, codec, enc, "find_records_quant", quant, 9, max_len=7, **kw)
        assert same_arrays(rec_call(torch, codec, enc, [quant], 0, ORDERED, 9, max_len=7, **kw), older), (shape, kw)
    # no anchor, no optional position: the terms call
    terms = [[b"ab"], [b"c", b"d"]]
    for mode in (ALL, ORDERED):
        for kw in ctx_kw:
            older = terms_call(torch, codec, enc, terms, mode, 9, max_len=7, **kw)
            mine = rec_call(torch, codec, enc, [[lit(a) for a in t] for t in terms], 0, mode, 9, max_len=7, **kw)
            assert int(older[2][0]) > 0 and same_arrays(mine, older), (shape, mode, kw)


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_word_with_optional_letters_is_the_anchored_call_over_the_written_out_forms(torch_mod, codec, shape):
    """grep -w 'colou?r|https?|gra?ys?': one call, and the forms written out through hufgpu_find_any_anchored"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    alts = [lit(b"colour", (4,)), lit(b"https", (4,)), lit(b"grays", (2, 4))]
    words = [b" color ", b" colour.", b"_colour ", b" http\n", b"\nhttps ", b" httpss", b" gry ", b" grays ", b"zgray ", b" grys\n"]
    found = 0
    for rot in range(3):
        at = [max(s - 1 - (i + rot) % 5, 0) for i, s in enumerate(starts)]
        data = planted_each(base_of(shape), [words[(i + rot) % len(words)] for i in range(len(starts))], at)
        enc = encode(torch, codec, data, bs)
        for anchors in (WORD, WORD | BOL, EOL):
            total, res = exact(torch, codec, enc, alts, anchors, at_least=0, what=(shape, rot, anchors))
            written = forms(alts)
            assert len(written) == 2 + 2 + 4 and sum(len(f) + 1 for f in written) <= 64
            assert same_arrays(res, positions(torch, codec, enc, written, anchors, total + 7)), (shape, rot, anchors)
            found += total
    assert found >= 1


# ---- anchors with optional positions, at every seam ------------------------------------------------------------------------
SEAM_PATTERNS = {"ab?": ([lit(b"ab", (1,))], [b"ab", b"a", b"abb", b"b"]),
                 "a?b": ([lit(b"ab", (0,))], [b"ab", b"b", b"aab", b"a"]),
                 "x{2,5}": ([rep(b"x", 2, 5)], [b"x" * r for r in (1, 2, 3, 5, 6, 7)])}
AROUND = [(b"\n", b"\n"), (b" ", b" "), (b"z", b"z"), (b"\n", b"z"), (b"z", b"\n"), (b" ", b"\n"), (b"\n", b" ")]


@pytest.mark.parametrize("anchors", EACH_ANCHOR, ids=lambda a: NAMES[a])
@pytest.mark.parametrize("name", list(SEAM_PATTERNS))
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_every_seam(torch_mod, codec, shape, name, anchors):
    """forms and strings that are none between every pair of neighbours, the match at every lane, tile, chunk and block seam
    and at a record start on bit 0 of a word, a tile, a block and a scan group, at every split: the plants rotate through the
    starts and move back byte by byte, so the boundary byte, the byte in front and every byte of a form lie on either side"""
    bs, n, _ = FOUR_SHAPES[shape]
    alts, cores = SEAM_PATTERNS[name]
    starts = all_starts(shape)
    for rot in range(4):
        strings, at = [], []
        for i, s in enumerate(starts):
            core, (left, right) = cores[(i + rot) % len(cores)], AROUND[(i + 2 * rot) % len(AROUND)]
            if i == 1:
                core, left, right = b"".join(forms(alts)[rot % 2]), b"\n", b"\n"      # a form that is a whole line, whatever else there is
            strings.append(left + core + right)
            at.append(max(s - 1 - (i + rot) % (len(core) + 2), 0))
        data = planted_each(scrubbed(shape), strings, at)
        enc = encode(torch_mod, codec, data, bs)
        exact(torch_mod, codec, enc, alts, anchors, what=(shape, name, anchors, rot))


def test_the_shortest_form_fails_its_anchor_and_a_longer_one_qualifies_and_the_reverse(torch_mod, codec):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["5x4099"]
    ab_ = [lit(b"ab", (1,))]
    at = {"ab\\n": bs - 2, "a\\n": 2 * bs - 1, "abz": TILE - 1, "a b": bs + TILE - 1, "abb\\n": 3 * bs - 1, "\\nabz": 2 * bs + TILE - 2}
    data = scrubbed("5x4099")
    data[data == 10] = 11
    data = planted_each(data, [b" ab\n", b" a\n", b" abz", b" a b", b" abb\n", b"\nabz"], [a - 1 for a in list(at.values())[:5]] + [at["\\nabz"]])
    enc = encode(torch, codec, data, bs)
    # 'ab?$': "a" lies at the start of "ab\n" and its R is 'b'; "ab" qualifies.  "abz", "a b", "abb\n": no form qualifies there
    total, _ = exact(torch, codec, enc, ab_, EOL, must=[at["ab\\n"], at["a\\n"]], must_not=[at["abz"], at["a b"], at["abb\\n"]], what="eol")
    assert total == 2
    # -w 'ab?': at "a b" the short form qualifies and the long one does not lie there; at "abz" the short one's R is a word byte
    exact(torch, codec, enc, ab_, WORD, must=[at["a b"], at["a\\n"], at["ab\\n"]], must_not=[at["abz"], at["abb\\n"], at["\\nabz"] + 1], what="word")
    exact(torch, codec, enc, ab_, BOL, must=[at["\\nabz"] + 1], must_not=[at["ab\\n"]], what="bol")


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_the_ends_of_the_data(torch_mod, codec, shape):
    """a form that ends exactly at raw_size, with and without a delimiter behind it, and a start at byte 0: an absent
    neighbour never stands in the way, and no form that would need a byte behind the data is reported"""
    bs, n, _ = FOUR_SHAPES[shape]
    for name, (alts, _) in SEAM_PATTERNS.items():
        short = b"".join(min(forms(alts), key=len))
        longest = b"".join(max(forms(alts), key=len))
        tails = (longest, short, longest + b"\n", short + b"\n", b" " + short, b"z" + longest, longest[:-1] + b"z")
        if shape == "3chunks":                                      # (the model's time: one pattern less, four tails)
            if name == "a?b":
                continue
            tails = tails[0:1] + tails[3:5] + tails[6:]
        for tail in tails:
            data = scrubbed(shape)
            data[-8:] = ord("\n")
            data[:8] = np.frombuffer((longest + b"\n\n\n\n\n\n\n\n")[:8], np.uint8)
            data[n - len(tail):] = np.frombuffer(tail, np.uint8)
            enc = encode(torch_mod, codec, data, bs)
            for anchors in EACH_ANCHOR:
                exact(torch_mod, codec, enc, alts, anchors, must=[0], what=(shape, name, tail, anchors))
    data = scrubbed(shape)
    data[n - 3:] = np.frombuffer(b"\nab", np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    exact(torch_mod, codec, enc, [lit(b"abc", (1,))], BOL | EOL, at_least=0, must_not=[n - 2], what=(shape, "'ab?c' cut: its last byte is not there"))
    exact(torch_mod, codec, enc, [lit(b"abc", (2,))], BOL | EOL, must=[n - 2], what=(shape, "'abc?' ends with the data"))


# ---- the layout of the state -------------------------------------------------------------------------------------------------
def narrow(rng, m, flags):
    """classes of three of the four letters at every fourth position and at the optional ones, all four elsewhere"""
    letters = np.frombuffer(b"abcd", np.uint8)
    return [O(c) if f else c for c, f in zip([bytes(rng.choice(letters, 3 if k % 4 == 0 or flags[k] else 4, replace=False)) for k in range(m)], flags)]


@pytest.mark.parametrize("shape", ["5x4099", "300x64"])
def test_the_layout_of_the_state_with_boundary_positions(torch_mod, codec, shape):
    bs, n, _ = FOUR_SHAPES[shape]
    data = np.random.default_rng(91).choice(np.frombuffer(b"abcd \n", np.uint8), n, p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02]).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    rng = np.random.default_rng(92)
    run = lambda m, lo, hi: [lo <= k < hi for k in range(m)]             # noqa: E731
    cases = {
        "63 positions and the boundary at bit 0, a run right above it": [narrow(rng, 63, run(63, 58, 63))],
        "63 positions, a run across bits 31 / 32": [narrow(rng, 63, run(63, 29, 35))],
        "the boundary of alternative 0 at bit 32, alternative 1 from bit 31 down to a boundary at bit 0": [narrow(rng, 31, run(31, 27, 31)), narrow(rng, 31, run(31, 0, 3))],
        "the boundary of alternative 0 at bit 31": [narrow(rng, 32, run(32, 30, 32)), narrow(rng, 6, run(6, 2, 4))],
        "a trailing run above a boundary right above the next alternative's leading run": [narrow(rng, 6, run(6, 3, 6)), narrow(rng, 5, run(5, 0, 3))],
        "32 alternatives of one position": [[bytes([v])] for v in b"ab"] * 16,
        "21 of two, each with a flag": [[O(b"c"), b"a"], [b"b", O(b"d")], [b"d", O(b"a")]] * 7,
    }
    for what, alts in cases.items():
        for anchors in (EOL, WORD, BOL | EOL):
            assert sum(len(a) + 1 for a in alts) <= 64
            exact(torch_mod, codec, enc, alts, anchors, at_least=0, what=(shape, what, anchors))
    total, _ = exact(torch_mod, codec, enc, cases["21 of two, each with a flag"], WORD, what="dense")
    assert total > 20


@pytest.mark.parametrize("shape", ["5x4099", "300x64", "200x3"])
def test_dense_random_data(torch_mod, codec, shape):
    """random patterns of every kind on lines of four letters: one term with every anchor, ALL of 2 to 4 quantified terms,
    ORDERED with a quantified last term and outer anchors"""
    bs, n, _ = FOUR_SHAPES[shape]
    enc = encode(torch_mod, codec, dense(n, 77), bs)
    rng = np.random.default_rng(78)
    letters = np.frombuffer(b"abcd ", np.uint8)

    def alternative(m, quantified):
        flags = [quantified and bool(rng.integers(0, 3) == 0) for _ in range(m)]
        flags[int(rng.integers(0, m))] = False
        classes = [bytes(rng.choice(letters, int(rng.integers(1, 3)), replace=False, p=[0.23, 0.23, 0.22, 0.22, 0.1])) for _ in range(m)]
        return [O(c) if f else c for c, f in zip(classes, flags)]

    found = 0
    for trial in range(6):
        alts = [alternative(int(rng.integers(1, 6)), True) for _ in range(int(rng.integers(1, 5)))]
        found += exact(torch_mod, codec, enc, alts, int(rng.integers(1, 8)), at_least=0, what=(shape, trial, alts))[0]
    assert found > 20, found
    for nt in (2, 3, 4):
        terms = [[alternative(int(rng.integers(2, 5)), True) for _ in range(int(rng.integers(1, 3)))] for _ in range(nt)]
        exact_records(torch_mod, codec, enc, terms, 0, ALL, at_least=1, what=(shape, "all", terms))
        for anchors in (0, int(rng.integers(1, 8)), int(rng.integers(1, 8))):
            terms = [[alternative(2, False) for _ in range(int(rng.integers(1, 3)))] for _ in range(nt - 1)]
            terms.append([alternative(int(rng.integers(1, 5)), True) for _ in range(int(rng.integers(1, 3)))])
            exact_records(torch_mod, codec, enc, terms, anchors, ORDERED, what=(shape, "ordered", anchors, terms))


# ---- quantified terms ------------------------------------------------------------------------------------------------------
TOOK = lit(b"took ") + rep(b"0123456789", 1, 5) + lit(b"ms")


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_quantified_terms(torch_mod, codec, shape):
    """ALL of 2, 3 and 4 quantified terms, and ORDERED with a quantified last term, the terms around every seam"""
    bs, n, _ = FOUR_SHAPES[shape]
    starts = all_starts(shape)
    lines = [b"\nab xd c\n", b"\nc ab\n", b"\nabb xxd\n", b"\nxd ac\n", b"\nac\n", b"\nxxd\nab\n", b"\nc c xd a\n"]
    terms = [[lit(b"ab", (1,))], [rep(b"x", 1, 2) + lit(b"d")], [lit(b"cc", (1,)), lit(b"b")], [lit(b"a"), lit(b" ", ())]]
    for rot in range(3):
        at = [max(s - 1 - (i + rot) % 7, 0) for i, s in enumerate(starts)]
        data = planted_each(scrubbed(shape), [lines[(i + rot) % len(lines)] for i in range(len(starts))], at)
        enc = encode(torch_mod, codec, data, bs)
        for nt in (2, 3, 4):
            exact_records(torch_mod, codec, enc, terms[:nt], 0, ALL, at_least=1, what=(shape, rot, "all", nt))
        ordered = [[lit(b"a")], [lit(b"xd"), lit(b" c")], [lit(b"cc", (0,)), rep(b"b", 1, 2)]]
        for nt in (2, 3):
            for anchors in (0, BOL, EOL, WORD, BOL | EOL | WORD):
                exact_records(torch_mod, codec, enc, ordered[:1] + ordered[3 - nt + 1:], anchors, ORDERED, what=(shape, rot, "ordered", nt, anchors),
                              **(dict(before=1, after=1) if anchors == WORD else {}))


def test_an_ordered_quantified_last_term_across_a_tile_seam_and_a_block_seam(torch_mod, codec):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["5x4099"]
    data = scrubbed("5x4099", b"ERORtokms0123456789")
    data[data == 10] = 11
    line = b"\nERROR x took 123ms\n"
    # the quantified term across a tile's end, across a block's end, its boundary byte in the next block, and the first term there
    at = [TILE - 15, bs - 16, 2 * bs - len(line) + 1, 3 * bs - 4, 3 * bs + TILE - len(line)]
    data = planted(data, line, at)
    data = planted(data, b"\ntook 5ms ERROR\n", [500])                                 # the wrong order
    data = planted(data, b"\nERROR took 123456ms\n", [4 * bs + 100])                    # six digits
    enc = encode(torch, codec, data, bs)
    terms = [[lit(b"ERROR")], [TOOK]]
    full, _ = exact_records(torch, codec, enc, terms, 0, ORDERED, must=[a + 1 for a in at], must_not=[501, 4 * bs + 101], what="took")
    assert int(full[3][0]) == len(at)
    for anchors in (BOL, EOL, BOL | EOL, WORD):
        exact_records(torch, codec, enc, terms, anchors, ORDERED, must=[a + 1 for a in at], must_not=[501], what=("took", anchors))
    exact_records(torch, codec, enc, terms, 0, ALL, must=[a + 1 for a in at] + [501], must_not=[4 * bs + 101], what="both, any order")


def test_bol_at_a_blocks_first_byte_and_eol_in_the_next_block(torch_mod, codec):
    """'^A.*B$': A at a block's first byte - its L is the last byte of the block in front -, and B's delimiter in the next block"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["5x4099"]
    data = scrubbed("5x4099")
    data[data == 10] = 11
    fill = bytes([ord("z")]) * (bs - 5)
    data = planted(data, b"\nab" + fill + b"xxd\n", [bs - 1])        # A at byte bs, B ends with block 1, its '\n' is block 2's first byte
    data = planted(data, b"\nab zz xd\nzab xxd\nab xdz\n", [3 * bs - 5])
    enc = encode(torch, codec, data, bs)
    terms = [[lit(b"ab")], [rep(b"x", 1, 2) + lit(b"d")]]
    full, _ = exact_records(torch, codec, enc, terms, BOL | EOL, ORDERED, must=[bs, 3 * bs - 4], must_not=[3 * bs + 5, 3 * bs + 13], what="^ab.*x{1,2}d$")
    assert int(full[3][0]) == 2
    for b, gone in ((0, [bs]), (2, [bs, 3 * bs - 4]), (3, [3 * bs - 4])):               # L's block, R's block, the second record's
        bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        errs = rec_or_not_served(torch, codec, bad, terms, BOL | EOL, ORDERED, 9, what=("block", b))
        assert errs.tolist() == [RW if j == b else OK for j in range(5)]
        res = seven(rec_call(torch, codec, bad, terms, BOL | EOL, ORDERED, 9))
        got = res[0][LEAD:LEAD + int(res[2][1])].tolist()
        assert not set(got) & set(gone), (b, got)


# ---- blocks that are not served ------------------------------------------------------------------------------------------------
def test_a_block_that_is_not_served_in_front_under_the_boundary_or_under_the_long_form(torch_mod, codec):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["5x4099"]
    data = scrubbed("5x4099")
    data[data == 10] = 11
    alts = [[b"a", O(b"b "), O(b"c")]]                              # 'a[b ]?c?': its second position takes a byte that is no word byte
    first, only_long, inside, under_r = 2 * bs, 3 * bs - 2, 3 * bs + 100, 4 * bs - 2
    data = planted(data, b" abc ", [first - 1, inside - 1])          # L of `first` is block 1's last byte
    data = planted(data, b" a c ", [only_long - 1])                  # "a" and its R lie in block 2, "a c" and its R reach block 3
    data = planted(data, b" ab ", [under_r - 1])                     # "a" has a word byte behind it; R of "ab" is block 4's first byte
    enc = encode(torch, codec, data, bs)
    total, _ = exact(torch, codec, enc, alts, WORD, must=[first, only_long, inside, under_r], what="all served")
    assert total == 4
    want = {1: [only_long, inside, under_r], 2: [inside, under_r], 3: [first, only_long], 4: [first, only_long, inside]}
    for b, left in want.items():
        bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        res = pos_call(torch, codec, bad, alts, WORD, 9)
        assert res[2].tolist() == [RW if j == b else OK for j in range(5)]
        check(res, find_any_expr_model(data, alts, NL, W, WORD, bs, 9, served=res[2] == OK), 9, ("block", b))
        assert res[0][LEAD:LEAD + int(res[1][1])].tolist() == left, (b, res[0])
    # the LONG form alone qualifies, and reaches the block: 'ab?$' on "ab\n" - "a" has 'b' behind it, the '\n' of "ab" is block 3's first byte
    ab_ = [lit(b"ab", (1,))]
    data2 = planted(data, b" ab\n", [3 * bs - 3])
    enc2 = encode(torch, codec, data2, bs)
    exact(torch, codec, enc2, ab_, EOL, must=[3 * bs - 2], what="ab\\n served")
    res = pos_call(torch, codec, damaged(enc2, int(enc2.h_offs[3]), 0x01), ab_, EOL, 9)
    check(res, find_any_expr_model(data2, ab_, NL, W, EOL, bs, 9, served=res[2] == OK), 9, "ab\\n, block 3")
    assert 3 * bs - 2 not in res[0][LEAD:].tolist()
    res = pos_call(torch, codec, damaged(enc2, int(enc2.h_offs[3]), 0x01), ab_, 0, 9)         # no anchor: "a" lies in block 2
    assert 3 * bs - 2 in res[0][LEAD:].tolist()


def damage_input(torch, codec):
    """two byte values - a 1 at an even payload bit leaves the tree -: 7 is the delimiter and no word byte, 207 the letter"""
    bs, n = 4099, 5 * 4099
    data = (np.random.default_rng(56).integers(0, 6, n) != 0).astype(np.uint8) * 200 + 7
    data[[0, bs - 1, bs, 2 * bs - 2, 3 * bs + 1, n - 1]] = 7
    run = [bytes([207])] * 3 + [O(bytes([207]))] * 3                  # 'x{3,6}'
    return encode(torch, codec, data, bs), [run], [[[bytes([207])] * 2], [rep(bytes([207]), 2, 4)]]


@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_damage_in_every_block(torch_mod, codec, damage):
    torch = torch_mod
    enc, alts, terms = damage_input(torch, codec)
    n = enc.n
    words = bytes([207])
    sets = dict(delims=bytes([7]), words=words)
    model = lambda anchors: lambda cap, served: find_any_expr_model(enc.data, alts, bytes([7]), words, anchors, enc.bs, cap, served)   # noqa: E731
    rmodel = lambda t, anchors, mode: lambda cap, served: find_records_expr_model(enc.data, t, bytes([7]), words, anchors, mode, enc.bs, cap, 0, served)   # noqa: E731
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for anchors in EACH_ANCHOR:
            errs = answer_or_not_served(lambda cap: pos_call(torch, codec, bad, alts, anchors, cap, **sets), model(anchors), n, (damage, b, anchors))
            assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
        for t, anchors, mode in (([alts], BOL | EOL, ORDERED), (terms, 0, ALL), (terms, EOL, ORDERED), (terms, WORD, ORDERED)):
            errs = answer_or_not_served(lambda cap: rec_call(torch, codec, bad, t, anchors, mode, cap, **sets), rmodel(t, anchors, mode), 40,
                                        (damage, b, anchors, mode))
            assert errs.tolist() == [RW if j == b else OK for j in range(5)]


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    n = 5 * bs + 1500
    data = dense(n, 31)
    enc = encode(torch, codec, data, bs)
    alts = [lit(b"abc", (1,)), rep(b"d", 2, 3)]
    terms = [[lit(b"ab")], [lit(b"cd", (1,)), rep(b"b", 2, 3)]]
    rng = np.random.default_rng(33)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    assert not pos_or_not_served(torch, codec, enc, alts, WORD, n, what="own").any()
    errs = pos_or_not_served(torch, codec, enc, alts, WORD, n, sub=other, what=sub)
    assert sub == "random" or errs.all()                    # (a bit count of 0 cannot be that of 32 codewords)
    for t, anchors, mode in ((terms, BOL | EOL, ORDERED), (terms, 0, ALL), ([alts], EOL, ORDERED)):
        assert not rec_or_not_served(torch, codec, enc, t, anchors, mode, n, what="own").any()
        rec_or_not_served(torch, codec, enc, t, anchors, mode, n, sub=other, what=sub)
    bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    pos_or_not_served(torch, codec, bad, alts, BOL | EOL, n, sub=other, what=(sub, "and a damaged block"))
    rec_or_not_served(torch, codec, bad, terms, WORD, ORDERED, n, sub=other, what=(sub, "and a damaged block"), before=1, after=1)


# ---- one-symbol blocks -----------------------------------------------------------------------------------------------------
def test_one_symbol_blocks_whose_value_is_in_or_out_of_the_boundary_class(torch_mod, codec):
    """every byte is ')': with -w it may stand behind a form (no word byte), with '$' it may not (no delimiter) - but for the
    form that ends where the data ends; as a delimiter it may, but then no class holds it"""
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    leaf, other = b")(", b"(*"
    for m, optional in ((1, ()), (5, (1, 3)), (33, (0, 1, 30, 31, 32)), (62, tuple(range(1, 62)))):
        alt = [O(leaf) if k in optional else leaf for k in range(m)]
        shortest = m - len(optional)
        want = find_any_expr_model(enc.data, [alt], NL, W, WORD, bs, n + 3)
        assert np.array_equal(want[0], np.arange(n - shortest + 1))             # the value is no word byte: every start
        res = pos_call(torch, codec, enc, [alt], WORD, n + 3)
        assert not res[2].any()
        check(res, want, n + 3, (m, optional, "word"))
        want = find_any_expr_model(enc.data, [alt], NL, b")", WORD, bs, 9, None)
        assert want[0].tolist() == []                                           # ... a word byte: a neighbour always stands in the way
        check(pos_call(torch, codec, enc, [alt], WORD, 9, words=b")"), want, 9, (m, optional, "a word byte"))
        for anchors in (EOL, BOL | EOL, BOL):                                   # no delimiter: only the forms that end with the data
            want = find_any_expr_model(enc.data, [alt], NL, W, anchors, bs, 99)
            assert want[0].tolist() == {EOL: list(range(n - m, n - shortest + 1)), BOL | EOL: [], BOL: [0]}[anchors]
            check(pos_call(torch, codec, enc, [alt], anchors, 99), want, 99, (m, optional, anchors))
        res = pos_call(torch, codec, enc, [[other] + alt], WORD, 4)              # the value in no class of a required position
        assert not res[2].any() and res[1].tolist() == [0, 0, 0, 0]
    terms = [[[leaf, leaf]], [[leaf] * 2 + [O(leaf)] * 2]]
    for anchors, mode in ((0, ALL), (WORD, ORDERED), (BOL | EOL, ORDERED), (EOL, ORDERED)):
        check(rec_call(torch, codec, enc, terms, anchors, mode, 3), find_records_expr_model(enc.data, terms, NL, W, anchors, mode, bs, 3), 3, (anchors, mode))


def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec):
    torch = torch_mod
    bs = 4099
    data = np.random.default_rng(26).choice(np.frombuffer(b"zyw.,\n", np.uint8), 6 * bs).astype(np.uint8)
    for b in range(0, 6, 2):
        data[b * bs:(b + 1) * bs] = 41
    data = planted_each(data, [b"))))ab ", b" ab))", b"))b\n", b"\nab))))", b")) ab"], [bs - 4, 2 * bs - 3, 3 * bs - 2, 4 * bs - 3, 6 * bs - 5])
    enc = encode(torch, codec, data, bs)
    assert [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)] == [True, False] * 3
    paren = b")("
    alts = [[paren, O(paren), paren] + lit(b"ab", (0,)), lit(b"ab", (0,)) + [paren, O(paren), O(paren)], [paren] * 3 + [O(paren)] * 2]
    for anchors in EACH_ANCHOR:
        exact(torch, codec, enc, alts, anchors, at_least=0, what=("alternate", anchors))
    total, _ = exact(torch, codec, enc, alts, WORD, what="alternate, word")
    assert total >= 3
    pos_or_not_served(torch, codec, enc, alts, WORD, 3 * bs, sub=torch.zeros_like(enc.sub), what="zeros")


# ---- the caps and the records ------------------------------------------------------------------------------------------------
LOG_WORDS = [b"color", b"colour", b"colouur", b"colors", b"took 5ms", b"took 12345ms", b"took 123456ms", b"ERROR", b"ERRORS", b"refused 7 times"]


def log_input(torch, codec, lines=400, seed=71):
    """a few hundred log lines of words, in blocks of 4 099 bytes"""
    rng = np.random.default_rng(seed)
    fill = [b"x", b"the", b"at", b"10.0.0.1", b"_", b"1234.5.6.7", b"ok"]
    made = [b"ERROR at took 5ms", b"ERROR took 12345ms", b"ERROR took 123456ms", b"xERROR took 5ms", b"ERROR took 5ms x",
            b"ERRORS refused 7 times", b"10.0.0.1 ok", b"the x at ok", b"x colour", b"took 77ms ERROR"]
    out = []
    for i in range(lines):
        words = [(LOG_WORDS, fill)[int(rng.integers(0, 3) != 0)] for _ in range(int(rng.integers(0, 7)))]
        out.append(made[i // 7 % len(made)] if i % 7 == 0 else b" ".join(w[int(rng.integers(0, len(w)))] for w in words))
    data = np.frombuffer(b"\n".join(out), np.uint8)
    return encode(torch, codec, data, 4099)


LOG_CASES = {"-w colou?r": ([[lit(b"colour", (4,))]], WORD, ORDERED), "^ERROR.*took [0-9]{1,5}ms$": ([[lit(b"ERROR")], [TOOK]], BOL | EOL, ORDERED),
             "colou?r and took": ([[lit(b"colour", (4,))], [TOOK, lit(b"ERRORS", (5,))]], 0, ALL)}


def test_caps(torch_mod, codec):
    torch = torch_mod
    enc = log_input(torch, codec)
    alts = [lit(b"colour", (4,)), TOOK]
    total = int(find_any_expr_model(enc.data, alts, NL, W, WORD, enc.bs)[2][0])
    assert total > 20
    for cap in (0, 1, total - 1, total):
        for counts in (True, False):
            res = pos_call(torch, codec, enc, alts, WORD, cap, counts=counts)                   # (cap 0: d_pos is NULL)
            assert not res[2].any() and int(res[1][0]) == total
            check(res, find_any_expr_model(enc.data, alts, NL, W, WORD, enc.bs, cap), cap, (cap, counts))
    for terms, anchors, mode in LOG_CASES.values():
        rtotal = int(find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs)[3][0])
        assert rtotal > 2
        for cap in (0, 1, rtotal - 1, rtotal):
            res = rec_call(torch, codec, enc, terms, anchors, mode, cap, counts=bool(cap % 2), numbers=bool(cap % 2), flags=False)
            assert not res[3].any() and int(res[2][0]) == rtotal
            want = find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, cap)
            check(res, want[:5] if cap % 2 else want[:4], cap, (cap, anchors, mode))


@pytest.mark.parametrize("kw", [dict(), dict(invert=True), dict(before=2, after=2), dict(invert=True, before=1, after=2), dict(before=0, after=2),
                                dict(max_len=6)], ids=str)
@pytest.mark.parametrize("case", list(LOG_CASES))
def test_records_invert_numbers_and_context(torch_mod, codec, case, kw):
    torch = torch_mod
    enc = log_input(torch, codec)
    terms, anchors, mode = LOG_CASES[case]
    kw = dict(kw)
    max_len = kw.pop("max_len", 0)
    total = int(find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, enc.n, max_len, **kw)[3][0])
    assert total > 2
    for cap in (total + 3, total - 1):
        res = rec_call(torch, codec, enc, terms, anchors, mode, cap, max_len=max_len, **kw)
        assert not res[3].any()
        check(res, find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, cap, max_len, **kw), cap, (case, kw, cap))


# ---- the Python layer --------------------------------------------------------------------------------------------------------
EGREPS = [rb"^[0-9]{1,3}\.[0-9]{1,3}", rb"\<colou?r\>", rb"\bcolou?rs?\b|\bERRORS?\b", rb"refused [0-9]{1,5} times$", rb"^ERROR.*took [0-9]{1,5}ms",
          rb"ERROR.*took [0-9]{1,5}ms$", rb"^the.*at.*ok$", rb"\<took.*[0-9]{5}ms\>", rb"^.*colou?r$", rb"^x.*"]


@pytest.mark.parametrize("expr", EGREPS, ids=lambda e: e.decode())
def test_grep_of_egrep_against_an_re_filter(torch_mod, codec, expr):
    """grep(egrep(...)) - enqueue-only, read back below - gives the lines that `re` keeps, with their numbers"""
    torch = torch_mod
    enc = log_input(torch, codec)
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
    pattern = GpuCodec.egrep(expr)
    assert isinstance(pattern, Expr)
    expr = expr.replace(rb"\<", rb"\b").replace(rb"\>", rb"\b")     # (`re` has '\b' alone)
    rx = re.compile(expr)
    lines = bytes(enc.data).split(b"\n")
    keep = [i for i, ln in enumerate(lines) if rx.search(ln) and ln]
    assert 0 < len(keep) < len(lines)
    rows, width = len(keep) + 2, 80
    out = codec.grep(*args, pattern, rows, width, line_numbers=True)
    got, raw_lens, gerrs, totals, berrs, numbers = [t.cpu().numpy() for t in out]
    assert totals.tolist()[:3] == [len(keep), len(keep), 0] and not berrs.any() and not gerrs.any()
    assert [bytes(got[i, :raw_lens[i]]) for i in range(len(keep))] == [lines[i][:width] for i in keep]
    assert numbers[:len(keep)].tolist() == keep
    totals, errs = codec.count_records(*args, pattern, invert=True)
    assert totals.cpu().tolist()[0] == sum(1 for ln in lines if ln) - len(keep)
    if len(pattern) == 1 and b".*" not in expr:                     # (a '.*' that egrep drops moves the start, not the line)
        want = [m.start() for m in re.finditer(b"(?=(?:" + expr + b"))", bytes(enc.data), re.MULTILINE)]
        pos, totals, errs, _ = codec.find_pattern(*args, pattern, max_positions=len(want) + 2)
        assert totals.cpu().tolist()[:3] == [len(want), len(want), 0] and pos.cpu().numpy()[:len(want)].tolist() == want
        assert codec.count_pattern(*args, pattern)[0].cpu().tolist()[0] == len(want)


def test_expr_by_hand_and_its_refusals(torch_mod, codec):
    torch = torch_mod
    enc = log_input(torch, codec)
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)
    by_hand = Expr(b"ERROR", list(b"took ") + [Rep(b"0123456789", 1, 5), ord("m"), ord("s")], bol=True, eol=True)
    terms, anchors, mode = LOG_CASES["^ERROR.*took [0-9]{1,5}ms$"]
    res = find_call(torch, codec, enc, "find_records", by_hand, 40, numbers=True)
    check(res[:6], find_records_expr_model(enc.data, terms, NL, W, anchors, mode, enc.bs, 40)[:5], 40, "by hand")
    both = Expr([ord("c"), ord("o"), ord("l"), ord("o"), Opt(b"u"), ord("r")], GpuCodec.AnyOf(b"ERROR", [Rep(b"s", 1, 2)]), ordered=False)
    want = find_records_expr_model(enc.data, [[lit(b"colour", (4,))], [lit(b"ERROR"), rep(b"s", 1, 2)]], NL, W, 0, ALL, enc.bs, 40, before=1)
    res = codec.find_records(*args, both, max_records=40, before=1, ignore_case=False)
    assert res[2].cpu().tolist() == want[3].tolist() and res[0].cpu().numpy()[:want[0].size].tolist() == want[0].tolist()
    upper = codec.count_records(*args, Expr(b"error", [ord("T"), Opt(b"o"), ord("O")], eol=False), ignore_case=True)[0].cpu().tolist()[0]
    assert upper == sum(1 for ln in bytes(enc.data).split(b"\n") if re.search(rb"error.*to?o", ln, re.IGNORECASE))
    for bad in (dict(bol=True), dict(word=True), dict(whole_line=True), dict(eol=True), dict(word_bytes=b"a")):
        with pytest.raises(ValueError, match="the Expr carries its anchors"):
            codec.find_records(*args, by_hand, **bad)
        with pytest.raises(ValueError, match="the Expr carries its anchors"):
            codec.find_pattern(*args, Expr(b"a"), **bad)
    with pytest.raises(TypeError, match="selects records"):
        codec.find_pattern(*args, by_hand)
    with pytest.raises(TypeError):
        codec.count_pattern(*args, both)


# ---- one context -----------------------------------------------------------------------------------------------------------
def test_calls_back_to_back_on_one_context(torch_mod, codec):
    """expr calls of every route between a literal call, an anchored call, a quant call, a terms call and find_bytes: each gives
    its own model's answer, and the older ones give the same after as before"""
    torch = torch_mod
    enc = log_input(torch, codec)
    data, bs = enc.data, enc.bs
    colour, anyof = [lit(b"colour", (4,))], [lit(b"took"), lit(b"color")]

    def older():
        return [psearch(torch, codec, enc, b"took ", 40), positions(torch, codec, enc, anyof, WORD, 40),
                positions_of(quant_call(torch, codec, enc, "find_any_quant", colour, 40)),
                terms_call(torch, codec, enc, [[b"ERROR"], [b"took"]], ORDERED, 40, before=1),
                context(torch, codec, enc, anyof, NL, 40, before=1, after=1), find(torch, codec, enc, NL, 40)]

    def mine():
        check(pos_call(torch, codec, enc, colour, WORD, 40), find_any_expr_model(data, colour, NL, W, WORD, bs, 40), 40, "positions")
        for terms, anchors, mode in LOG_CASES.values():
            res = rec_call(torch, codec, enc, terms, anchors, mode, 40, before=1)
            check(res, find_records_expr_model(data, terms, NL, W, anchors, mode, bs, 40, before=1), 40, ("records", anchors, mode))

    mine()
    before = older()
    check(before[0], find_any_model(data, [lit(b"took ")], bs, 40), 40, "older")
    check(before[4], find_context_model(data, anyof, NL, bs, 40, before=1, after=1), 40, "older")
    mine()
    for a, b in zip(before, older()):
        assert same_arrays(a, b)
    mine()

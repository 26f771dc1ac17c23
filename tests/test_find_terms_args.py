"""hufgpu_find_records_terms: its declaration, the checks of the arguments of its own and their order, the older call's checks
under the new prefix, the Python model of its result (tests/find_terms_model.py) against Python's `re`, and GpuCodec.AllOf /
GpuCodec.Seq (no GPU needed: argument errors are found before the context is looked at).
"""
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
from find_args_support import HUFE_ARGUMENT, LAYOUTS, ROOT, alts_of, bracket, lib, valid  # noqa: F401 (lib: a fixture)
from find_args_support import call as older_call
from find_context_model import find_context_model
from find_terms_model import ALL, ORDERED, find_terms_model, satisfying
from find_terms_support import ONE, SLOTS, TWO, WHO, call
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

AnyOf, AllOf, Seq = GpuCodec.AnyOf, GpuCodec.AllOf, GpuCodec.Seq
MODES = pytest.mark.parametrize("mode", [ALL, ORDERED], ids=["all", "ordered"])


# ---- the symbol ------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared(lib):
    """the context call's 26 arguments with (term_alts, n_terms, terms_mode) behind n_alts: 29, as the header declares them"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    name, sibling = "hufgpu_find_records_terms", "hufgpu_find_records_context"
    assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
    mine, theirs = list(getattr(lib, name).argtypes), list(getattr(lib, sibling).argtypes)
    assert len(theirs) == 26 and len(mine) == 29 == len(SLOTS) and mine[:12] == theirs[:12] and mine[15:] == theirs[12:]
    vp, u32 = theirs[1], theirs[11]
    assert mine[12:15] == [vp, u32, u32]
    assert getattr(lib, name).restype is getattr(lib, sibling).restype
    m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 28
    want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t n_alts,", "uint32_t n_alts, const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode,")
    assert want == re.sub(r"\s+", " ", m.group(1))
    assert header.index(name + "(hufgpu_ctx_t") > header.index("hufgpu_find_records_anchored(hufgpu_ctx_t")
    assert (_native.FIND_TERMS_MAX, _native.TERMS_ALL, _native.TERMS_ORDERED) == (4, ALL, ORDERED) == (4, 0, 1)
    for text in (r"HUFGPU_FIND_TERMS_MAX\s+4\b", r"HUFGPU_TERMS_ALL\s+0u\b", r"HUFGPU_TERMS_ORDERED\s+1u\b"):
        assert re.search(r"#define\s+" + text, header)
    doc = header[header.index("FIND, ALL OF SEVERAL TERMS"):header.index(name + "(hufgpu_ctx_t")]
    for words in ("OUT OF SCOPE", "anchors together with terms", "unequal lengths", "positions call", "which occurrences", "ends first"):
        assert words in doc, words


# ---- the new errors --------------------------------------------------------------------------------------------------------
def refused(rc, msg, *words):
    assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "needs a context" not in msg, msg
    for w in words:
        assert w in msg, (w, msg)
    return True


@MODES
def test_valid_terms_reach_the_last_check(lib, mode):
    for nblocks, raw_size in LAYOUTS:
        kw = dict(nblocks=nblocks, raw_size=raw_size, mode=mode)
        assert valid(*call(lib, **kw), WHO)
        assert valid(*call(lib, alts=ONE, **kw), WHO)                                  # one term
        assert valid(*call(lib, ta=(3,), mode=ALL, nblocks=nblocks, raw_size=raw_size), WHO)      # ... of three alternatives
        assert valid(*call(lib, ta=(1, 1, 1), **kw), WHO)
        assert valid(*call(lib, alts=alts_of(*[[b"xy"]] * 4), ta=(1, 1, 1, 1), **kw), WHO)
        assert valid(*call(lib, alts=alts_of(*[[b"x"] * 16] * 4), ta=(1, 1, 1, 1), **kw), WHO)    # 64 positions in all
        assert valid(*call(lib, alts=alts_of(*[[b"x"]] * 64), ta=(61, 1, 1, 1), **kw), WHO)
        assert valid(*call(lib, alts=alts_of([b"a"] * 2, [b"b"] * 2, [b"c"] * 3, [b"d"] * 3), ta=(2, 2), **kw), WHO)
    for ba in ((0, 0), (0, 1), (2**32 - 1, 2**32 - 1)):
        for out in (dict(), dict(no=None), dict(sel=None), dict(no=None, sel=None, cap=0, pos=None, rlens=None, counts=None)):
            assert valid(*call(lib, ba=ba, **out), WHO)


def test_an_unknown_mode(lib):
    for mode in (2, 3, 0x80000000, 0xFFFFFFFF):
        for more in (dict(), dict(ta=None), dict(ta=(1, 2, 0)), dict(cls=None, totals=None), dict(delims=None)):
            assert refused(*call(lib, mode=mode, **more), "terms_mode %u" % mode, "HUFGPU_TERMS_ORDERED")


@MODES
def test_a_null_term_alts(lib, mode):
    for nblocks, raw_size in LAYOUTS:
        for more in (dict(), dict(nt=2), dict(nt=0), dict(nt=9), dict(cls=None), dict(totals=None)):
            assert refused(*call(lib, ta=None, mode=mode, nblocks=nblocks, raw_size=raw_size, **more), "term_alts is required")


@MODES
def test_the_number_of_terms(lib, mode):
    for ta in ((), (1,) * 5, (1,) * 64):
        alts = alts_of(*[[b"x"]] * max(len(ta), 1))
        for more in (dict(), dict(cls=None), dict(n=7)):
            assert refused(*call(lib, alts=alts, ta=ta, mode=mode, **more), "n_terms %d is not 1 to 4" % len(ta))
    assert refused(*call(lib, nt=0xFFFFFFFF, mode=mode), "n_terms 4294967295 is not 1 to 4")


@MODES
def test_a_term_without_alternatives(lib, mode):
    for ta, at in (((0, 3), 0), ((3, 0), 1), ((1, 2, 0), 2), ((1, 1, 1, 0), 3), ((0, 0), 0), ((0,), 0)):
        for nblocks, raw_size in LAYOUTS:
            assert refused(*call(lib, ta=ta, mode=mode, nblocks=nblocks, raw_size=raw_size), "term %d has no alternative" % at)
    assert refused(*call(lib, ta=(2, 0, 5), mode=mode), "term 1 has no alternative")    # in front of the sum


@MODES
def test_counts_that_do_not_sum_to_n_alts(lib, mode):
    for ta in ((1, 1), (2, 2), (1,), (1, 1, 1, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 4)):
        total = sum(ta)
        for more in (dict(), dict(cls=None), dict(lens=None)):
            assert refused(*call(lib, ta=ta, mode=mode, **more), "have %d alternatives" % total, "n_alts is 3")
    assert refused(*call(lib, ta=(1, 2), n=0, mode=mode), "have 3 alternatives", "n_alts is 0")     # in front of the older n_alts check
    assert refused(*call(lib, ta=(1, 2), n=65, mode=mode), "n_alts is 65")


def test_an_ordered_term_of_unequal_lengths(lib):
    mixed = alts_of([b"a"] * 2, [b"b"] * 3, [b"c"] * 3, [b"d"])
    for nblocks, raw_size in LAYOUTS:
        kw = dict(nblocks=nblocks, raw_size=raw_size)
        assert refused(*call(lib, alts=mixed, ta=(2, 2), mode=ORDERED, **kw), "term 0", "lengths 2 and 3", "one length a term")
        assert refused(*call(lib, alts=mixed, ta=(1, 3), mode=ORDERED, **kw), "term 1", "lengths 3 and 1")
        assert refused(*call(lib, alts=mixed, ta=(1, 1, 2), mode=ORDERED, **kw), "term 2", "lengths 3 and 1")
        assert valid(*call(lib, alts=mixed, ta=(1, 2, 1), mode=ORDERED, **kw), WHO)     # terms may differ
        assert valid(*call(lib, alts=mixed, ta=(2, 2), mode=ALL, **kw), WHO)            # ... and ALL does not mind
        assert valid(*call(lib, alts=mixed, ta=(4,), mode=ALL, **kw), WHO)
    assert refused(*call(lib, alts=mixed, ta=(4,), mode=ORDERED), "term 0", "lengths 2 and 3")      # one term as well
    # behind the counts' checks, in front of the older ones; the lengths are not read where the older checks would not read them
    assert refused(*call(lib, alts=mixed, ta=(2, 2), mode=ORDERED, totals=None, delims=None, pos=None), "term 0")
    assert refused(*call(lib, alts=mixed, ta=(2, 1), mode=ORDERED), "have 3 alternatives")
    assert "are required" in call(lib, alts=mixed, ta=(2, 2), mode=ORDERED, cls=None)[1]
    assert "are required" in call(lib, alts=mixed, ta=(2, 2), mode=ORDERED, lens=None)[1]
    sixty_five = alts_of(*[[b"x"]] * 65)
    assert "n_alts 65 is not 1 to 64" in call(lib, alts=sixty_five, ta=(62, 1, 1, 1), mode=ORDERED)[1]
    assert refused(*call(lib, alts=alts_of([b"a"], []), ta=(2,), mode=ORDERED), "lengths 1 and 0")
    assert "alternative 1 has length 0" in call(lib, alts=alts_of([b"a"], []), ta=(1, 1), mode=ORDERED)[1]


def test_the_order_of_the_new_checks(lib):
    """select, the mode, the array, the number of terms, an empty term, the sum, the lengths; then the older checks"""
    mixed = alts_of([b"a"] * 2, [b"b"] * 3)
    steps = [(dict(select=2), "select 0x2"), (dict(mode=5), "terms_mode 5"), (dict(terms=None), "term_alts is required"),
             (dict(nt=0), "n_terms 0"), (dict(terms=np.array([0, 2], np.uint32).tobytes(), nt=2), "term 0 has no alternative"),
             (dict(n=1), "n_alts is 1"), (dict(), "lengths 2 and 3")]
    for i, (first, words) in enumerate(steps):
        for second, _ in steps[i:]:
            if set(first) & set(second) and first is not second:
                continue                                    # (two mistakes in one argument)
            rc, msg = call(lib, **{**dict(alts=mixed, ta=(2,), mode=ORDERED, totals=None, delims=None), **second, **first})
            assert refused(rc, msg, words), (first, second, msg)


# ---- the older call's checks, in its order and wording ---------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("terms", ["one term", "two terms"])
def test_the_older_checks_follow_in_the_older_order(lib, mode, terms):
    """every pair of mistakes: the call and hufgpu_find_records_context complain about the same one, in the same words"""
    two = terms == "two terms"
    good = alts_of([b"a"], [b"b"])
    mistakes = [dict(cls=None), dict(lens=None), dict(pos=None), dict(rlens=None), dict(index=None), dict(stream=None), dict(errs=None),
                dict(sub=0x30004), dict(sub=None), dict(raw_size=5 * 4096), dict(blocksize=0), dict(totals=None), dict(delims=None),
                dict(alts=alts_of([b"a"], [b""])), dict(alts=alts_of([b"x"] * 35, [b"y"] * 35)), dict(alts=alts_of([b"a\n"], [b"b"])),
                dict(alts=alts_of([b"a", b"c"], [b"b", b""])), dict(nblocks=0), dict(nblocks=0, raw_size=0, stream=None, index=None, sub=None, errs=None)]
    for i, a in enumerate(mistakes):
        for b in mistakes[i:]:
            kw = {**dict(alts=good), **a, **b}
            rc, msg = call(lib, ta=(1, 1) if two else (2,), mode=mode, **kw)
            rc0, other = older_call(lib, "find_records_context", **kw)
            assert rc == rc0 == HUFE_ARGUMENT and msg == other.replace("find_records_context:", WHO), (kw, msg, other)
    for select in (2, 3, 0x80000000):
        rc, msg = call(lib, select=select, mode=7, ta=None)
        assert msg == older_call(lib, "find_records_context", select=select)[1].replace("find_records_context:", WHO)


def test_the_older_calls_keep_their_wording(lib):
    for older in cases.WORDING:
        cases.the_call_keeps_its_wording(lib, older)


# ---- the Python patterns ---------------------------------------------------------------------------------------------------
def test_allof_and_seq_and_their_errors():
    bare = GpuCodec.__new__(GpuCodec)                       # the checks below speak before the context is looked at
    args = (None, 0, None, 0, None, 0, 4096)
    records = ((bare.find_records, ()), (bare.count_records, ()), (bare.grep, (4, 16)))
    for kind in (AllOf, Seq):
        two = kind(b"ab", b"cd")
        assert len(two) == 2 and list(two) == [b"ab", b"cd"] and repr(two) == kind.__name__ + "(b'ab', b'cd')"
        for f in (bare.find_pattern, bare.count_pattern):
            with pytest.raises(TypeError, match=kind.__name__):
                f(*args, two)
            with pytest.raises(TypeError, match=kind.__name__):
                f(*args, kind(b"ab"))
        for f, more in records:
            for kw in (dict(word=True), dict(whole_line=True), dict(bol=True), dict(eol=True), dict(word=True, word_bytes=b"ab")):
                with pytest.raises(ValueError, match="anchored"):
                    f(*args, two, *more, **kw)
                with pytest.raises(ValueError, match="anchored"):
                    f(*args, kind(b"ab"), *more, **kw)
            with pytest.raises(ValueError, match="1 to 4 items, not 5"):
                f(*args, kind(b"a", b"b", b"c", b"d", b"e"), *more)
            with pytest.raises(ValueError, match="1 to 4 items, not 0"):
                f(*args, kind(), *more)
            with pytest.raises(TypeError, match="do not nest"):
                f(*args, kind(b"a", AllOf(b"b", b"c")), *more)
            with pytest.raises(TypeError, match="do not nest"):
                f(*args, kind(Seq(b"b", b"c")), *more)
            with pytest.raises(TypeError, match="not a " + kind.__name__):
                f(*args, AnyOf(b"a", kind(b"b", b"c")), *more)
            with pytest.raises(TypeError, match="not a " + kind.__name__):
                f(*args, AllOf(b"x", AnyOf(b"a", kind(b"b", b"c"))), *more)
            with pytest.raises(ValueError, match="holds a delimiter"):
                f(*args, kind(b"ab", b"c\nd"), *more)
            with pytest.raises(ValueError, match="sum to 65"):
                f(*args, kind(b"x" * 33, b"y" * 32), *more)
            with pytest.raises(ValueError, match="no alternative"):
                f(*args, kind(b"ab", AnyOf()), *more)
            with pytest.raises(TypeError):
                f(*args, kind(b"ab", "text"), *more)
    for f, more in records:
        with pytest.raises(ValueError, match="item 1 of Seq has alternatives of the lengths \\[2, 3\\]"):
            f(*args, Seq(b"ab", AnyOf(b"cd", b"efg")), *more)
        with pytest.raises(ValueError, match="item 0 of Seq"):
            f(*args, Seq(AnyOf(b"cd", [b"e", b"f", b"g"])), *more)
    anchors = (False,) * 4 + (None,)
    key, st, counts, n, mode = GpuCodec._find_terms(AllOf(b"ab", AnyOf(b"cd", b"efg"), [b"xy", b"z"]), True, b"\n", anchors)
    assert (np.frombuffer(counts, np.uint32).tolist(), n, mode) == ([1, 2, 1], 3, ALL)
    assert np.frombuffer(key[1], np.uint32).tolist() == [2, 2, 3, 2] and key[2] == 4 and st == GpuCodec.byte_set(b"\n")
    assert key == GpuCodec._find_route(AnyOf(b"ab", b"cd", b"efg", [b"xy", b"z"]), True, b"\n", True)[1]
    assert GpuCodec._find_terms(Seq(b"ab", AnyOf(b"cd", b"ef")), False, b"\n", anchors)[2:] == (np.array([1, 2], np.uint32).tobytes(), 2, ORDERED)


# ---- the model -------------------------------------------------------------------------------------------------------------
def starts(data, terms, mode, **kw):
    data = np.frombuffer(data, np.uint8)
    return find_terms_model(data, terms, b"\n", 0, data.size, mode=mode, **kw)[0].tolist()


def test_the_model_by_hand():
    ab_bc, aa_aa = [[b"ab"], [b"bc"]], [[b"aa"], [b"aa"]]
    assert starts(b"abc\nabbc\nbcab\n", ab_bc, ORDERED) == [4]                  # "abc" holds both, not one behind the other
    assert starts(b"abc\nabbc\nbcab\n", ab_bc, ALL) == [0, 4, 9]
    assert starts(b"abc\nabbc\nbcab\nxx\n\n", ab_bc, ORDERED, invert=True) == [0, 9, 14]      # (no empty record)
    assert starts(b"aaa\naaaa\naa\n", aa_aa, ORDERED) == [4]
    assert starts(b"aaa\naaaa\naa\n", aa_aa, ALL) == [0, 4, 9]                    # the same bytes serve both terms
    assert starts(b"abc\nab\nbc", [[b"ab"], [b"abc"]], ALL) == [0]                # as grep ab | grep abc
    assert starts(b"abc\nab\nbc", [[b"ab"], [b"abc"]], ORDERED) == []
    assert starts(b"b a\na b\nb\na", [[b"a"], [b"b"]], ORDERED) == [4]            # nothing is borrowed across a delimiter
    assert starts(b"b a\na b\nb\na", [[b"a"], [b"b"]], ALL) == [0, 4]
    abc = [[b"A"], [b"B"], [b"C"]]
    assert starts(b"A C B C\nA C B\nCBA\nABC", abc, ORDERED) == [0, 18]
    assert starts(b"A C B C\nA C B\nCBA\nABC", abc, ALL) == [0, 8, 14, 18]
    assert starts(b"xd yb\nxc ya\nyb xd", [[b"xc", b"xd"], [b"ya", b"yb"]], ORDERED) == [0, 6]       # the second alternative alone
    assert starts(b"ab b ab", [[b"b"], [b"ab"]], ORDERED) == [0]                  # the "ab" at 0 lies in front of every "b": a later one fits
    assert starts(b"ab", [[b"b"], [b"ab"]], ORDERED) == []
    with pytest.raises(ValueError, match="one length"):
        starts(b"abcd", [[b"abcd", b"bc"], [b"d"]], ORDERED)
    # ... which is why: the leftmost occurrence of ("abcd" or "bc") ends behind the later, shorter one
    data = np.frombuffer(b"abcd", np.uint8)
    assert satisfying(data, [[b"abcd", b"bc"], [b"d"]], b"\n", ALL)[2].tolist() == [True]
    # context, numbers and flags are the context call's
    got = find_terms_model(np.frombuffer(b"x\nab bc\ny\n\nz\nbc ab\n", np.uint8), ab_bc, b"\n", 0, 9, mode=ORDERED, before=1, after=2)
    assert got[0].tolist() == [0, 2, 8] and got[4].tolist() == [0, 1, 2] and got[5].tolist() == [0, 1, 0]


def literal_regex(term):
    return b"(?:" + b"|".join(re.escape(a) for a in term) + b")"


@MODES
@pytest.mark.parametrize("nterms", [2, 3, 4])
def test_the_model_against_re_on_random_data(mode, nterms):
    """per line: all(re.search(t, line) for t) for AllOf, re.search(b"(?:a|b).*(?:c|d)", line) for Seq; `re` is the reference"""
    rng = np.random.default_rng(900 + 10 * nterms + mode)
    letters = np.frombuffer(b"abcd\n", np.uint8)
    seen = {False: 0, True: 0}
    for trial in range(30):
        n, bs = int(rng.integers(1, 500)), int(rng.integers(0, 70))
        data = rng.choice(letters, n, p=[0.25, 0.25, 0.2, 0.2, 0.1]).astype(np.uint8)
        terms = []
        for _ in range(nterms):
            m = int(rng.integers(1, 4))                     # literal terms of 1 to 3 bytes, one length a term
            terms.append([bytes(rng.choice(letters[:4], m).astype(np.uint8)) for _ in range(int(rng.integers(1, 3)))])
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, np.arange(nb) != int(rng.integers(0, nb)), rng.integers(0, 4, nb) != 0):
            ok = [True] * nb if served is None else list(served)
            for invert in (False, True):
                want, s = [], 0
                for line in bytes(data).split(b"\n"):
                    e = s + len(line)
                    if s < n and e > s and all(ok[b] for b in range(max(s - 1, 0) // (bs or n), min(e, n - 1) // (bs or n) + 1)):
                        if mode == ALL:
                            holds = all(re.search(literal_regex(t), line) for t in terms)
                        else:
                            holds = re.search(b".*".join(literal_regex(t) for t in terms), line) is not None
                        if holds != invert:
                            want.append(s)
                        seen[holds] += 1
                    s = e + 1
                got = find_terms_model(data, terms, b"\n", bs, n, 0, served, invert, mode=mode)
                assert got[0].tolist() == want, (bytes(data), terms, bs, served, invert)
                assert got[3].tolist() == [len(want), len(want), nb - sum(ok), 0]
    assert seen[True] > 20 and seen[False] > 20


@MODES
def test_one_term_is_the_context_model(mode):
    rng = np.random.default_rng(78)
    for trial in range(12):
        n, bs = int(rng.integers(1, 300)), int(rng.integers(0, 50))
        data = rng.choice(np.frombuffer(b"abc\n", np.uint8), n).astype(np.uint8)
        alts = [[b"ab", b"c"], [b"a", b"b"]] if mode == ORDERED else [[b"ab", b"c"], [b"a"]]
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 4, nb) != 0
        a = find_terms_model(data, [alts], b"\n", bs, n, 3, served, bool(trial & 1), 1, 2, mode)
        b = find_context_model(data, alts, b"\n", bs, n, 3, served, bool(trial & 1), 1, 2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))

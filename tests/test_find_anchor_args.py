"""hufgpu_find_any_anchored and hufgpu_find_records_anchored: their declarations, the checks of the arguments of their own, the
NumPy models of their results (tests/find_anchor_model.py) and the `bol` / `eol` / `whole_line` / `word` / `word_bytes`
keywords of GpuCodec (no GPU needed).  The checks they share with the other calls of the search family, with and without
anchors, are the functions of tests/find_args_cases.py.  The models are checked against Python's `re`: look-behind and look-ahead
assertions around an alternative for the positions, `bytes.split` and the same expression a piece for the records.
"""
import inspect
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
from find_anchor_model import BOL, EOL, WORD, anchored_hits, find_any_anchored_model, find_records_anchored_model
from find_any_model import alt_tables, find_any_model
from find_args_support import HUFE_ARGUMENT, LAYOUTS, NEWLINE, ROOT, WORDS, alts_of, bracket, call, lib, regex, valid
from find_context_model import find_context_model
from find_model import byte_set
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

AnyOf = GpuCodec.AnyOf
ANCHORS = [0, BOL, EOL, WORD, BOL | EOL, BOL | WORD, EOL | WORD, 7]
EVERY = pytest.mark.parametrize("anchors", ANCHORS)


def call_pos(lib, older=False, **kw):
    return call(lib, "find_any" if older else "find_any_anchored", **kw)


def call_rec(lib, older=False, **kw):
    return call(lib, "find_records_context" if older else "find_records_anchored", **kw)


CALLS = [(call_pos, "find_any_anchored:", "find_any:"), (call_rec, "find_records_anchored:", "find_records_context:")]
BOTH = pytest.mark.parametrize("call,who,was", CALLS, ids=["positions", "records"])


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_declared(lib):
    """hufgpu_find_any's arguments with (delim_set, word_set, anchors) behind n_alts: 21; the context call's with (word_set,
    anchors) behind n_alts: 28"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    for name, sibling, nargs, more in (("hufgpu_find_any_anchored", "hufgpu_find_any", 21,
                                        "const uint8_t delim_set[32], const uint8_t word_set[32], uint32_t anchors,"),
                                       ("hufgpu_find_records_anchored", "hufgpu_find_records_context", 28,
                                        "const uint8_t word_set[32], uint32_t anchors,")):
        assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
        mine, theirs = list(getattr(lib, name).argtypes), list(getattr(lib, sibling).argtypes)
        at = 11 if nargs == 21 else 12                      # behind n_alts
        assert len(mine) == nargs and mine[:at] == theirs[:at] and mine[at + nargs - len(theirs):] == theirs[at:]
        vp, u32 = theirs[1], theirs[at - 1]
        assert mine[at:at + nargs - len(theirs)] == ([vp, vp, u32] if nargs == 21 else [vp, u32])
        assert getattr(lib, name).restype is getattr(lib, sibling).restype
        m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        assert m and m.group(0).count(",") == nargs - 1
        s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t n_alts,", "uint32_t n_alts, " + more)
        assert want == re.sub(r"\s+", " ", m.group(1))
        assert header.index(name + "(hufgpu_ctx_t") > header.index("hufgpu_find_records_context(hufgpu_ctx_t")
    assert (_native.ANCHOR_BOL, _native.ANCHOR_EOL, _native.ANCHOR_WORD) == (BOL, EOL, WORD) == (1, 2, 4)
    for name, value in (("BOL", 1), ("EOL", 2), ("WORD", 4)):
        assert re.search(r"#define\s+HUFGPU_ANCHOR_%s\s+%du\b" % (name, value), header)
    doc = header[header.index("FIND, ANCHORED"):header.index("hufgpu_find_any_anchored(hufgpu_ctx_t")]
    assert "OUT OF SCOPE" in doc and "per alternative" in doc and "variable length" in doc and "INSIDE a pattern" in doc


# ---- the older calls' arguments, in their order ----------------------------------------------------------------------------
@BOTH
@EVERY
def test_null_arrays_counts_lengths_and_classes(lib, call, who, was, anchors):
    name, kw = who[:-1], dict(anchors=anchors)
    cases.null_arrays_and_counts_of_0_and_65(lib, name, kw)
    cases.an_alternative_of_length_0(lib, name, kw, [3, 0, 2], 1)
    cases.a_total_above_64(lib, name, kw, [32, 33])
    cases.an_empty_class(lib, name, kw, *cases.EMPTY_CLASSES[-1])


@EVERY
def test_the_records_call_s_delimiters(lib, anchors):
    """... and an unknown select bit is refused in front of everything else, the anchors included; the numbers and the flags
    are optional"""
    who = "find_records_anchored:"
    for select in (0, 1):
        cases.a_class_that_meets_the_delimiter_set(lib, who[:-1], dict(anchors=anchors, select=select), *cases.DELIMITER_CLASSES[-1])
    cases.a_null_delimiter_set(lib, who[:-1], dict(anchors=anchors))
    cases.the_full_class_and_the_delimiter_set(lib, who[:-1], dict(anchors=anchors))
    for select in (2, 3, 0x80000000, 0xFFFFFFFE):           # the first check of all
        for more in (dict(), dict(cls=None, totals=None), dict(anchors=8), dict(words=None, anchors=WORD)):
            rc, msg = call_rec(lib, **{**dict(anchors=anchors, select=select), **more})
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and "select 0x%x" % select in msg and "HUFGPU_SELECT_INVERT" in msg
    for ba in ((0, 0), (0, 1), (2**32 - 1, 2**32 - 1)):
        for out in (dict(), dict(no=None), dict(sel=None), dict(no=None, sel=None, cap=0, pos=None, rlens=None, counts=None)):
            assert valid(*call_rec(lib, anchors=anchors, ba=ba, **out), who)


@BOTH
@EVERY
def test_caps_layouts_and_device_arrays(lib, call, who, was, anchors):
    name, kw = who[:-1], dict(anchors=anchors)
    cases.a_cap_without_its_outputs(lib, name, kw)
    for missing in cases.NULL_ARRAYS:
        cases.null_device_arrays(lib, name, kw, missing)
    cases.missing_or_misaligned_sub_index(lib, name, kw)
    for layout in cases.BAD_LAYOUTS:
        cases.a_layout_that_does_not_give_nblocks(lib, name, kw, layout)
    cases.valid_arguments_still_need_a_context(lib, name, kw)


@BOTH
@pytest.mark.parametrize("anchors", [0, BOL, 7])
def test_the_order_of_the_checks_is_the_older_call_s(lib, call, who, was, anchors):
    """every pair of mistakes: the anchored call and the older one complain about the same one"""
    mistakes = [dict(cls=None), dict(n=0), dict(pos=None), dict(index=None), dict(sub=0x30004), dict(raw_size=5 * 4096), dict(totals=None),
                dict(alts=alts_of([b"a", b""])), dict(alts=alts_of([b"x"] * 40, [b"y"] * 30))]
    if call is call_rec:
        mistakes += [dict(select=2), dict(delims=None), dict(alts=alts_of([b"a\n"]))]
    for i, a in enumerate(mistakes):
        for b in mistakes[i:]:
            kw = {**a, **b}
            rc, msg = call(lib, anchors=anchors, **kw)
            other = call(lib, older=True, **kw)[1]
            assert rc == HUFE_ARGUMENT and msg == other.replace(was, who), (kw, msg, other)


def test_the_older_calls_keep_their_wording(lib):
    for older in ("find_any", "find_records_context"):
        cases.the_call_keeps_its_wording(lib, older)


# ---- the four new errors -------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("anchors", [8, 9, 16, 0x80000000, 0xFFFFFFFF, 0xFFFFFFF8])
def test_an_unknown_anchor_bit(lib, call, who, was, anchors):
    for nblocks, raw_size in LAYOUTS:
        for more in (dict(), dict(words=None), dict(cls=None, totals=None), dict(delims=None)):
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, anchors=anchors, **more)
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg
            assert "anchors 0x%x" % anchors in msg and "HUFGPU_ANCHOR_WORD" in msg


@pytest.mark.parametrize("anchors", ANCHORS)
def test_the_sets_an_anchor_needs(lib, anchors):
    for nblocks, raw_size in LAYOUTS:
        kw = dict(nblocks=nblocks, raw_size=raw_size, anchors=anchors)
        rc, msg = call_pos(lib, delims=None, **kw)
        if anchors & (BOL | EOL):
            assert rc == HUFE_ARGUMENT and msg.startswith("find_any_anchored:") and "need the delim_set" in msg and "needs a context" not in msg
            assert "need the delim_set" in call_pos(lib, delims=None, words=None, cls=None, **kw)[1]        # in front of the older checks
        else:
            assert valid(rc, msg, "find_any_anchored:")
        for call, who, _ in CALLS:
            rc, msg = call(lib, words=None, **kw)
            if anchors & WORD:
                assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs the word_set" in msg and "needs a context" not in msg
                assert "needs the word_set" in call(lib, words=None, cls=None, totals=None, **kw)[1]
            else:
                assert valid(rc, msg, who)
    if anchors == 0:                                        # the sets are not looked at
        assert valid(*call_pos(lib, delims=None, words=None, anchors=0), "find_any_anchored:")


@BOTH
def test_the_budget_of_the_matcher_s_state(lib, call, who, was):
    """with EOL or WORD every alternative takes one bit more: sum(alt_lens) + n_alts <= 64; BOL alone costs nothing"""
    fits, over = ([63], [31, 31], [1] * 32), ([64], [32, 31], [1] * 33)
    for lens in fits + over:
        alts = alts_of(*[[b"x"] * m for m in lens])
        total = sum(lens) + len(lens)
        for anchors in ANCHORS:
            for nblocks, raw_size in LAYOUTS:
                rc, msg = call(lib, alts=alts, anchors=anchors, nblocks=nblocks, raw_size=raw_size)
                if lens in over and anchors & (EOL | WORD):
                    assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg, (lens, anchors, msg)
                    assert "sum to %d" % total in msg and "above 64" in msg and "boundary" in msg
                else:
                    assert valid(rc, msg, who), (lens, anchors, msg)
    rc, msg = call(lib, alts=alts_of([b"x"] * 64, [b"y"]), anchors=WORD)       # the older total speaks first
    assert "alternatives sum to 65" in msg and "boundary" not in msg
    rc, msg = call(lib, alts=alts_of([b"x"] * 64, [b""]), anchors=WORD)        # ... and `classes` is not read in front of either
    assert "sum to 65" in msg


# ---- the Python keywords -------------------------------------------------------------------------------------------------
def test_the_keywords_and_their_value_errors():
    names = ["bol", "eol", "whole_line", "word", "word_bytes"]
    for name in ("find_records", "count_records", "grep"):
        p = list(inspect.signature(getattr(GpuCodec, name)).parameters)
        at = p.index("context")
        assert p[at + 1:] == names + ["invert", "line_numbers"], name
    for name in ("find_pattern", "count_pattern"):
        p = list(inspect.signature(getattr(GpuCodec, name)).parameters)
        assert p[p.index("ignore_case") + 1:] == names + ["delimiters"], name
    for name in ("find_records", "count_records", "grep", "find_pattern", "count_pattern"):
        p = inspect.signature(getattr(GpuCodec, name)).parameters
        assert all(p[k].default is False for k in names[:4]) and p["word_bytes"].default is None and p["delimiters"].default == b"\n"
    assert sorted(GpuCodec.WORD_BYTES) == sorted(v for v in range(128) if re.match(rb"\w", bytes([v])))
    bare = GpuCodec.__new__(GpuCodec)                       # the checks below speak before the context is looked at
    args = (None, 0, None, 0, None, 0, 4096)
    for kw in (dict(word_bytes=b"abc"), dict(word_bytes=b"abc", bol=True), dict(word_bytes=b"", whole_line=True)):
        for f, more in ((bare.find_records, ()), (bare.count_records, ()), (bare.grep, (4, 16)), (bare.find_pattern, ()), (bare.count_pattern, ())):
            with pytest.raises(ValueError, match="word_bytes"):
                f(*args, b"x", *more, **kw)
    for kw in (dict(word=True), dict(eol=True), dict(whole_line=True), dict(word=True, bol=True)):
        for pattern, total in ((b"x" * 64, 65), (AnyOf(b"x" * 32, b"y" * 31), 65), (AnyOf(*[b"x"] * 33), 66)):
            for f, more in ((bare.find_records, ()), (bare.grep, (4, 16)), (bare.find_pattern, ()), (bare.count_pattern, ())):
                with pytest.raises(ValueError, match="sum to %d" % total):
                    f(*args, pattern, *more, **kw)
    with pytest.raises(ValueError, match="class 1 of alternative 0 holds a delimiter"):
        bare.find_records(*args, b"a\nb", word=True)
    with pytest.raises(ValueError, match="out of range"):
        bare.find_records(*args, b"ab", word=True, word_bytes=[300])
    with pytest.raises(TypeError):
        bare.find_records(*args, "text", word=True)
    for pattern in (b"x" * 64, AnyOf(b"x" * 32, b"y" * 32)):       # BOL alone costs nothing
        route, key, st, (bits, ws) = GpuCodec._find_route(pattern, False, b"\n", False, (True, False, False, False, None))
        assert route == "any" and bits == BOL and ws is None
    route, key, st, (bits, ws) = GpuCodec._find_route(b"ab", True, b"\n", False, (False, False, True, True, b"ab_"))
    assert (route, bits, ws, st) == ("any", 7, byte_set(b"ab_"), NEWLINE) and key[2] == 1
    assert GpuCodec._find_route(b"ab", False, b"\n", False, (False,) * 4 + (None,)) == GpuCodec._find_route(b"ab", False, b"\n") + ((0, None),)
    assert GpuCodec._find_route(b"ab", False, anchors=(False,) * 4 + (None,))[0] == "literal"        # what is called today
    assert GpuCodec._find_route(b"ab", False, b"\n", False, (False, False, False, True, None))[3] == (WORD, WORDS)


# ---- the models against `re` ---------------------------------------------------------------------------------------------
def cls_of(values):
    return bracket(sorted(set(bytes(values)))) if len(values) else b"(?!)"     # (an empty set: a class that nothing is in)


def anchored_regex(sets, delims, words, anchors):
    """one alternative between its assertions"""
    front = (b"(?<!" + cls_of(words) + b")" if anchors & WORD and len(words) else b"") + \
            (b"(?:^|(?<=" + cls_of(delims) + b"))" if anchors & BOL else b"")
    behind = (b"(?!" + cls_of(words) + b")" if anchors & WORD and len(words) else b"") + \
             (b"(?=" + cls_of(delims) + rb"|\Z)" if anchors & EOL else b"")
    return front + b"(?:" + regex(sets) + b")" + behind


def re_positions(data, alts, delims, words, anchors, blocksize, cap=0, served=None):
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    found = set()
    for sets in alts:
        for hit in re.finditer(b"(?=(" + anchored_regex(sets, delims, words, anchors) + b"))", raw, re.DOTALL):
            p = hit.start()
            lo = p - 1 if p > 0 and anchors & (BOL | WORD) else p
            hi = p + len(sets) if p + len(sets) < n and anchors & (EOL | WORD) else p + len(sets) - 1
            if all(served[b] for b in range(lo // bs, hi // bs + 1)):
                found.add(p)
    pos, counts = sorted(found), [0] * nb
    for p in pos:
        counts[p // bs] += 1
    written = min(len(pos), cap)
    return pos[:written], counts, [len(pos), written, nb - sum(served), 0]


def re_records(data, alts, delims, words, anchors, blocksize, served=None, invert=False):
    """the starts of the selected records over bytes.split: a piece of known extent is selected when the anchored expression
    - with its look-behind and look-ahead into the bytes around the piece: a delimiter may be a word byte - starts in it"""
    raw, n = bytes(data), len(data)
    assert len(delims) == 1
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    want = re.compile(b"(?=(" + b"|".join(anchored_regex(sets, delims, words, anchors) for sets in alts) + b"))", re.DOTALL)
    at = [m.start() for m in want.finditer(raw)]           # (over the whole data: the look-arounds see the neighbours)
    out, s = [], 0
    for piece in raw.split(bytes(delims)) if n else []:
        e = s + len(piece)
        if s < n and e > s and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            if any(s <= p < e for p in at) != invert:
                out.append(s)
        s = e + 1
    return out


def same(data, alts, delims, words, anchors, blocksize, served=None):
    data = np.frombuffer(data, np.uint8) if isinstance(data, bytes) else np.asarray(data, np.uint8)
    n = int(data.size)
    got = find_any_anchored_model(data, alts, delims, words, anchors, blocksize, n, served)
    want = re_positions(data, alts, delims, words, anchors, blocksize, n, served)
    assert tuple(g.tolist() for g in got) == want, (bytes(data), alts, delims, words, anchors, blocksize, served)
    if len(delims) == 1 and not any(delims[0] in s for a in alts for s in a):
        for invert in (False, True):
            rec = find_records_anchored_model(data, alts, delims, words, anchors, blocksize, n, 0, served, invert)
            assert rec[0].tolist() == re_records(data, alts, delims, words, anchors, blocksize, served, invert), (bytes(data), alts, anchors, invert)
            assert rec[5].all()
    return want[0]


W = b"abcdefghijklmnopqrstuvwxyz_"


def test_the_model_by_hand():
    lit = lambda *words: [[bytes([v]) for v in w] for w in words]
    foo = lit(b"foo")
    assert same(b"foo", foo, b"\n", W, 7, 0) == [0]                            # the whole data
    assert same(b"foo bar\nfoo", foo, b"\n", W, WORD, 4) == [0, 8]             # a hit at byte 0 and at the last byte
    assert same(b"foo bar\nfoo", foo, b"\n", W, BOL, 4) == [0, 8]
    assert same(b"foo bar\nfoo", foo, b"\n", W, EOL, 4) == [8]
    assert same(b"foo bar\nfoo", foo, b"\n", W, BOL | EOL, 4) == [8]
    assert same(b"foofoo foo", foo, b"\n", W, WORD, 0) == [7]
    assert same(b"foofoo foo", foo, b"\n", W, 0, 0) == [0, 3, 7]
    data = np.frombuffer(b"xfoofoo foo\nfoofoo\n", np.uint8)
    assert find_records_anchored_model(data, foo, b"\n", W, WORD, 0, 9)[0].tolist() == [0]      # as GNU grep -w
    assert find_records_anchored_model(data, foo, b"\n", W, WORD, 0, 9, invert=True)[0].tolist() == [12]
    assert find_records_anchored_model(data, foo, b"\n", W, BOL, 0, 9)[0].tolist() == [12]
    assert find_records_anchored_model(data, foo, b"\n", W, EOL, 0, 9)[0].tolist() == [0, 12]
    assert find_records_anchored_model(data, foo, b"\n", W, BOL | EOL, 0, 9)[0].tolist() == []
    ab = lit(b"ab", b"abc")                                                    # one start, two alternatives, one qualifies
    assert same(b"abc abd ab", ab, b"\n", W, WORD, 0) == [0, 8]
    assert same(b"abc\nab\nabcd", ab, b"\n", W, EOL, 0) == [0, 4]
    assert same(b"abc\nab\nabcd", ab, b"\n", W, BOL | EOL, 0) == [0, 4]
    assert same(b"ab_ab\nab", ab, b"_", W, EOL | WORD, 0) == [6]                # D within W: only the data's end is left behind a match
    assert same(b"ab ab_ab", ab, b"_", W, BOL | WORD, 0) == [0]                 # ... and only its start in front of one
    assert same(b"ab_ab_ab", ab, b"_", W, BOL, 0) == [0, 3, 6]                  # a delimiter that is a word byte
    assert same(b"ab_ab_ab", ab, b"_", W, WORD, 0) == []
    assert same(b"ab ab", ab, b"\n", b"", WORD, 0) == [0, 3]                    # no word bytes: every occurrence
    assert same(b"ab ab", ab, b"", W, BOL | EOL, 0) == []                       # no delimiters: the data is one record
    assert same(b"ab", ab, b"", W, BOL | EOL, 0) == [0]
    # [xx a][b yy]: the hit's bytes lie in both blocks; [x ab][ yyy]: the right neighbour alone lies in block 1
    for data, bs, left_in, right_in in ((b"xx ab yy", 4, 0, 1), (b"x ab yyy", 4, 0, 1), (b"xxx ab y", 4, 0, 1), (b"xxxx ab yy", 4, 0, 1)):
        for bad in range((len(data) + bs - 1) // bs):
            served = [b != bad for b in range((len(data) + bs - 1) // bs)]
            p = data.index(b"ab")
            for anchors in ANCHORS:
                lo = p - 1 if anchors & (BOL | WORD) else p
                hi = p + 2 if anchors & (EOL | WORD) else p + 1
                qualifies = anchors & (BOL | EOL) == 0
                got = same(data, lit(b"ab"), b"\n", W, anchors, bs, served)
                assert got == ([p] if qualifies and not lo // bs <= bad <= hi // bs else []), (data, bad, anchors)


@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
@pytest.mark.parametrize("anchors", ANCHORS)
def test_the_model_on_random_data(alphabet, anchors):
    rng = np.random.default_rng(4000 + anchors + len(alphabet))
    seen = 0
    for trial in range(16):
        n, bs = int(rng.integers(1, 400)), int(rng.integers(0, 60))
        if alphabet == "four letters":                      # four letters and two word bytes that are none of them
            values, p = np.frombuffer(b"abc\nxy", np.uint8), [0.25, 0.25, 0.2, 0.1, 0.1, 0.1]
            data = rng.choice(values, n, p=p).astype(np.uint8)
            alts = [[bytes(rng.choice(values[:3], int(rng.integers(1, 3)), replace=False).astype(np.uint8)) for _ in range(m)]
                    for m in [(1,), (2, 3), (1, 2, 2), (5,)][trial % 4]]
            words = [b"xy", b"abcxy", b"", b"xy\n"][trial % 4]     # ... a delimiter that is a word byte
        else:
            data = rng.integers(0, 256, n).astype(np.uint8)
            data[rng.integers(0, n, n // 5 + 1)] = 10
            alts = [[bytes(v for v in range(256) if v != 10 and rng.integers(0, 3)) or b"\x01" for _ in range(m)] for m in [(1,), (2, 1)][trial % 2]]
            words = bytes(v for v in range(256) if rng.integers(0, 2))
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, np.arange(nb) != int(rng.integers(0, nb)), rng.integers(0, 4, nb) != 0):
            seen += len(same(data, alts, b"\n", words, anchors, bs, served))
    assert seen > 0


def test_no_anchor_is_the_older_models():
    rng = np.random.default_rng(77)
    for trial in range(10):
        n, bs = int(rng.integers(1, 300)), int(rng.integers(0, 50))
        data = rng.choice(np.frombuffer(b"abc\n", np.uint8), n).astype(np.uint8)
        alts = [[b"ab", b"c"], [b"a"]]
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 4, nb) != 0
        a, b = find_any_anchored_model(data, alts, b"\n", W, 0, bs, n, served), find_any_model(data, alts, bs, n, served)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        a = find_records_anchored_model(data, alts, b"\n", W, 0, bs, n, 3, served, bool(trial & 1), 1, 2)
        b = find_context_model(data, alts, b"\n", bs, n, 3, served, bool(trial & 1), 1, 2)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert anchored_hits(data, alt_tables(alts), b"\n", W, 0).sum() >= anchored_hits(data, alt_tables(alts), b"\n", W, WORD).sum()

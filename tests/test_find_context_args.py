"""hufgpu_find_records_context: its declaration, the checks of the arguments of its own, the NumPy model of its results
(tests/find_context_model.py) and the `before` / `after` / `context` keywords of GpuCodec (no GPU needed).  The checks it
shares with the other calls of the search family, for distances of 0 and others, are the functions of tests/find_args_cases.py.  The
model is checked against plain Python over `bytes.split`: the indices of the selected pieces, a window around each, the
union, the empty pieces dropped.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
import find_args_support
from find_args_support import FAR, HUFE_ARGUMENT, LAYOUTS, ROOT, alts_of, lib, random_case, regex, valid
from find_context_model import find_context_model
from find_select_model import NO_UNKNOWN, find_select_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

WHO = "find_records_context:"
AnyOf = GpuCodec.AnyOf
NAME = "find_records_context"
call = functools.partial(find_args_support.call, name=NAME)
DISTANCES = [(0, 1), (1, 0), (2, 2), (0, 5), (7, 0), (3, 40), (FAR, FAR)]
WINDOWS = pytest.mark.parametrize("ba", [(0, 0), (2, 3), (FAR, FAR)], ids=["select", "2-3", "all"])


# ---- the symbol ----------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared(lib):
    """hufgpu_find_records_select's arguments with `before`, `after` behind select and `d_rec_sel` behind d_rec_no: 26"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    name, sibling = "hufgpu_find_records_context", "hufgpu_find_records_select"
    assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
    mine, theirs = list(getattr(lib, name).argtypes), list(getattr(lib, sibling).argtypes)
    assert len(mine) == 26 == len(theirs) + 3
    u32, vp = type(theirs[12]), theirs[15]
    assert mine == theirs[:13] + [theirs[12], theirs[12]] + theirs[13:16] + [vp] + theirs[16:] and u32 is type(mine[13])
    assert getattr(lib, name).restype is getattr(lib, sibling).restype
    m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 25
    s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t select,", "uint32_t select, uint32_t before, uint32_t after,")
    want = want.replace("uint64_t *d_rec_no,", "uint64_t *d_rec_no, uint8_t *d_rec_sel,")
    assert want == re.sub(r"\s+", " ", m.group(1))
    assert header.index(name + "(hufgpu_ctx_t") > header.index(sibling + "(hufgpu_ctx_t")
    doc = header[header.index("FIND RECORDS, WITH CONTEXT"):header.index(name + "(hufgpu_ctx_t")]
    assert "EMPTY records" in doc and "distances count them" in doc and "no\n *                   context of their own" in doc
    assert "hufgpu_find_records_context(): the distances COUNT empty records" in header     # next to the older note


# ---- the new arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", [2, 3, 4, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE])
def test_an_unknown_select_bit(lib, select):
    for nblocks, raw_size in LAYOUTS:
        for ba in ((0, 0), (1, 0), (FAR, FAR)):
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, select=select, ba=ba)
            assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "needs a context" not in msg, msg
            assert "select 0x%x" % select in msg and "HUFGPU_SELECT_INVERT" in msg
    rc, msg = call(lib, select=select, cls=None, totals=None)   # ... and it is the first check of all
    assert "select 0x%x" % select in msg


@pytest.mark.parametrize("select", [0, 1])
@WINDOWS
def test_the_numbers_and_the_flags_are_optional(lib, select, ba):
    for out in (dict(), dict(no=None), dict(sel=None), dict(no=None, sel=None)):
        for kw in (dict(), dict(cap=0), dict(cap=0, pos=None, rlens=None)):
            assert valid(*call(lib, select=select, ba=ba, **out, **kw), WHO), (out, kw)
        rc, msg = call(lib, select=select, ba=ba, pos=None, **out)      # neither stands in for one of the two other outputs
        assert rc == HUFE_ARGUMENT and "needs d_rec_pos and d_rec_len" in msg and msg.startswith(WHO)


@pytest.mark.parametrize("ba", [(0, 0), (0, 1), (1, 0), (0x80000000, 5), (FAR, 0), (0, FAR), (FAR, FAR)])
def test_any_distance_is_valid(lib, ba):
    for select in (0, 1):
        assert valid(*call(lib, select=select, ba=ba), WHO)


# ---- the older checks, in the older order ------------------------------------------------------------------------------------


def test_the_order_of_the_checks_is_the_select_call_s(lib):
    """every pair of mistakes: both calls complain about the same one"""
    mistakes = [dict(select=2), dict(cls=None), dict(n=0), dict(delims=None), dict(pos=None), dict(index=None), dict(sub=0x30004),
                dict(raw_size=5 * 4096), dict(alts=alts_of([b"a\n"]))]
    for i, a in enumerate(mistakes):
        for b in mistakes[i:]:
            kw = {**a, **b}
            rc, msg = call(lib, **kw)
            other = find_args_support.call(lib, "find_records_select", **kw)[1]
            assert rc == HUFE_ARGUMENT and msg == other.replace("find_records_select:", WHO), (kw, msg, other)


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
BOTH_SELECTS = (0, 1)


@WINDOWS
def test_null_arrays_and_counts_of_0_and_65(lib, ba):
    cases.null_arrays_and_counts_of_0_and_65(lib, NAME, dict(ba=ba))


@WINDOWS
def test_lengths_classes_and_delimiters(lib, ba):
    kw = dict(ba=ba)
    cases.an_alternative_of_length_0(lib, NAME, kw, [3, 0, 2], 1)
    cases.a_total_above_64(lib, NAME, kw, [32, 33])
    cases.an_empty_class(lib, NAME, kw, *cases.EMPTY_CLASSES[-1])
    for select in BOTH_SELECTS:
        cases.a_class_that_meets_the_delimiter_set(lib, NAME, dict(ba=ba, select=select), *cases.DELIMITER_CLASSES[-1])
    cases.the_full_class_and_the_delimiter_set(lib, NAME, dict(ba=ba, select=1))
    cases.a_null_delimiter_set(lib, NAME, kw)
    cases.null_totals(lib, NAME, kw)


@WINDOWS
def test_caps_layouts_and_device_arrays(lib, ba):
    kw = dict(ba=ba)
    cases.a_cap_without_its_outputs(lib, NAME, kw)
    for missing in cases.NULL_ARRAYS:
        cases.null_device_arrays(lib, NAME, kw, missing)
    cases.missing_or_misaligned_sub_index(lib, NAME, kw)
    for layout in cases.BAD_LAYOUTS:
        cases.a_layout_that_does_not_give_nblocks(lib, NAME, kw, layout)
    for select in BOTH_SELECTS:
        cases.valid_arguments_still_need_a_context(lib, NAME, dict(ba=ba, select=select))


def test_the_select_call_keeps_its_wording(lib):
    cases.the_call_keeps_its_wording(lib, "find_records_select")


# ---- the Python keywords -------------------------------------------------------------------------------------------------
def test_the_keywords_and_their_value_errors():
    for name in ("find_records", "count_records", "grep"):
        p = inspect.signature(getattr(GpuCodec, name)).parameters
        assert p["before"].default == 0 and p["after"].default == 0 and p["context"].default is None, name
        assert p["invert"].default is False and p["line_numbers"].default is False, name
    bare = GpuCodec.__new__(GpuCodec)                       # the checks below speak before the context is looked at
    args = (None, 0, None, 0, None, 0, 4096)
    for kw in (dict(context=2, before=1), dict(context=2, after=1), dict(context=1, before=1, after=1), dict(before=-1), dict(after=-1),
               dict(context=-1), dict(before=2**32), dict(after=2**32), dict(context=2**32), dict(before=1, after=2**40)):
        with pytest.raises(ValueError):
            bare.find_records(*args, b"x", **kw)
        with pytest.raises(ValueError):
            bare.count_records(*args, b"x", **kw)
        with pytest.raises(ValueError):
            bare.grep(*args, b"x", 4, 16, **kw)
    assert GpuCodec._find_context(0, 0, None) == (0, 0) and GpuCodec._find_context(0, 0, 3) == (3, 3)
    assert GpuCodec._find_context(FAR, 0, None) == (FAR, 0) and GpuCodec._find_context(0, 0, FAR) == (FAR, FAR)
    assert GpuCodec._find_context(1, 2, None) == (1, 2) and GpuCodec._find_context(0, 0, 0) == (0, 0)
    for kw in (dict(context=2), dict(before=1), dict(after=3, invert=True), dict(context=1, line_numbers=True)):
        for bad in (b"", b"x" * 65, [], [b"a", b""], AnyOf(), AnyOf(b"x" * 32, b"y" * 33), AnyOf(b"x", b"")):
            with pytest.raises(ValueError):
                bare.find_records(*args, bad, **kw)
            with pytest.raises(ValueError):
                bare.grep(*args, bad, 4, 16, **kw)
        with pytest.raises(ValueError, match="class 1 of alternative 0 holds a delimiter"):
            bare.find_records(*args, b"a\nb", **kw)
        with pytest.raises(ValueError, match="max_len"):
            bare.grep(*args, b"x", 4, 0, **kw)
        with pytest.raises(TypeError):
            bare.find_records(*args, "text", **kw)


# ---- the model against plain Python ----------------------------------------------------------------------------------------
def py_context(data, alts, delims, blocksize, cap=0, max_len=0, served=None, invert=False, before=0, after=0):
    """the same answer from bytes.split: the indices of the selected pieces, a window of indices around each - cut where a block
    between the two pieces is not served -, their union, the pieces that are empty or of unknown extent dropped"""
    raw, n = bytes(data), len(data)
    delims = sorted(set(bytes(delims)))
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pieces = [raw] if not delims else raw.split(bytes(delims)) if len(delims) == 1 else re.split(b"[" + b"".join(re.escape(bytes([d])) for d in delims) + b"]", raw, flags=re.DOTALL)
    want = re.compile(b"|".join(b"(?:" + regex(sets) + b")" for sets in alts), re.DOTALL)
    ext, s = [], 0
    for piece in pieces if n else []:
        ext.append((s, s + len(piece)))
        s += len(piece) + 1

    def fine(lo, hi):                                       # every block with a byte of [lo, hi] is served
        return all(served[b] for b in range(lo // bs, min(hi, n - 1) // bs + 1))

    known = [s < n and e > s and fine(max(s - 1, 0), e) for s, e in ext]
    chosen = [k and ((not want.search(raw[s:e])) if invert else bool(want.search(raw[s:e]))) for k, (s, e) in zip(known, ext)]
    report = set()
    for m, (ms, me) in enumerate(ext):
        if chosen[m]:
            report.add(m)
            report |= {c for c in range(max(m - before, 0), m) if known[c] and fine(ext[c][0], me)}
            report |= {c for c in range(m + 1, min(m + after, len(ext) - 1) + 1) if known[c] and fine(ms, ext[c][1])}
    pos, lens, counts, cut, numbers, flags = [], [], [0] * nb, [], [], []
    for c in sorted(report):
        s, e = ext[c]
        pos.append(s)
        lens.append(min(e - s, clip))
        cut.append(e - s > clip)
        counts[s // bs] += 1
        numbers.append(c if all(served[:s // bs]) else NO_UNKNOWN)
        flags.append(int(chosen[c]))
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])], numbers[:written], flags[:written]


def same(data, alts, delims, blocksize, cap=0, max_len=0, served=None, invert=False, before=0, after=0):
    got = find_context_model(data, alts, delims, blocksize, cap, max_len, served, invert, before, after)
    want = py_context(data, alts, delims, blocksize, cap, max_len, served, invert, before, after)
    assert tuple(g.tolist() for g in got) == want, (bytes(data), alts, delims, blocksize, served, invert, before, after)
    sel = find_select_model(data, alts, delims, blocksize, len(data), max_len, served, invert)
    full = find_context_model(data, alts, delims, blocksize, len(data), max_len, served, invert, before, after)
    assert set(sel[0].tolist()) <= set(full[0].tolist())    # S is there in full
    assert full[0][full[5] == 1].tolist() == sel[0].tolist() and full[4][full[5] == 1].tolist() == sel[4].tolist()
    if before == after == 0:                                # the identity
        assert all(np.array_equal(g, w) for g, w in zip(full[:5], sel)) and full[5].all()
    return want


def test_the_model_by_hand():
    data = np.frombuffer(b"\nab\n\ncd ab\nxy\nzz\n\n\nq\nab", np.uint8)    # a delimiter as byte 0, two and three in a row
    alts = [[b"a", b"b"]]                                   # pieces: '', ab, '', 'cd ab', xy, zz, '', '', q, ab
    assert same(data, alts, b"\n", 4, cap=99)[0] == [1, 5, 21]
    assert same(data, alts, b"\n", 4, cap=99, after=1) == ([1, 5, 11, 21], [2, 5, 2, 2], [1, 1, 1, 0, 0, 1], [4, 4, 0, 0], [1, 3, 4, 9], [1, 1, 0, 1])
    assert same(data, alts, b"\n", 4, cap=99, before=1) == ([1, 5, 19, 21], [2, 5, 1, 2], [1, 1, 0, 0, 1, 1], [4, 4, 0, 0], [1, 3, 8, 9], [1, 1, 0, 1])
    assert same(data, alts, b"\n", 4, cap=99, after=2)[0] == [1, 5, 11, 14, 21]         # touching windows: 1 + 2 reaches 3
    assert same(data, alts, b"\n", 4, cap=99, before=3)[0] == [1, 5, 19, 21]            # three empty pieces inside the window
    assert same(data, alts, b"\n", 4, cap=99, before=4)[0] == [1, 5, 14, 19, 21]
    assert same(data, alts, b"\n", 4, cap=99, before=FAR, after=FAR)[0] == [1, 5, 11, 14, 19, 21]   # past both ends: every non-empty piece
    assert same(data, alts, b"\n", 4, cap=3, max_len=2, before=FAR, after=FAR)[3] == [6, 3, 0, 1]
    assert same(data, [[b"q"]], b"\n", 4, cap=99, invert=True, before=1)[5] == [1, 1, 1, 1, 0, 1]     # q, in front of the last piece
    assert same(data, [[b"q"]], b"\n", 4, cap=99, invert=True, after=1)[0] == [1, 5, 11, 14, 21]        # ... not behind an empty piece
    assert same(data, [[b"x"], [b"z"]], b"\n", 4, cap=99, invert=True, before=1, after=1)[0] == [1, 5, 11, 19, 21]
    assert same(data, alts, b"", 4, cap=9, before=5, after=5)[:2] == ([0], [23])        # the empty set: one record
    assert same(data, [[b"#"]], b"", 4, cap=9, before=5, after=5)[0] == []
    assert same(data, [[b"#"]], b"\n", 4, cap=9, before=FAR, after=FAR)[0] == []        # S is empty: nothing
    data = np.frombuffer(b"ab\ncd\n", np.uint8)              # a delimiter as the last byte starts no record
    assert same(data, alts, b"\n", 3, cap=9, after=5) == ([0, 3], [2, 2], [1, 1], [2, 2, 0, 0], [0, 1], [1, 0])
    # [ab\nc][d\nef][\ngh][\nab\n]: block 1 is not served - cd ends in it, ef lies in it; gh lies in block 2 behind its delimiter
    data = np.frombuffer(b"ab\ncd\nef\ngh\nab\n", np.uint8)
    for ba in DISTANCES:
        got = same(data, alts, b"\n", 4, cap=9, served=[True, False, True, True], before=ba[0], after=ba[1])
        assert got[0] == ([0, 9, 12] if ba[0] else [0, 12]), ba   # S as it was; gh on the second hit's own side; none across the block
        assert got[5] == ([1, 0, 1] if ba[0] else [1, 1])
    got = same(data, alts, b"\n", 4, cap=9, served=[True, False, True, True], before=1, after=3)
    assert got[0] == [0, 9, 12] and got[4] == [0, NO_UNKNOWN, NO_UNKNOWN] and got[5] == [1, 0, 1]   # no context across the block
    got = same(data, alts, b"\n", 4, cap=9, before=1, after=3)
    assert got[0] == [0, 3, 6, 9, 12] and got[5] == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
@pytest.mark.parametrize("ba", DISTANCES, ids=lambda ba: "%d-%d" % ba if ba[0] < FAR else "all")
def test_the_model_on_random_data(alphabet, ba):
    rng = np.random.default_rng(1000 + sum(ba) % 977 + len(alphabet))
    sizes = []
    for trial in range(12):
        data, alts, n, bs = random_case(rng, [(1,), (2, 5, 33)][trial % 2], alphabet, trial)
        if trial % 4 == 1:                                  # two and three delimiters in a row
            data[n // 3:n // 3 + 3] = 10
            data[n // 2:n // 2 + 2] = 10
        nb = (n + (bs or n) - 1) // (bs or n)
        one_bad = np.arange(nb) != int(rng.integers(0, nb))
        for served in (None, one_bad, rng.integers(0, 5, nb) != 0):
            cap = int(rng.integers(0, 50))
            for delims in (b"\n", b""):
                max_len = int(rng.integers(0, 12))
                for invert in (False, True):
                    got = same(data, alts, delims, bs, cap, max_len, served, invert, *ba)
                    sizes.append((got[3][0], sum(got[5])))
    assert any(t > s > 0 for t, s in sizes), "no trial had context"


@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
def test_one_block_not_served(alphabet):
    """S is the select model's; no reported pair spans the block; context on the hit's own side is what it is with the data
    cut at the block"""
    rng = np.random.default_rng(5 + len(alphabet))
    seen = 0
    for trial in range(30):
        data, alts, n, bs = random_case(rng, (1,), alphabet, trial)
        bs = bs or max(n // 3, 1)
        nb = (n + bs - 1) // bs
        bad = int(rng.integers(0, nb))
        served = np.arange(nb) != bad
        for before, after in ((2, 2), (0, 5), (7, 0)):
            got = find_context_model(data, alts, b"\n", bs, n, 0, served, False, before, after)
            sel = find_select_model(data, alts, b"\n", bs, n, 0, served)
            assert got[0][got[5] == 1].tolist() == sel[0].tolist()
            whole = find_context_model(data, alts, b"\n", bs, n, 0, None, False, before, after)
            assert set(got[0].tolist()) <= set(whole[0].tolist())
            for s, f in zip(got[0].tolist(), got[5].tolist()):          # a context record has a selected one on its side of the block
                if not f:
                    side = [m for m in sel[0].tolist() if (m < bad * bs) == (s < bad * bs)]
                    assert side, (trial, s)
                    seen += 1
    assert seen > 0

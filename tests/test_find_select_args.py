"""hufgpu_find_records_select: its declaration, the checks of the arguments of its own, the NumPy model of its results
(tests/find_select_model.py) and the `invert` / `line_numbers` keywords of GpuCodec (no GPU needed).  The checks it shares
with the other calls of the search family, plain and inverted, are the functions of tests/find_args_cases.py.  The model is checked
against plain Python: `re` / split over `bytes` for the records - the non-empty pieces without a match are the inverted
answer - and data[:s].count(delimiter) for the numbers.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
import find_args_support
from find_any_model import find_any_records_model
from find_args_support import HUFE_ARGUMENT, LAYOUTS, ROOT, bracket, lib, random_case, regex, valid
from find_select_model import NO_UNKNOWN, find_select_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

WHO = "find_records_select:"
AnyOf = GpuCodec.AnyOf
NAME = "find_records_select"
call = functools.partial(find_args_support.call, name=NAME)


# ---- the symbol ----------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared(lib):
    """hufgpu_find_records_any's arguments with `select` behind n_alts and `d_rec_no` behind d_rec_len: 23"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    name, sibling = "hufgpu_find_records_select", "hufgpu_find_records_any"
    assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == 23 == len(getattr(lib, sibling).argtypes) + 2
    m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 22
    s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t n_alts,", "uint32_t n_alts, uint32_t select,")
    want = want.replace("uint32_t *d_rec_len,", "uint32_t *d_rec_len, uint64_t *d_rec_no,")
    assert want == re.sub(r"\s+", " ", m.group(1))
    assert header.index(name + "(hufgpu_ctx_t") > header.index(sibling + "(hufgpu_ctx_t")
    assert re.search(r"#define\s+HUFGPU_SELECT_INVERT\s+1u", header) and _native.SELECT_INVERT == 1
    assert re.search(r"#define\s+HUFGPU_REC_NO_UNKNOWN\s+\(~\(uint64_t\)0\)", header)
    assert np.array([NO_UNKNOWN], np.int64).view(np.uint64)[0] == 2**64 - 1


# ---- the new arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", [2, 3, 4, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE])
def test_an_unknown_select_bit(lib, select):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, select=select)
        assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "needs a context" not in msg, msg
        assert "select 0x%x" % select in msg and "HUFGPU_SELECT_INVERT" in msg
    rc, msg = call(lib, select=select, cls=None, totals=None)   # ... and it is the first check of all
    assert "select 0x%x" % select in msg


@pytest.mark.parametrize("select", [0, 1])
def test_the_numbers_are_optional(lib, select):
    for kw in (dict(no=None), dict(no=None, cap=0, pos=None, rlens=None), dict(cap=0), dict(cap=0, pos=None, rlens=None), dict()):
        assert valid(*call(lib, select=select, **kw), WHO), kw
    rc, msg = call(lib, select=select, pos=None)                # the numbers stand in for neither of the two other outputs
    assert rc == HUFE_ARGUMENT and "needs d_rec_pos and d_rec_len" in msg and msg.startswith(WHO)


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
SELECTS = pytest.mark.parametrize("select", [0, 1], ids=["plain", "invert"])
BOTH_SELECTS = (dict(select=0), dict(select=1))


@SELECTS
def test_null_arrays_and_counts_of_0_and_65(lib, select):
    cases.null_arrays_and_counts_of_0_and_65(lib, NAME, dict(select=select))


@pytest.mark.parametrize("lens,at", cases.LENGTHS_OF_0)
def test_an_alternative_of_length_0(lib, lens, at):
    cases.an_alternative_of_length_0(lib, NAME, {}, lens, at)


@pytest.mark.parametrize("lens", cases.TOTALS_ABOVE_64)
def test_a_total_above_64(lib, lens):
    cases.a_total_above_64(lib, NAME, {}, lens)


@pytest.mark.parametrize("lens,j,k", cases.EMPTY_CLASSES[:8])
def test_an_empty_class(lib, lens, j, k):
    cases.an_empty_class(lib, NAME, {}, lens, j, k)


@pytest.mark.parametrize("lens,j,k", cases.DELIMITER_CLASSES[:6])
def test_a_class_that_meets_the_delimiter_set(lib, lens, j, k):
    for kw in BOTH_SELECTS:
        cases.a_class_that_meets_the_delimiter_set(lib, NAME, kw, lens, j, k)


def test_the_full_class_and_the_delimiter_set(lib):
    cases.the_full_class_and_the_delimiter_set(lib, NAME, dict(select=1))


def test_a_null_delimiter_set(lib):
    for kw in BOTH_SELECTS:
        cases.a_null_delimiter_set(lib, NAME, kw)


def test_a_cap_without_both_outputs(lib):
    cases.a_cap_without_its_outputs(lib, NAME, {})


@SELECTS
def test_valid_arguments_still_need_a_context(lib, select):
    cases.valid_arguments_still_need_a_context(lib, NAME, dict(select=select))


@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, missing):
    cases.null_device_arrays(lib, NAME, {}, missing)


def test_null_totals(lib):
    cases.null_totals(lib, NAME, {})


def test_missing_or_misaligned_sub_index(lib):
    cases.missing_or_misaligned_sub_index(lib, NAME, {})


@pytest.mark.parametrize("kw", cases.BAD_LAYOUTS)
def test_a_layout_that_does_not_give_nblocks(lib, kw):
    cases.a_layout_that_does_not_give_nblocks(lib, NAME, {}, kw)


def test_the_any_of_call_keeps_its_wording(lib):
    cases.the_call_keeps_its_wording(lib, "find_records_any")


# ---- the Python keywords -------------------------------------------------------------------------------------------------
def test_the_keywords_and_their_value_errors():
    for name in ("find_records", "count_records", "grep"):
        p = inspect.signature(getattr(GpuCodec, name)).parameters
        assert p["invert"].default is False and p["line_numbers"].default is False, name
        assert list(p)[-2:] == ["invert", "line_numbers"], name         # behind everything the methods had
    bare = GpuCodec.__new__(GpuCodec)                       # the checks below speak before the context is looked at
    args = (None, 0, None, 0, None, 0, 4096)
    for kw in (dict(invert=True), dict(line_numbers=True), dict(invert=True, line_numbers=True)):
        for bad in (b"", b"x" * 65, [], [b"a", b""], AnyOf(), AnyOf(b"x" * 32, b"y" * 33), AnyOf(b"x", b""), [b"a", 256]):
            with pytest.raises(ValueError):
                bare.find_records(*args, bad, **kw)
            with pytest.raises(ValueError):
                bare.count_records(*args, bad, **kw)
            with pytest.raises(ValueError):
                bare.grep(*args, bad, 4, 16, **kw)
        with pytest.raises(ValueError, match="class 1 of alternative 0 holds a delimiter"):
            bare.find_records(*args, b"a\nb", **kw)
        with pytest.raises(ValueError, match="class 2 of alternative 1 holds a delimiter"):
            bare.find_records(*args, AnyOf(b"x", [b"a", b"b", GpuCodec.ANY]), **kw)
        with pytest.raises(ValueError, match="class 0 of alternative 0 "):
            bare.find_records(*args, b",x", b";,", ignore_case=True, **kw)
        with pytest.raises(ValueError, match="max_len"):
            bare.grep(*args, b"x", 4, 0, **kw)
        with pytest.raises(TypeError):
            bare.find_records(*args, "text", **kw)


# ---- the model against plain Python ----------------------------------------------------------------------------------------
def py_select(data, alts, delims, blocksize, cap=0, max_len=0, served=None, invert=False):
    """the same answer from bytes.split / re.split with re.search of the alternation a piece, non-empty pieces only for the
    inverted set, and data[:s].count for the numbers"""
    raw, n = bytes(data), len(data)
    delims = sorted(set(bytes(delims)))
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pieces = [raw] if not delims else raw.split(bytes(delims)) if len(delims) == 1 else re.split(bracket(delims), raw, flags=re.DOTALL)
    want = re.compile(b"|".join(b"(?:" + regex(sets) + b")" for sets in alts), re.DOTALL)
    pos, lens, counts, cut, numbers = [], [], [0] * nb, [], []
    s = 0
    for piece in pieces if n else []:
        e = s + len(piece)
        chosen = (piece and not want.search(piece)) if invert else want.search(piece)
        if chosen and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            pos.append(s)
            lens.append(min(e - s, clip))
            cut.append(e - s > clip)
            counts[s // bs] += 1
            numbers.append(sum(raw[:s].count(bytes([d])) for d in delims) if all(served[:s // bs]) else NO_UNKNOWN)
        s = e + 1
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])], numbers[:written]


def same(data, alts, delims, blocksize, cap=0, max_len=0, served=None, invert=False):
    got = find_select_model(data, alts, delims, blocksize, cap, max_len, served, invert)
    want = py_select(data, alts, delims, blocksize, cap, max_len, served, invert)
    assert tuple(g.tolist() for g in got) == want, (bytes(data), alts, delims, blocksize, served, invert)
    if not invert:                                          # the plain answer is the any-of records' model's
        older = find_any_records_model(data, alts, delims, blocksize, cap, max_len, served)
        assert all(np.array_equal(g, w) for g, w in zip(got, older))
    return want


def test_the_model_by_hand():
    data = np.frombuffer(b"\nab\n\ncd ab\nxy", np.uint8)      # a delimiter as byte 0, two in a row, no delimiter at the end
    alts = [[b"a", b"b"]]
    assert same(data, alts, b"\n", 4, cap=9) == ([1, 5], [2, 5], [1, 1, 0, 0], [2, 2, 0, 0], [1, 3])
    assert same(data, alts, b"\n", 4, cap=9, invert=True) == ([11], [2], [0, 0, 1, 0], [1, 1, 0, 0], [4])
    assert same(data, [[b"q"]], b"\n", 4, cap=9, invert=True)[0] == [1, 5, 11]          # the empty records are absent
    assert same(data, [[b"q"]], b"\n", 4, cap=9, invert=True)[4] == [1, 3, 4]
    assert same(data, alts, b"", 4, cap=9)[:2] == ([0], [13])                          # the empty set: one record
    assert same(data, alts, b"", 4, cap=9, invert=True)[0] == []
    assert same(data, [[b"q"]], b"", 4, cap=9, invert=True)[:2] == ([0], [13])
    data = np.frombuffer(b"ab\ncd\n", np.uint8)              # a delimiter as the last byte starts no record
    assert same(data, alts, b"\n", 3, cap=9, invert=True) == ([3], [2], [0, 1], [1, 1, 0, 0], [1])
    # block 1 of [ab\nc][d\nef][\ngh] is not served: cd ends in it, ef lies in it; gh and the delimiter in front of it lie in block 2
    data = np.frombuffer(b"ab\ncd\nef\ngh", np.uint8)
    got = same(data, [[b"q"]], b"\n", 4, cap=9, invert=True, served=[True, False, True])
    assert got[0] == [0, 9] and got[4] == [0, NO_UNKNOWN]
    assert same(data, [[b"q"]], b"\n", 4, cap=9, invert=True, served=[True, True, False])[0] == [0, 3]
    got = same(data, [[b"q"]], b"\n", 4, cap=9, invert=True, served=[False, True, True])
    assert got[0] == [6, 9] and got[4] == [NO_UNKNOWN, NO_UNKNOWN]
    got = same(data, [[b"q"]], b"\n", 3, cap=9, invert=True, served=[True, True, False, True])
    assert got[0] == [0, 3] and got[4] == [0, 1]
    got = same(data, [[b"g"], [b"a"]], b"\n", 3, cap=9, served=[True, False, True, True])
    assert got[0] == [0, 9] and got[4] == [0, NO_UNKNOWN]   # the record is reported, its number is not known


MIXES = [(1,), (64,), (2, 5, 33), (32, 32)]


@pytest.mark.parametrize("mix", MIXES, ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
def test_the_model_on_random_data(mix, alphabet):
    rng = np.random.default_rng(200 * sum(mix) + len(mix) + len(alphabet))
    plain = inverted = 0
    for trial in range(10):
        data, alts, n, bs = random_case(rng, mix, alphabet, trial)
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, rng.integers(0, 5, nb) != 0):
            cap = int(rng.integers(0, 50))
            for delims in (b"\n", b"", b"\n" + bytes([int(data[n // 2])])):
                if any(set(s) & set(delims) for sets in alts for s in sets):
                    continue
                max_len = int(rng.integers(0, 12))
                plain += same(data, alts, delims, bs, cap, max_len, served)[3][0]
                inverted += same(data, alts, delims, bs, cap, max_len, served, invert=True)[3][0]
    assert inverted > 0 and (plain > 0 or mix == (64,)), "no trial had a record"


@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
def test_the_partition_and_the_drop_out(alphabet):
    """all blocks served: plain and inverted are disjoint and together every non-empty record.  One block not served: together
    every non-empty record that does not touch it - no byte of [max(s - 1, 0), min(e, n - 1)] lies in it"""
    rng = np.random.default_rng(len(alphabet))
    for trial in range(30):
        data, alts, n, bs = random_case(rng, MIXES[trial % 2 * 2], alphabet, trial)
        bs = bs or n
        nb = (n + bs - 1) // bs
        pieces, s = [], 0
        for piece in bytes(data).split(b"\n"):
            if piece:
                pieces.append((s, s + len(piece)))
            s += len(piece) + 1
        for bad in (None, int(rng.integers(0, nb))):
            served = None if bad is None else np.arange(nb) != bad
            a = find_select_model(data, alts, b"\n", bs, n, served=served)
            b = find_select_model(data, alts, b"\n", bs, n, served=served, invert=True)
            assert not set(a[0].tolist()) & set(b[0].tolist())
            both = sorted(zip(a[0].tolist() + b[0].tolist(), (a[0] + a[1]).tolist() + (b[0] + b[1]).tolist()))
            want = [(s, e) for s, e in pieces if bad is None or not max(s - 1, 0) // bs <= bad <= min(e, n - 1) // bs]
            assert both == want, (trial, bad)
            assert int(a[3][0]) + int(b[3][0]) == len(want)
            assert np.array_equal(a[2] + b[2], np.bincount(np.array([s for s, _ in want], np.int64) // bs, minlength=nb))

"""hufgpu_find_classes and hufgpu_find_records_classes: their declarations, the argument checks of their own, the NumPy models
of their results and GpuCodec.byte_classes (no GPU needed).  The checks they share with the other calls of the search family
are the functions of tests/find_args_cases.py.  The models are checked against Python's `re` on `bytes`: bracket expressions under a
look-ahead for the positions, bytes.split and re.search for the records.
"""
import functools
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
import find_args_support
from find_args_support import EMPTY, FULL, HUFE_ARGUMENT, LAYOUTS, ROOT, classes_of, lib, members, re_positions, re_records
from find_classes_model import class_table, find_class_records_model, find_classes_model
from find_model import byte_set, find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

call_pos = functools.partial(find_args_support.call, name="find_classes")
call_rec = functools.partial(find_args_support.call, name="find_records_classes")
CALLS = [(call_pos, "find_classes:"), (call_rec, "find_records_classes:")]
BOTH = pytest.mark.parametrize("call,who", CALLS, ids=["positions", "records"])
NAMES = ("find_classes", "find_records_classes")
EACH = pytest.mark.parametrize("name", NAMES, ids=["positions", "records"])


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    for name, sibling, nargs in (("hufgpu_find_classes", "hufgpu_find_pattern", 17), ("hufgpu_find_records_classes", "hufgpu_find_records", 20)):
        assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
        m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        assert m and m.group(0).count(",") == nargs - 1
        assert "*classes" in m.group(1) and "pattern_len" in m.group(1) and "*pattern" not in m.group(1)
        s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        assert re.sub(r"\s+", " ", s.group(1)).replace("*pattern", "*classes") == re.sub(r"\s+", " ", m.group(1))
        assert header.index(name + "(hufgpu_ctx_t") > header.index("hufgpu_find_records(hufgpu_ctx_t")


# ---- the classes -----------------------------------------------------------------------------------------------------------
@BOTH
def test_null_classes_and_lengths_of_0_and_65(lib, call, who):
    for kw in (dict(cls=None), dict(plen=0), dict(cls=classes_of(*[b"x"] * 65)), dict(plen=65), dict(plen=0xFFFFFFFF)):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg, (kw, msg)
    rc, msg = call(lib, cls=None)
    assert "classes and d_totals are required" in msg
    rc, msg = call(lib, plen=65, cls=classes_of(*[b"x"] * 65))
    assert "pattern_len 65" in msg
    rc, msg = call(lib, plen=0)
    assert "pattern_len 0" in msg
    for n in (1, 64):                                    # the two ends of what is allowed reach the last check
        rc, msg = call(lib, cls=classes_of(*[b"xy"] * n))
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


@BOTH
@pytest.mark.parametrize("at,n", [(0, 5), (2, 5), (4, 5), (0, 1), (63, 64), (31, 64), (32, 64)])
def test_an_empty_class(lib, call, who, at, n):
    sets = [b"ab"] * n
    sets[at] = b""
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, cls=classes_of(*sets))
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and "is empty" in msg and "needs a context" not in msg, msg
        assert f"class {at} of the pattern" in msg


@pytest.mark.parametrize("at,n", [(0, 5), (2, 5), (4, 5), (0, 1), (63, 64), (33, 64)])
def test_a_class_that_meets_the_delimiter_set(lib, at, n):
    sets = [b"ab"] * n
    sets[at] = b"a\nz"
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, cls=classes_of(*sets))
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records_classes:") and "holds a delimiter" in msg, msg
        assert "needs a context" not in msg and f"class {at} of the pattern" in msg and "(value 10)" in msg
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, cls=classes_of(*sets), delims=byte_set(b"\r\x00"))     # (no delimiter now)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
        rc, msg = call_pos(lib, nblocks=nblocks, raw_size=raw_size, cls=classes_of(*sets))       # the positions' call has no delimiters
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_rec(lib, cls=classes_of(b"a", [3, 255], b"b"), delims=byte_set([255]))
    assert rc == HUFE_ARGUMENT and "class 1 of the pattern holds a delimiter (value 255)" in msg


def test_the_full_class_and_the_delimiter_set(lib):
    for cls, at in ((b"".join([FULL, byte_set(b"a")]), 0), (b"".join([byte_set(b"a"), byte_set(b"b"), FULL]), 2)):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, cls=cls)
            assert rc == HUFE_ARGUMENT and "holds a delimiter" in msg and f"class {at} " in msg and "(value 10)" in msg
            assert "needs a context" not in msg
        rc, msg = call_rec(lib, cls=cls, delims=EMPTY)     # the empty delimiter set: valid
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
        rc, msg = call_pos(lib, cls=cls)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------

@EACH
def test_valid_arguments_still_need_a_context(lib, name):
    cases.valid_arguments_still_need_a_context(lib, name, {})


@EACH
@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, name, missing):
    cases.null_device_arrays(lib, name, {}, missing)


@EACH
def test_null_totals(lib, name):
    cases.null_totals(lib, name, {})


@EACH
def test_missing_or_misaligned_sub_index(lib, name):
    cases.missing_or_misaligned_sub_index(lib, name, {})


@EACH
@pytest.mark.parametrize("kw", cases.BAD_LAYOUTS)
def test_a_layout_that_does_not_give_nblocks(lib, name, kw):
    cases.a_layout_that_does_not_give_nblocks(lib, name, {}, kw)


def test_a_null_delimiter_set(lib):
    cases.a_null_delimiter_set(lib, NAMES[1], {})


def test_a_cap_without_both_outputs(lib):
    for name in NAMES:
        cases.a_cap_without_its_outputs(lib, name, {})


def test_the_other_calls_keep_their_wording(lib):
    for older in ("find_bytes", "find_pattern", "find_records"):
        cases.the_call_keeps_its_wording(lib, older)


# ---- byte_classes --------------------------------------------------------------------------------------------------------
def test_byte_classes_of_a_literal():
    c = GpuCodec.byte_classes(b"a\x00\xff")
    assert c.dtype == np.uint8 and c.shape == (3, 32)
    assert [members(r) for r in c] == [[97], [0], [255]]
    assert np.array_equal(GpuCodec.byte_classes(bytearray(b"a\x00\xff")), c)
    assert GpuCodec.byte_classes(b"x" * 64).shape == (64, 32)


def test_byte_classes_ignore_case():
    c = GpuCodec.byte_classes(b"aZ5@[`{\xe4\xc4", ignore_case=True)
    assert [members(r) for r in c] == [[65, 97], [90, 122], [53], [64], [91], [96], [123], [0xe4], [0xc4]]
    c = GpuCodec.byte_classes([b"ab", ord("Q"), {0x30, 0x41}], ignore_case=True)
    assert [members(r) for r in c] == [[65, 66, 97, 98], [81, 113], [0x30, 0x41, 0x61]]


def test_byte_classes_of_lists():
    c = GpuCodec.byte_classes([7, b"0123456789abcdef", {1, 2}, GpuCodec.ANY, range(250, 256), (3,)])
    assert [members(r) for r in c[:3]] == [[7], sorted(b"0123456789abcdef"), [1, 2]]
    assert members(c[3]) == list(range(256)) and members(c[4]) == list(range(250, 256)) and members(c[5]) == [3]
    assert np.array_equal(GpuCodec.byte_classes((7, b"a")), GpuCodec.byte_classes([[7], [97]]))
    assert np.array_equal(class_table(c), class_table([7, b"0123456789abcdef", {1, 2}, GpuCodec.ANY, range(250, 256), (3,)]))


def test_byte_classes_of_numpy_integers_and_other_bytes_like_objects():
    assert np.array_equal(GpuCodec.byte_classes([np.uint8(7), np.int64(200), [np.uint8(1), 2]]), GpuCodec.byte_classes([7, 200, {1, 2}]))
    for ic in (False, True):
        assert np.array_equal(GpuCodec.byte_classes(memoryview(b"aB1"), ic), GpuCodec.byte_classes(b"aB1", ic))
        assert np.array_equal(GpuCodec.byte_classes(np.frombuffer(b"aB1", np.uint8), ic), GpuCodec.byte_classes(b"aB1", ic))
    assert np.array_equal(GpuCodec.byte_classes([memoryview(b"ab")]), GpuCodec.byte_classes([b"ab"]))


def test_byte_classes_errors():
    for bad in (b"", [], b"x" * 65, [1] * 65):
        with pytest.raises(ValueError):
            GpuCodec.byte_classes(bad)
    for bad, at in (([b"", 1, 2], 0), ([1, [], 2], 1), ([1, 2, set()], 2)):
        with pytest.raises(ValueError, match=f"class {at} "):
            GpuCodec.byte_classes(bad)
    with pytest.raises(ValueError):
        GpuCodec.byte_classes([1, 256])
    with pytest.raises(TypeError):
        GpuCodec.byte_classes("text")


# ---- the models against re -----------------------------------------------------------------------------------------------


def random_sets(rng, m, alphabet, width):
    """m classes of 1 to `width` values of the alphabet"""
    return [sorted(set(int(v) for v in rng.choice(alphabet, int(rng.integers(1, width + 1))))) for _ in range(m)]


def same_positions(data, sets, blocksize, cap=0, served=None):
    got = find_classes_model(data, sets, blocksize, cap, served)
    want = re_positions(data, [sets], blocksize, cap, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def same_records(data, sets, delims, blocksize, cap=0, max_len=0, served=None):
    got = find_class_records_model(data, sets, delims, blocksize, cap, max_len, served)
    want = re_records(data, [sets], delims, blocksize, cap, max_len, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def test_models_by_hand():
    assert same_positions(np.frombuffer(b"Error eRRor errOr", np.uint8), [b"eE", b"rR", b"rR", b"oO", b"rR"], 4, cap=9)[0] == [0, 6, 12]
    assert same_positions(np.frombuffer(b"aaaa", np.uint8), [b"a", GpuCodec.ANY], 3, cap=9) == ([0, 1, 2], [3, 0], [3, 3, 0, 0])
    assert same_positions(np.frombuffer(b"aaaa", np.uint8), [GpuCodec.ANY, b"a"], 3, cap=9, served=[True, False])[0] == [0, 1]
    assert same_positions(np.frombuffer(b"a\nb", np.uint8), [b"a", GpuCodec.ANY, b"b"], 0, cap=9)[0] == [0]      # (DOTALL: any byte)
    data = np.frombuffer(b"x Err\nerr y\n\nERR", np.uint8)
    assert same_records(data, [b"eE", b"rR", b"rR"], b"\n", 4, cap=9, max_len=4) == ([0, 6, 13], [4, 4, 3], [1, 1, 0, 1], [3, 3, 0, 2])
    assert same_records(data, [b"eE", b"rR", b"rR"], b"", 4, cap=9)[:2] == ([0], [16])


@pytest.mark.parametrize("m", [1, 2, 5, 33, 64])
@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
def test_models_on_random_data(m, alphabet):
    rng = np.random.default_rng(100 * m + len(alphabet))
    values = np.array([97, 98, 99, 10]) if alphabet == "four letters" else np.arange(256)
    hits = 0
    for trial in range(12):
        n, bs = int(rng.integers(1, 700)), int(rng.integers(0, 90))
        data = (rng.choice(values, n, p=[0.32, 0.32, 0.32, 0.04]) if values.size == 4 else rng.choice(values, n)).astype(np.uint8)
        # classes wide enough for patterns of 33 and 64 positions to occur: most of the alphabet a position
        wide = trial % 2 == 0
        if alphabet == "four letters":
            narrow = rng.integers(0, max(m // 3, 1), m) == 0            # about three positions lack a letter (or are one letter)
            sets = [sorted(set(int(v) for v in rng.choice(values[:3], 1 if m <= 5 and not wide else 2, replace=False))) if narrow[k]
                    else [97, 98, 99] for k in range(m)]
        else:
            sets = [[v for v in range(256) if v != 10 and rng.integers(0, 64 if wide or m > 5 else 2)] or [1] for _ in range(m)]
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, rng.integers(0, 5, nb) != 0):
            cap = int(rng.integers(0, 50))
            hits += same_positions(data, sets, bs, cap=cap, served=served)[2][0]
            for delims in (b"\n", b"", b"\n" + bytes([int(values[-1])])):
                if any(set(s) & set(delims) for s in sets):
                    continue
                hits += same_records(data, sets, delims, bs, cap=cap, max_len=int(rng.integers(0, 12)), served=served)[3][0]
    assert hits > 0, "no trial had a match"


def test_classes_of_one_value_are_the_literal_models():
    rng = np.random.default_rng(9)
    for trial in range(40):
        n, bs = int(rng.integers(1, 400)), int(rng.integers(0, 40))
        data = rng.choice(np.array([97, 98, 10]), n).astype(np.uint8)
        pat = bytes(rng.choice(np.array([97, 98]), int(rng.integers(1, 7))).astype(np.uint8))
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 5, nb) != 0
        cap = int(rng.integers(0, 60))
        for cls in (list(pat), GpuCodec.byte_classes(pat), pat):
            got, want = find_classes_model(data, cls, bs, cap, served), find_pattern_model(data, pat, bs, cap, served)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            got = find_class_records_model(data, cls, b"\n", bs, cap, 5, served)
            want = find_records_model(data, pat, b"\n", bs, cap, 5, served)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
        got, want = find_classes_model(data, [b"ab"], bs, cap, served), find_model(data, [97, 98], bs, cap, served)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))

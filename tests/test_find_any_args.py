"""hufgpu_find_any and hufgpu_find_records_any: their declarations, the NumPy models of their results, and GpuCodec.AnyOf /
alt_classes (no GPU needed).  Their argument checks - those of every call and those of the any-of table, which the four later
calls take as well - are the functions of tests/find_args_cases.py.  The models are checked against Python's `re` on `bytes`: an
alternation of bracket expressions under a look-ahead for the positions - with the served rule applied per alternative -,
bytes.split and re.search for the records.
"""
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
from find_any_model import find_any_model, find_any_records_model
from find_args_support import ROOT, lib, members, re_positions, re_records
from find_classes_model import find_class_records_model, find_classes_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

AnyOf = GpuCodec.AnyOf
NAMES = ("find_any", "find_records_any")
EACH = pytest.mark.parametrize("name", NAMES, ids=["positions", "records"])


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(lib):
    """(classes, alt_lens, n_alts) in the place of the class calls' (classes, pattern_len), everything else theirs: one
    argument more than they have, 18 and 21"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    for name, sibling, nargs in (("hufgpu_find_any", "hufgpu_find_classes", 18), ("hufgpu_find_records_any", "hufgpu_find_records_classes", 21)):
        assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs == len(getattr(lib, sibling).argtypes) + 1
        m = re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        assert m and m.group(0).count(",") == nargs - 1
        s = re.search(r"\bint\s+" + sibling + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
        want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t pattern_len", "const uint32_t *alt_lens, uint32_t n_alts")
        assert want == re.sub(r"\s+", " ", m.group(1))
        assert header.index(name + "(hufgpu_ctx_t") > header.index("hufgpu_find_records_classes(hufgpu_ctx_t")


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
@EACH
def test_null_arrays_and_counts_of_0_and_65(lib, name):
    cases.null_arrays_and_counts_of_0_and_65(lib, name, {})


@EACH
@pytest.mark.parametrize("lens,at", cases.LENGTHS_OF_0)
def test_an_alternative_of_length_0(lib, name, lens, at):
    cases.an_alternative_of_length_0(lib, name, {}, lens, at)


@EACH
@pytest.mark.parametrize("lens", cases.TOTALS_ABOVE_64)
def test_a_total_above_64(lib, name, lens):
    cases.a_total_above_64(lib, name, {}, lens)


@EACH
@pytest.mark.parametrize("lens,j,k", cases.EMPTY_CLASSES[:8])
def test_an_empty_class(lib, name, lens, j, k):
    cases.an_empty_class(lib, name, {}, lens, j, k)


@pytest.mark.parametrize("lens,j,k", cases.DELIMITER_CLASSES[:6])
def test_a_class_that_meets_the_delimiter_set(lib, lens, j, k):
    for name in NAMES:                                      # (the positions' call has no delimiters)
        cases.a_class_that_meets_the_delimiter_set(lib, name, {}, lens, j, k)


def test_the_full_class_and_the_delimiter_set(lib):
    for name in NAMES:
        cases.the_full_class_and_the_delimiter_set(lib, name, {})


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
    for older in ("find_bytes", "find_classes", "find_records_classes"):
        cases.the_call_keeps_its_wording(lib, older)


# ---- AnyOf and alt_classes -----------------------------------------------------------------------------------------------
def test_alt_classes():
    a = AnyOf(b"ERROR", [b"fF", ord("x"), {1, 2}], b"p")
    assert len(a) == 3 and list(a) == [b"ERROR", [b"fF", ord("x"), {1, 2}], b"p"] and "AnyOf(" in repr(a)
    classes, lens = GpuCodec.alt_classes(a)
    assert classes.dtype == np.uint8 and classes.shape == (9, 32) and lens.dtype == np.uint32 and lens.tolist() == [5, 3, 1]
    assert np.array_equal(classes[:5], GpuCodec.byte_classes(b"ERROR"))
    assert [members(r) for r in classes[5:]] == [[70, 102], [120], [1, 2], [112]]
    classes, lens = GpuCodec.alt_classes(AnyOf(b"ab", [b"c", GpuCodec.ANY]), ignore_case=True)
    assert lens.tolist() == [2, 2]
    assert [members(r) for r in classes[:3]] == [[65, 97], [66, 98], [67, 99]] and members(classes[3]) == list(range(256))
    for mix in ((1,), (64,), (1,) * 64, (2, 5, 33), (31, 33), (32, 32), (1, 63)):
        classes, lens = GpuCodec.alt_classes(AnyOf(*[b"x" * m for m in mix]))
        assert classes.shape == (sum(mix), 32) and lens.tolist() == list(mix)
    one = GpuCodec.alt_classes(AnyOf(b"needle"), ignore_case=True)
    assert np.array_equal(one[0], GpuCodec.byte_classes(b"needle", ignore_case=True)) and one[1].tolist() == [6]


def test_alt_classes_errors():
    for bad in (AnyOf(), AnyOf(*[b"x"] * 65), AnyOf(b"x" * 64, b"y"), AnyOf(b"x" * 32, b"y" * 33), AnyOf(b"x" * 65)):
        with pytest.raises(ValueError):
            GpuCodec.alt_classes(bad)
    with pytest.raises(ValueError, match="sum to 65"):
        GpuCodec.alt_classes(AnyOf(b"x" * 32, b"y" * 33))
    for bad, at in ((AnyOf(b"", b"a"), 0), (AnyOf(b"a", []), 1), (AnyOf(b"a", b"b", b""), 2)):
        with pytest.raises(ValueError, match=f"alternative {at} has length 0"):
            GpuCodec.alt_classes(bad)
    with pytest.raises(ValueError, match="alternative 1: class 2 "):
        GpuCodec.alt_classes(AnyOf(b"a", [1, 2, b""]))
    with pytest.raises(ValueError):
        GpuCodec.alt_classes(AnyOf(b"a", [1, 256]))
    with pytest.raises(TypeError):
        GpuCodec.alt_classes(AnyOf(b"a", "text"))
    with pytest.raises(TypeError):
        GpuCodec.alt_classes([b"a", b"b"])


# ---- the models against re -----------------------------------------------------------------------------------------------
def same_positions(data, alts, blocksize, cap=0, served=None):
    got = find_any_model(data, alts, blocksize, cap, served)
    want = re_positions(data, alts, blocksize, cap, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def same_records(data, alts, delims, blocksize, cap=0, max_len=0, served=None):
    got = find_any_records_model(data, alts, delims, blocksize, cap, max_len, served)
    want = re_records(data, alts, delims, blocksize, cap, max_len, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def test_models_by_hand():
    data = np.frombuffer(b"ab abc cab", np.uint8)
    assert same_positions(data, [[b"a", b"b"], [b"a", b"b", b"c"]], 4, cap=9) == ([0, 3, 8], [2, 0, 1], [3, 3, 0, 0])      # the same start: once
    # the long alternative reaches block 1, which is not served, the short one does not: the start stays; both reach it: dropped
    assert same_positions(np.frombuffer(b"abcxxx", np.uint8), [[b"a", b"b"], [b"a", b"b", b"c", b"x"]], 3, cap=9, served=[True, False])[0] == [0]
    assert same_positions(np.frombuffer(b"xabcxx", np.uint8), [[b"a", b"b"], [b"a", b"b", b"c"]], 3, cap=9, served=[True, False])[0] == [1]
    assert same_positions(np.frombuffer(b"xxabcx", np.uint8), [[b"a", b"b"], [b"a", b"b", b"c"]], 3, cap=9, served=[True, False])[0] == []
    assert same_positions(np.frombuffer(b"ad cb bc abcd", np.uint8), [[b"a", b"b"], [b"c", b"d"]], 5, cap=9)[0] == [9, 11]      # no cross-talk
    data = np.frombuffer(b"x Err and fatal\nerr y\n\nfatal\nnone", np.uint8)
    alts = [[b"eE", b"rR", b"rR"], [b"f", b"a", b"t", b"a", b"l"]]
    assert same_records(data, alts, b"\n", 8, cap=9, max_len=6) == ([0, 16, 23], [6, 5, 5], [1, 0, 2, 0, 0], [3, 3, 0, 1])
    assert same_records(data, alts, b"", 8, cap=9)[:2] == ([0], [33])


MIXES = [(1,), (64,), (1,) * 64, (2, 5, 33), (31, 33), (32, 32), (1, 63)]


@pytest.mark.parametrize("mix", MIXES, ids=lambda m: "x".join(map(str, m)) if len(m) < 9 else "1x64")
@pytest.mark.parametrize("alphabet", ["four letters", "all values"])
def test_models_on_random_data(mix, alphabet):
    rng = np.random.default_rng(100 * sum(mix) + len(mix) + len(alphabet))
    values = np.array([97, 98, 99, 10]) if alphabet == "four letters" else np.arange(256)
    hits = 0
    for trial in range(10):
        n, bs = int(rng.integers(1, 700)), int(rng.integers(0, 90))
        data = (rng.choice(values, n, p=[0.32, 0.32, 0.32, 0.04]) if values.size == 4 else rng.choice(values, n)).astype(np.uint8)
        alts = []
        for m in mix:
            # classes wide enough for alternatives of 31 to 64 positions to occur: most of the alphabet a position
            wide = trial % 2 == 0
            if alphabet == "four letters":
                if len(mix) == 64:                          # 64 alternatives of one position: one or two letters each
                    sets = [sorted(set(int(v) for v in rng.choice(values[:3], int(rng.integers(1, 3)), replace=False)))]
                else:
                    narrow = rng.integers(0, max(m // 3, 1), m) == 0
                    sets = [sorted(set(int(v) for v in rng.choice(values[:3], 1 if m <= 5 and not wide else 2, replace=False))) if narrow[k]
                            else [97, 98, 99] for k in range(m)]
            else:
                sets = [[v for v in range(256) if v != 10 and rng.integers(0, 64 if wide or m > 5 else 2)] or [1] for _ in range(m)]
            alts.append(sets)
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, rng.integers(0, 5, nb) != 0):
            cap = int(rng.integers(0, 50))
            hits += same_positions(data, alts, bs, cap=cap, served=served)[2][0]
            for delims in (b"\n", b"", b"\n" + bytes([int(values[-1])])):
                if any(set(s) & set(delims) for sets in alts for s in sets):
                    continue
                hits += same_records(data, alts, delims, bs, cap=cap, max_len=int(rng.integers(0, 12)), served=served)[3][0]
    assert hits > 0, "no trial had a match"


def test_models_of_one_alternative_are_the_class_models():
    rng = np.random.default_rng(19)
    for trial in range(40):
        n, bs = int(rng.integers(1, 400)), int(rng.integers(0, 40))
        data = rng.choice(np.array([97, 98, 10]), n).astype(np.uint8)
        m = int(rng.integers(1, 7))
        sets = [sorted(set(int(v) for v in rng.choice(np.array([97, 98]), int(rng.integers(1, 3))))) for _ in range(m)]
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 5, nb) != 0
        cap = int(rng.integers(0, 60))
        for alts in ([sets], [GpuCodec.byte_classes(sets)], [sets, sets]):
            got, want = find_any_model(data, alts, bs, cap, served), find_classes_model(data, sets, bs, cap, served)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            got = find_any_records_model(data, alts, b"\n", bs, cap, 5, served)
            want = find_class_records_model(data, sets, b"\n", bs, cap, 5, served)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))

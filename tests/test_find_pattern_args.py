"""hufgpu_find_pattern: its declaration, the argument check of its own and the NumPy model of its result (no GPU needed).  The
checks it shares with the other calls of the search family are the functions of tests/find_args_cases.py.  The model is checked
against a plain bytes.find loop.
"""
import functools
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
import find_args_support
from find_args_support import HUFE_ARGUMENT, LAYOUTS, ROOT, lib
from find_model import find_model
from find_pattern_model import find_pattern_model
from libhuffman_amd import _native

NAME = "find_pattern"
call = functools.partial(find_args_support.call, name=NAME)


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_find_pattern" in _native.GPU_SYMBOLS
    assert hasattr(lib, "hufgpu_find_pattern")
    assert len(lib.hufgpu_find_pattern.argtypes) == 17
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    m = re.search(r"\bint\s+hufgpu_find_pattern\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 16
    m = re.search(r"#define\s+HUFGPU_FIND_PATTERN_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == 64 == _native.FIND_PATTERN_MAX


def test_a_pattern_of_no_or_too_many_bytes(lib):
    for kw in (dict(pattern=None), dict(plen=0), dict(pattern=b"x" * 65), dict(plen=65), dict(plen=0xFFFFFFFF)):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_pattern:") and "needs a context" not in msg, (kw, msg)
    rc, msg = call(lib, pattern=None)
    assert "pattern and d_totals are required" in msg
    rc, msg = call(lib, plen=65)
    assert "pattern_len 65" in msg
    for pat in (b"x", b"x" * 64):                        # the two ends of what is allowed reach the last check
        rc, msg = call(lib, pattern=pat)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
def test_valid_arguments_still_need_a_context(lib):
    cases.valid_arguments_still_need_a_context(lib, NAME, {})


@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, missing):
    cases.null_device_arrays(lib, NAME, {}, missing)


def test_null_totals(lib):
    cases.null_totals(lib, NAME, {})


def test_a_cap_without_positions(lib):
    cases.a_cap_without_its_outputs(lib, NAME, {})


def test_missing_or_misaligned_sub_index(lib):
    cases.missing_or_misaligned_sub_index(lib, NAME, {})


@pytest.mark.parametrize("kw", cases.BAD_LAYOUTS)
def test_a_layout_that_does_not_give_nblocks(lib, kw):
    cases.a_layout_that_does_not_give_nblocks(lib, NAME, {}, kw)


def test_find_bytes_keeps_its_wording(lib):
    cases.the_call_keeps_its_wording(lib, "find_bytes")


# ---- the model -----------------------------------------------------------------------------------------------------------
def plain(data, pattern, blocksize, cap=0, served=None):
    """the same answer from bytes.find, one start at a time"""
    raw, n, m = bytes(data), len(data), len(pattern)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    pos, counts = [], [0] * nb
    p = raw.find(pattern)
    while p >= 0:
        if all(served[b] for b in range(p // bs, (p + m - 1) // bs + 1)):
            pos.append(p)
            counts[p // bs] += 1
        p = raw.find(pattern, p + 1)
    written = min(len(pos), cap)
    return pos[:written], counts, [len(pos), written, nb - sum(served), 0]


def same(data, pattern, blocksize, cap=0, served=None):
    data = np.frombuffer(bytes(data), np.uint8)
    pos, counts, totals = find_pattern_model(data, pattern, blocksize, cap, served)
    want = plain(data, pattern, blocksize, cap, served)
    assert (pos.tolist(), counts.tolist(), totals.tolist()) == (want[0], want[1], want[2])
    return want


def test_model_overlapping_matches():
    assert same(b"aaaa", b"aa", 0, cap=10) == ([0, 1, 2], [3], [3, 3, 0, 0])
    assert same(b"aaaa", b"aa", 3, cap=2) == ([0, 1], [3, 0], [3, 2, 0, 0])          # the start at 2 ends in block 1
    assert same(b"abababa", b"aba", 2, cap=10)[0] == [0, 2, 4]
    assert same(b"aaaa", b"aaaaa", 0, cap=10) == ([], [0], [0, 0, 0, 0])


def test_model_a_match_across_a_block_seam():
    data = b"..ERR" + b"OR..." + b"....."
    assert same(data, b"ERROR", 5, cap=10) == ([2], [1, 0, 0], [1, 1, 0, 0])
    assert same(b"xERRORx" * 3, b"ERROR", 3, cap=10)[0] == [1, 8, 15]               # every match spans blocks


def test_model_a_match_across_a_block_that_is_not_served():
    data = b"ab" * 6                                       # blocks of 4: "abab" x 3
    assert same(data, b"ab", 4, cap=10)[0] == [0, 2, 4, 6, 8, 10]
    assert same(data, b"ab", 4, cap=10, served=[True, False, True]) == ([0, 2, 8, 10], [2, 0, 2], [4, 4, 1, 0])
    # "ba" at 3 starts in block 0 and ends in block 1, "ba" at 7 starts in block 1: both go with block 1
    assert same(data, b"ba", 4, cap=10, served=[True, False, True]) == ([1, 9], [1, 0, 1], [2, 2, 1, 0])
    # nine bytes touch three blocks: any of them not served drops the match
    assert same(data, b"babababab", 4, cap=10, served=[True, False, True])[0] == []
    assert same(data, b"babababab", 4, cap=10)[0] == [1, 3]
    for served in ([False, True, True], [True, True, False]):
        assert same(data, b"babababab", 4, cap=10, served=served)[0] == []


def test_model_a_match_that_would_end_past_the_data():
    assert same(b"....ERRO", b"ERROR", 3, cap=10) == ([], [0, 0, 0], [0, 0, 0, 0])
    assert same(b"...ERROR", b"ERROR", 3, cap=10) == ([3], [0, 1, 0], [1, 1, 0, 0])
    assert same(b"", b"a", 3, cap=10) == ([], [], [0, 0, 0, 0])


def test_model_one_byte_is_find_model():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 4, 1000).astype(np.uint8)
    served = rng.integers(0, 4, 1000 // 7 + 1) != 0
    for cap in (0, 5, 2000):
        for sv in (None, served):
            got, want = find_pattern_model(data, bytes([2]), 7, cap, sv), find_model(data, [2], 7, cap, sv)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_model_random_inputs():
    rng = np.random.default_rng(4)
    for _ in range(50):
        n, bs = int(rng.integers(1, 200)), int(rng.integers(0, 9))
        data = rng.integers(0, 2, n).astype(np.uint8)
        nb = (n + (bs or n) - 1) // (bs or n)
        pattern = bytes(rng.integers(0, 2, int(rng.integers(1, 12))).astype(np.uint8))
        same(data, pattern, bs, cap=int(rng.integers(0, 50)), served=rng.integers(0, 5, nb) != 0)

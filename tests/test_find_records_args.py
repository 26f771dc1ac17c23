"""hufgpu_find_records: its declaration, the argument checks of its own and the NumPy model of its result (no GPU needed).  The
checks it shares with the other calls of the search family are the functions of tests/find_args_cases.py.  The model is checked
against a plain loop over `bytes`: split at the delimiters, `in` for the pattern.
"""
import functools
import os
import re

import numpy as np
import pytest

import find_args_cases as cases
import find_args_support
from find_args_support import HUFE_ARGUMENT, LAYOUTS, ROOT, lib
from find_model import byte_set
from find_records_model import find_records_model
from libhuffman_amd import _native

NAME = "find_records"
call = functools.partial(find_args_support.call, name=NAME)


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_find_records" in _native.GPU_SYMBOLS
    assert hasattr(lib, "hufgpu_find_records")
    assert len(lib.hufgpu_find_records.argtypes) == 20
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    m = re.search(r"\bint\s+hufgpu_find_records\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 19
    for name in ("delim_set[32]", "*pattern", "pattern_len", "*d_rec_pos", "*d_rec_len", "rec_cap", "max_len", "*d_block_counts",
                 "*d_totals", "*d_block_errs"):
        assert name in m.group(1), name
    assert header.index("hufgpu_find_records(hufgpu_ctx_t") > header.index("hufgpu_find_pattern(hufgpu_ctx_t")


def test_a_pattern_of_no_or_too_many_bytes(lib):
    for kw in (dict(pattern=None), dict(plen=0), dict(pattern=b"x" * 65), dict(plen=65), dict(plen=0xFFFFFFFF)):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "needs a context" not in msg, (kw, msg)
    rc, msg = call(lib, pattern=None)
    assert "pattern and d_totals are required" in msg
    rc, msg = call(lib, plen=65)
    assert "pattern_len 65" in msg
    for pat in (b"x", b"x" * 64):                        # the two ends of what is allowed reach the last check
        rc, msg = call(lib, pattern=pat)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


@pytest.mark.parametrize("pat", [b"\nRROR", b"ER\nOR", b"ERRO\n", b"\n", b"x" * 63 + b"\n"])
def test_a_pattern_that_holds_a_delimiter(lib, pat):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, pattern=pat)
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "is a delimiter" in msg, msg
        assert "needs a context" not in msg
        assert f"byte {pat.index(10)} of the pattern" in msg
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, pattern=pat, delims=byte_set(b"\r\x00"))     # (no delimiter now)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, pattern=b"a\xffb", delims=byte_set([255]))
    assert rc == HUFE_ARGUMENT and "byte 1 of the pattern (value 255)" in msg


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
def test_valid_arguments_still_need_a_context(lib):
    cases.valid_arguments_still_need_a_context(lib, NAME, {})


@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, missing):
    cases.null_device_arrays(lib, NAME, {}, missing)


def test_null_totals(lib):
    cases.null_totals(lib, NAME, {})


def test_a_null_delimiter_set(lib):
    cases.a_null_delimiter_set(lib, NAME, {})


def test_a_cap_without_both_outputs(lib):
    cases.a_cap_without_its_outputs(lib, NAME, {})


def test_missing_or_misaligned_sub_index(lib):
    cases.missing_or_misaligned_sub_index(lib, NAME, {})


@pytest.mark.parametrize("kw", cases.BAD_LAYOUTS)
def test_a_layout_that_does_not_give_nblocks(lib, kw):
    cases.a_layout_that_does_not_give_nblocks(lib, NAME, {}, kw)


def test_the_other_calls_keep_their_wording(lib):
    for older in ("find_bytes", "find_pattern"):
        cases.the_call_keeps_its_wording(lib, older)


# ---- the model -----------------------------------------------------------------------------------------------------------
def plain(data, pattern, delims, blocksize, cap=0, max_len=0, served=None):
    """the same answer from a walk over `bytes`, one record at a time"""
    raw, n = bytes(data), len(data)
    delims = set(bytes(delims))
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pos, lens, counts, cut = [], [], [0] * nb, []
    s = 0
    while s <= n and n:
        e = s
        while e < n and raw[e] not in delims:
            e += 1
        if raw[s:e].find(pattern) >= 0 and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            pos.append(s)
            lens.append(min(e - s, clip))
            cut.append(e - s > clip)
            counts[s // bs] += 1
        s = e + 1
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])]


def same(data, pattern, delims, blocksize, cap=0, max_len=0, served=None):
    data = np.frombuffer(bytes(data), np.uint8)
    got = find_records_model(data, pattern, delims, blocksize, cap, max_len, served)
    want = plain(data, pattern, delims, blocksize, cap, max_len, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def test_model_records_and_their_ends():
    assert same(b"ab\ncab\n\nab", b"ab", b"\n", 0, cap=9) == ([0, 3, 8], [2, 3, 2], [3], [3, 3, 0, 0])
    assert same(b"ab\ncab\n\nab\n", b"ab", b"\n", 0, cap=9) == ([0, 3, 8], [2, 3, 2], [3], [3, 3, 0, 0])
    assert same(b"\n\nab", b"ab", b"\n", 0, cap=9)[:2] == ([2], [2])
    assert same(b"xx\nyy", b"ab", b"\n", 0, cap=9) == ([], [], [0], [0, 0, 0, 0])
    assert same(b"", b"ab", b"\n", 0, cap=9) == ([], [], [], [0, 0, 0, 0])
    assert same(b"a,b;ab,", b"b", b",;", 0, cap=9)[:2] == ([2, 4], [1, 2])


def test_model_a_record_with_many_matches_is_one_entry():
    assert same(b"ababab\nabab", b"abab", b"\n", 0, cap=9) == ([0, 7], [6, 4], [2], [2, 2, 0, 0])
    assert same(b"aaaa", b"a", b"", 3, cap=9) == ([0], [4], [1, 0], [1, 1, 0, 0])          # no delimiter: one record
    assert same(b"aaaa", b"a", b"z", 3, cap=9) == ([0], [4], [1, 0], [1, 1, 0, 0])


def test_model_caps():
    data = b"ab\nabcdef\nab\nxx\nabc"
    assert same(data, b"ab", b"\n", 4, cap=9, max_len=3) == ([0, 3, 10, 16], [2, 3, 2, 3], [2, 0, 1, 0, 1], [4, 4, 0, 1])
    assert same(data, b"ab", b"\n", 4, cap=1, max_len=3)[3] == [4, 1, 0, 0]                   # the cut record is not written
    assert same(data, b"ab", b"\n", 4, cap=2, max_len=2)[3] == [4, 2, 0, 1]
    assert same(data, b"ab", b"\n", 4, cap=0, max_len=1)[3] == [4, 0, 0, 0]
    assert same(data, b"ab", b"\n", 4, cap=9, max_len=6)[1] == [2, 6, 2, 3]


def test_model_blocks_that_are_not_served():
    data = b"ab\nab\nab\nab"                                # blocks of 3: "ab\n" x 3 + "ab"
    assert same(data, b"ab", b"\n", 3, cap=9)[0] == [0, 3, 6, 9]
    # block 1 holds the record at 3, the delimiter that ends it - and the delimiter in front of the record at 6
    assert same(data, b"ab", b"\n", 3, cap=9, served=[True, False, True, True]) == ([0, 9], [2, 2], [1, 0, 0, 1], [2, 2, 1, 0])
    # ... block 0 the delimiter in front of the record at 3
    assert same(data, b"ab", b"\n", 3, cap=9, served=[False, True, True, True])[0] == [6, 9]
    assert same(data, b"ab", b"\n", 3, cap=9, served=[True, True, True, False])[0] == [0, 3, 6]
    # a record over three blocks needs all of them, and the one behind with its end
    data = b"x\nab......\nx"
    assert same(data, b"ab", b"\n", 4, cap=9)[0] == [2]
    for k in range(3):
        assert same(data, b"ab", b"\n", 4, cap=9, served=[j != k for j in range(3)])[0] == []
    data = b"ab..\n..."                                     # the delimiter that ends the record opens block 1
    assert same(data, b"ab", b"\n", 4, cap=9, served=[True, False])[0] == []
    assert same(b"ab...\n..", b"ab", b"\n", 4, cap=9, served=[True, False])[0] == []
    assert same(b"ab.\n....", b"ab", b"\n", 4, cap=9, served=[True, False])[0] == [0]
    assert same(b"ab..", b"ab", b"\n", 2, cap=9, served=[True, False])[0] == []               # raw_size ends it, behind block 1


def test_model_random_log_like_inputs():
    rng = np.random.default_rng(5)
    words = [b"ERROR", b"INFO", b"warn", b"ERR", b"OR", b" ", b"12", b"E", b"R"]
    for _ in range(60):
        lines = [b"".join(words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(0, 6)))) for _ in range(int(rng.integers(1, 30)))]
        data = b"\n".join(lines) + (b"\n" if rng.integers(0, 2) else b"")
        if not data:
            continue
        bs = int(rng.integers(0, 40))
        nb = (len(data) + (bs or len(data)) - 1) // (bs or len(data))
        pattern = [b"ERROR", b"RO", b"E", b"ERRORERR", b"zz"][int(rng.integers(0, 5))]
        for served in (None, rng.integers(0, 6, nb) != 0):
            same(data, pattern, b"\n " if rng.integers(0, 3) == 0 else b"\n", bs, cap=int(rng.integers(0, 40)),
                 max_len=int(rng.integers(0, 12)), served=served)

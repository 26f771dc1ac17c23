"""hufgpu_find_records: the symbol, its declaration, its argument checks and the NumPy model of its result (no GPU needed).

As for hufgpu_find_pattern (tests/test_find_pattern_args.py, whose cases are repeated here with the `find_records:`
wording) argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked
with a NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.  The
model is checked against a plain loop over `bytes`: split at the delimiters, `in` for the pattern.
"""
import os
import re

import numpy as np
import pytest

from find_model import byte_set
from find_records_model import find_records_model
from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM, INDEX, SUB, POS, LEN, COUNTS, TOTALS, ERRS = 0x10000, 0x20000, 0x30008, 0x40000, 0x48000, 0x50000, 0x60000, 0x70000
PAT = b"ERROR"
NEWLINE = byte_set(b"\n")
DEFAULT = object()


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, delims=NEWLINE,
         pat=PAT, plen=DEFAULT, pos=POS, lens=LEN, cap=16, max_len=128, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    if plen is DEFAULT:
        plen = len(pat) if pat is not None else 5
    rc = lib.hufgpu_find_records(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, delims, pat, plen, pos, lens,
                                 cap, max_len, counts, totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


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
    for kw in (dict(pat=None), dict(plen=0), dict(pat=b"x" * 65), dict(plen=65), dict(plen=0xFFFFFFFF)):
        for nblocks, raw_size in ((4, 4 * 4096), (0, 0)):
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "needs a context" not in msg, (kw, msg)
    rc, msg = call(lib, pat=None)
    assert "pattern and d_totals are required" in msg
    rc, msg = call(lib, plen=65)
    assert "pattern_len 65" in msg
    for pat in (b"x", b"x" * 64):                        # the two ends of what is allowed reach the last check
        rc, msg = call(lib, pat=pat)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


# ---- the new cases -----------------------------------------------------------------------------------------------------
def test_a_null_delimiter_set(lib):
    for nblocks, raw_size in ((4, 4 * 4096), (0, 0)):
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, delims=None)
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "delim_set is required" in msg, msg
        assert "needs a context" not in msg
    rc, msg = call(lib, delims=bytes(32))                # the empty set is valid
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, delims=byte_set(range(256)), pat=None)
    assert "pattern and d_totals are required" in msg


@pytest.mark.parametrize("pat", [b"\nRROR", b"ER\nOR", b"ERRO\n", b"\n", b"x" * 63 + b"\n"])
def test_a_pattern_that_holds_a_delimiter(lib, pat):
    for nblocks, raw_size in ((4, 4 * 4096), (0, 0)):
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, pat=pat)
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "is a delimiter" in msg, msg
        assert "needs a context" not in msg
        assert f"byte {pat.index(10)} of the pattern" in msg
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, pat=pat, delims=byte_set(b"\r\x00"))     # (no delimiter now)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, pat=b"a\xffb", delims=byte_set([255]))
    assert rc == HUFE_ARGUMENT and "byte 1 of the pattern (value 255)" in msg


def test_a_cap_without_both_outputs(lib):
    for kw in (dict(pos=None), dict(lens=None), dict(pos=None, lens=None)):
        for cap in (1, 16):
            rc, msg = call(lib, cap=cap, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_records:") and "needs d_rec_pos and d_rec_len" in msg, (kw, msg)
            assert f"rec_cap {cap}" in msg and "needs a context" not in msg
        rc, msg = call(lib, cap=0, **kw)                 # with rec_cap = 0 both may be NULL
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


# ---- the cases of tests/test_find_pattern_args.py ------------------------------------------------------------------------
def test_valid_arguments_still_need_a_context(lib):
    rc, msg = call(lib)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith("find_records:")
    rc, msg = call(lib, pos=None, lens=None, cap=0, counts=None)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, max_len=0)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, blocksize=0, nblocks=1)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    # nblocks = 0 is success only with a context to enqueue the zeroing of d_totals on
    rc, msg = call(lib, stream=None, index=None, sub=None, errs=None, nblocks=0, raw_size=0)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


@pytest.mark.parametrize("missing", ["stream", "index", "errs"])
def test_null_device_arrays(lib, missing):
    rc, msg = call(lib, **{missing: None})
    assert rc == HUFE_ARGUMENT and "are required" in msg and "needs a context" not in msg and msg.startswith("find_records:")


def test_null_totals(lib):
    for nblocks, raw_size in ((4, 4 * 4096), (0, 0)):
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, totals=None)
        assert rc == HUFE_ARGUMENT and "pattern and d_totals are required" in msg and msg.startswith("find_records:")


def test_missing_or_misaligned_sub_index(lib):
    for sub in (None, 0x30004, 0x30001):
        rc, msg = call(lib, sub=sub)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg and msg.startswith("find_records:")


@pytest.mark.parametrize("kw", [
    dict(raw_size=5 * 4096),                            # five blocks
    dict(raw_size=3 * 4096),                            # three
    dict(raw_size=0),
    dict(blocksize=0),                                  # one block
    dict(nblocks=0),                                    # no blocks, but bytes
    dict(blocksize=(1 << 38) + 1, raw_size=4 * ((1 << 38) + 1)),
])
def test_a_layout_that_does_not_give_nblocks(lib, kw):
    rc, msg = call(lib, **kw)
    assert rc == HUFE_ARGUMENT and "must be those of the encode" in msg and msg.startswith("find_records:")


def test_the_other_calls_keep_their_wording(lib):
    rc = lib.hufgpu_find_bytes(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, None, POS, 16, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode() == "find_bytes: the set and d_totals are required"
    rc = lib.hufgpu_find_pattern(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, b"a\nb", 3, None, 1, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode() == "find_pattern: pos_cap 1 needs d_pos"


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

"""hufgpu_find_classes and hufgpu_find_records_classes: the symbols, their declarations, their argument checks, the NumPy
models of their results and GpuCodec.byte_classes (no GPU needed).

As for the literal calls (tests/test_find_pattern_args.py and tests/test_find_records_args.py, whose cases are repeated
here with the `find_classes:` / `find_records_classes:` wording) argument errors are found before anything is enqueued and
before the context is looked at, so they can be provoked with a NULL context and made-up device pointers (never
dereferenced); hufgpu_last_error(NULL) says which check spoke.  The models are checked against Python's `re` on `bytes`:
bracket expressions under a look-ahead for the positions, bytes.split and re.search for the records.
"""
import os
import re

import numpy as np
import pytest

from find_classes_model import class_table, find_class_records_model, find_classes_model
from find_model import byte_set, find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM, INDEX, SUB, POS, LEN, COUNTS, TOTALS, ERRS = 0x10000, 0x20000, 0x30008, 0x40000, 0x48000, 0x50000, 0x60000, 0x70000
NEWLINE = byte_set(b"\n")
FULL, EMPTY = bytes([255] * 32), bytes(32)
DEFAULT = object()


def classes_of(*sets):
    """the C array: 32 bytes a class"""
    return b"".join(byte_set(s) for s in sets)


CLS = classes_of(b"eE", b"rR", b"rR", b"oO", b"rR")


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call_pos(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, cls=CLS,
             plen=DEFAULT, pos=POS, cap=16, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    if plen is DEFAULT:
        plen = len(cls) // 32 if cls is not None else 5
    rc = lib.hufgpu_find_classes(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, cls, plen, pos, cap, counts,
                                 totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


def call_rec(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, delims=NEWLINE,
             cls=CLS, plen=DEFAULT, pos=POS, lens=LEN, cap=16, max_len=128, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    if plen is DEFAULT:
        plen = len(cls) // 32 if cls is not None else 5
    rc = lib.hufgpu_find_records_classes(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, delims, cls, plen, pos,
                                         lens, cap, max_len, counts, totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


CALLS = [(call_pos, "find_classes:"), (call_rec, "find_records_classes:")]
BOTH = pytest.mark.parametrize("call,who", CALLS, ids=["positions", "records"])
LAYOUTS = ((4, 4 * 4096), (0, 0))


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


# ---- the new cases -------------------------------------------------------------------------------------------------------
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


def test_a_null_delimiter_set(lib):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, delims=None)
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records_classes:") and "delim_set is required" in msg, msg
        assert "needs a context" not in msg
    rc, msg = call_rec(lib, delims=EMPTY)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_rec(lib, delims=byte_set(range(256)), cls=None)
    assert "classes and d_totals are required" in msg


def test_a_cap_without_both_outputs(lib):
    for kw in (dict(pos=None), dict(lens=None), dict(pos=None, lens=None)):
        for cap in (1, 16):
            rc, msg = call_rec(lib, cap=cap, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_records_classes:") and "needs d_rec_pos and d_rec_len" in msg, (kw, msg)
            assert f"rec_cap {cap}" in msg and "needs a context" not in msg
        rc, msg = call_rec(lib, cap=0, **kw)             # with rec_cap = 0 both may be NULL
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_pos(lib, pos=None, cap=1)
    assert rc == HUFE_ARGUMENT and "needs d_pos" in msg and msg.startswith("find_classes:")


# ---- the cases of the literal calls --------------------------------------------------------------------------------------
@BOTH
def test_valid_arguments_still_need_a_context(lib, call, who):
    rc, msg = call(lib)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith(who)
    rc, msg = call(lib, pos=None, cap=0, counts=None, **(dict(lens=None) if call is call_rec else {}))
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    if call is call_rec:
        rc, msg = call(lib, max_len=0)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, blocksize=0, nblocks=1)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    # nblocks = 0 is success only with a context to enqueue the zeroing of d_totals on
    rc, msg = call(lib, stream=None, index=None, sub=None, errs=None, nblocks=0, raw_size=0)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


@BOTH
@pytest.mark.parametrize("missing", ["stream", "index", "errs"])
def test_null_device_arrays(lib, call, who, missing):
    rc, msg = call(lib, **{missing: None})
    assert rc == HUFE_ARGUMENT and "are required" in msg and "needs a context" not in msg and msg.startswith(who)


@BOTH
def test_null_totals(lib, call, who):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, totals=None)
        assert rc == HUFE_ARGUMENT and "classes and d_totals are required" in msg and msg.startswith(who)


@BOTH
def test_missing_or_misaligned_sub_index(lib, call, who):
    for sub in (None, 0x30004, 0x30001):
        rc, msg = call(lib, sub=sub)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg and msg.startswith(who)


@BOTH
@pytest.mark.parametrize("kw", [
    dict(raw_size=5 * 4096),                            # five blocks
    dict(raw_size=3 * 4096),                            # three
    dict(raw_size=0),
    dict(blocksize=0),                                  # one block
    dict(nblocks=0),                                    # no blocks, but bytes
    dict(blocksize=(1 << 38) + 1, raw_size=4 * ((1 << 38) + 1)),
])
def test_a_layout_that_does_not_give_nblocks(lib, call, who, kw):
    rc, msg = call(lib, **kw)
    assert rc == HUFE_ARGUMENT and "must be those of the encode" in msg and msg.startswith(who)


def test_the_other_calls_keep_their_wording(lib):
    rc = lib.hufgpu_find_bytes(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, None, POS, 16, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode() == "find_bytes: the set and d_totals are required"
    rc = lib.hufgpu_find_pattern(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, b"a\nb", 3, None, 1, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode() == "find_pattern: pos_cap 1 needs d_pos"
    rc = lib.hufgpu_find_records(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, NEWLINE, b"a\nb", 3, POS, LEN, 1, 0, COUNTS, TOTALS,
                                 ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode().startswith("find_records: byte 1 of the pattern (value 10)")


# ---- byte_classes --------------------------------------------------------------------------------------------------------
def members(row):
    return [v for v in range(256) if row[v >> 3] >> (v & 7) & 1]


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
def bracket(values):
    return b"[" + b"".join(b"\\x%02x" % v for v in sorted(values)) + b"]"


def regex(sets):
    return b"".join(bracket(s) for s in sets)


def re_positions(data, sets, blocksize, cap=0, served=None):
    """the same answer from re.finditer: a look-ahead sees overlapping matches"""
    raw, n, m = bytes(data), len(data), len(sets)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    pos, counts = [], [0] * nb
    for hit in re.finditer(b"(?=(" + regex(sets) + b"))", raw, re.DOTALL):
        p = hit.start()
        if all(served[b] for b in range(p // bs, (p + m - 1) // bs + 1)):
            pos.append(p)
            counts[p // bs] += 1
    written = min(len(pos), cap)
    return pos[:written], counts, [len(pos), written, nb - sum(served), 0]


def re_records(data, sets, delims, blocksize, cap=0, max_len=0, served=None):
    """... and from bytes.split (one delimiter value) or re.split, with re.search a piece"""
    raw, n = bytes(data), len(data)
    delims = sorted(set(bytes(delims)))
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pieces = [raw] if not delims else raw.split(bytes(delims)) if len(delims) == 1 else re.split(bracket(delims), raw, flags=re.DOTALL)
    want = re.compile(regex(sets), re.DOTALL)
    pos, lens, counts, cut = [], [], [0] * nb, []
    s = 0
    for piece in pieces if n else []:
        e = s + len(piece)
        if want.search(piece) and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            pos.append(s)
            lens.append(min(e - s, clip))
            cut.append(e - s > clip)
            counts[s // bs] += 1
        s = e + 1
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])]


def random_sets(rng, m, alphabet, width):
    """m classes of 1 to `width` values of the alphabet"""
    return [sorted(set(int(v) for v in rng.choice(alphabet, int(rng.integers(1, width + 1))))) for _ in range(m)]


def same_positions(data, sets, blocksize, cap=0, served=None):
    got = find_classes_model(data, sets, blocksize, cap, served)
    want = re_positions(data, sets, blocksize, cap, served)
    assert tuple(g.tolist() for g in got) == want
    return want


def same_records(data, sets, delims, blocksize, cap=0, max_len=0, served=None):
    got = find_class_records_model(data, sets, delims, blocksize, cap, max_len, served)
    want = re_records(data, sets, delims, blocksize, cap, max_len, served)
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

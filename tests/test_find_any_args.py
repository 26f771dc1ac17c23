"""hufgpu_find_any and hufgpu_find_records_any: the symbols, their declarations, their argument checks, the NumPy models of
their results, and GpuCodec.AnyOf / alt_classes (no GPU needed).

As for the class calls (tests/test_find_classes_args.py, whose cases are repeated here with the `find_any:` /
`find_records_any:` wording) argument errors are found before anything is enqueued and before the context is looked at, so
they can be provoked with a NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which
check spoke.  The models are checked against Python's `re` on `bytes`: an alternation of bracket expressions under a
look-ahead for the positions - with the served rule applied per alternative -, bytes.split and re.search for the records.
"""
import os
import re

import numpy as np
import pytest

from find_any_model import find_any_model, find_any_records_model
from find_classes_model import find_class_records_model, find_classes_model
from find_model import byte_set
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM, INDEX, SUB, POS, LEN, COUNTS, TOTALS, ERRS = 0x10000, 0x20000, 0x30008, 0x40000, 0x48000, 0x50000, 0x60000, 0x70000
NEWLINE = byte_set(b"\n")
FULL, EMPTY = bytes([255] * 32), bytes(32)
DEFAULT = object()
AnyOf = GpuCodec.AnyOf


def alts_of(*alternatives):
    """the two C arrays: 32 bytes a class, the alternatives one behind the other, and their lengths"""
    return (b"".join(byte_set(s) for a in alternatives for s in a), np.array([len(a) for a in alternatives], np.uint32).tobytes(),
            len(alternatives))


ALTS = alts_of([b"eE", b"rR", b"rR"], [b"f", b"a", b"t", b"a", b"l"], [b"pP"])


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call_pos(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, alts=ALTS,
             cls=DEFAULT, lens=DEFAULT, n=DEFAULT, pos=POS, cap=16, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    cls, lens, n = (alts[0] if cls is DEFAULT else cls, alts[1] if lens is DEFAULT else lens, alts[2] if n is DEFAULT else n)
    rc = lib.hufgpu_find_any(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, cls, lens, n, pos, cap, counts,
                             totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


def call_rec(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, delims=NEWLINE,
             alts=ALTS, cls=DEFAULT, lens=DEFAULT, n=DEFAULT, pos=POS, rlens=LEN, cap=16, max_len=128, counts=COUNTS, totals=TOTALS,
             errs=ERRS, flags=0):
    cls, lens, n = (alts[0] if cls is DEFAULT else cls, alts[1] if lens is DEFAULT else lens, alts[2] if n is DEFAULT else n)
    rc = lib.hufgpu_find_records_any(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, delims, cls, lens, n, pos,
                                     rlens, cap, max_len, counts, totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


CALLS = [(call_pos, "find_any:"), (call_rec, "find_records_any:")]
BOTH = pytest.mark.parametrize("call,who", CALLS, ids=["positions", "records"])
LAYOUTS = ((4, 4 * 4096), (0, 0))


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


# ---- the new cases -------------------------------------------------------------------------------------------------------
@BOTH
def test_null_arrays_and_counts_of_0_and_65(lib, call, who):
    for kw in (dict(cls=None), dict(lens=None), dict(cls=None, lens=None), dict(n=0), dict(n=65), dict(n=0xFFFFFFFF),
               dict(alts=alts_of(*[[b"x"]] * 65))):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg, (kw, msg)
    for kw in (dict(cls=None), dict(lens=None)):
        rc, msg = call(lib, **kw)
        assert "classes, alt_lens and d_totals are required" in msg
    rc, msg = call(lib, n=0)
    assert "n_alts 0 is not 1 to 64" in msg
    rc, msg = call(lib, alts=alts_of(*[[b"x"]] * 65))
    assert "n_alts 65 is not 1 to 64" in msg
    for alts in (alts_of([b"xy"]), alts_of([b"xy"] * 64), alts_of(*[[b"xy"]] * 64), alts_of([b"x"] * 31, [b"y"] * 33),
                 alts_of([b"x"], [b"y"] * 63)):     # the ends of what is allowed reach the last check
        rc, msg = call(lib, alts=alts)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith(who), msg


@BOTH
@pytest.mark.parametrize("lens,at", [([0], 0), ([3, 0, 2], 1), ([1, 1, 0], 2), ([1] * 63 + [0], 63), ([0, 70], 0)])
def test_an_alternative_of_length_0(lib, call, who, lens, at):
    cls = b"".join([byte_set(b"ab")] * 64)
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, cls=cls, lens=np.array(lens, np.uint32).tobytes(), n=len(lens))
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg, msg
        assert f"alternative {at} has length 0" in msg


@BOTH
@pytest.mark.parametrize("lens", [[65], [64, 1], [32, 33], [1] * 63 + [2], [2, 5, 33, 25], [0xFFFFFFFF, 2], [0x80000000, 0x80000000]])
def test_a_total_above_64(lib, call, who, lens):
    cls = b"".join([byte_set(b"ab")] * 64)                 # (never read past: the total is looked at first)
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, cls=cls, lens=np.array(lens, np.uint32).tobytes(), n=len(lens))
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and "needs a context" not in msg, msg
        assert f"sum to {sum(lens)}" in msg and "above 64" in msg


@BOTH
@pytest.mark.parametrize("lens,j,k", [([5], 0, 0), ([5], 0, 4), ([2, 5, 33], 1, 2), ([2, 5, 33], 2, 32), ([31, 33], 1, 0), ([1] * 64, 63, 0),
                                      ([1, 63], 1, 62), ([32, 32], 0, 31)])
def test_an_empty_class(lib, call, who, lens, j, k):
    alts = [[b"ab"] * m for m in lens]
    alts[j][k] = b""
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts))
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and "is empty" in msg and "needs a context" not in msg, msg
        assert f"class {k} of alternative {j} " in msg


@pytest.mark.parametrize("lens,j,k", [([5], 0, 0), ([2, 5, 33], 1, 4), ([2, 5, 33], 2, 0), ([31, 33], 1, 32), ([1] * 64, 40, 0), ([1, 63], 0, 0)])
def test_a_class_that_meets_the_delimiter_set(lib, lens, j, k):
    alts = [[b"ab"] * m for m in lens]
    alts[j][k] = b"a\nz"
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts))
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records_any:") and "holds a delimiter" in msg, msg
        assert "needs a context" not in msg and f"class {k} of alternative {j} " in msg and "(value 10)" in msg
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts), delims=byte_set(b"\r\x00"))   # (no delimiter now)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
        rc, msg = call_pos(lib, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts))         # the positions' call has no delimiters
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_rec(lib, alts=alts_of([b"a"], [b"b", [3, 255]]), delims=byte_set([255]))
    assert rc == HUFE_ARGUMENT and "class 1 of alternative 1 holds a delimiter (value 255)" in msg


def test_the_full_class_and_the_delimiter_set(lib):
    for cls, j, k in (((FULL + byte_set(b"a"), np.array([1, 1], np.uint32).tobytes(), 2), 0, 0),
                      ((byte_set(b"a") + byte_set(b"b") + FULL, np.array([1, 2], np.uint32).tobytes(), 2), 1, 1)):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, alts=cls)
            assert rc == HUFE_ARGUMENT and "holds a delimiter" in msg and f"class {k} of alternative {j} " in msg and "(value 10)" in msg
            assert "needs a context" not in msg
        rc, msg = call_rec(lib, alts=cls, delims=EMPTY)    # the empty delimiter set: valid
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
        rc, msg = call_pos(lib, alts=cls)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_a_null_delimiter_set(lib):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call_rec(lib, nblocks=nblocks, raw_size=raw_size, delims=None)
        assert rc == HUFE_ARGUMENT and msg.startswith("find_records_any:") and "delim_set is required" in msg, msg
        assert "needs a context" not in msg
    rc, msg = call_rec(lib, delims=EMPTY)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_rec(lib, delims=byte_set(range(256)), cls=None)
    assert "classes, alt_lens and d_totals are required" in msg


def test_a_cap_without_both_outputs(lib):
    for kw in (dict(pos=None), dict(rlens=None), dict(pos=None, rlens=None)):
        for cap in (1, 16):
            rc, msg = call_rec(lib, cap=cap, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith("find_records_any:") and "needs d_rec_pos and d_rec_len" in msg, (kw, msg)
            assert f"rec_cap {cap}" in msg and "needs a context" not in msg
        rc, msg = call_rec(lib, cap=0, **kw)             # with rec_cap = 0 both may be NULL
        assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call_pos(lib, pos=None, cap=1)
    assert rc == HUFE_ARGUMENT and "needs d_pos" in msg and msg.startswith("find_any:")


# ---- the cases of the older calls ----------------------------------------------------------------------------------------
@BOTH
def test_valid_arguments_still_need_a_context(lib, call, who):
    rc, msg = call(lib)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith(who)
    rc, msg = call(lib, pos=None, cap=0, counts=None, **(dict(rlens=None) if call is call_rec else {}))
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
        assert rc == HUFE_ARGUMENT and "classes, alt_lens and d_totals are required" in msg and msg.startswith(who)


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
    rc = lib.hufgpu_find_classes(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, None, 3, POS, 1, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT and lib.hufgpu_last_error(None).decode() == "find_classes: the classes and d_totals are required"
    rc = lib.hufgpu_find_records_classes(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, NEWLINE, byte_set(b"a") + byte_set(b"\n"), 2,
                                         POS, LEN, 1, 0, COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT
    assert lib.hufgpu_last_error(None).decode().startswith("find_records_classes: class 1 of the pattern holds a delimiter (value 10)")


# ---- AnyOf and alt_classes -----------------------------------------------------------------------------------------------
def members(row):
    return [v for v in range(256) if row[v >> 3] >> (v & 7) & 1]


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
def bracket(values):
    return b"[" + b"".join(b"\\x%02x" % v for v in sorted(values)) + b"]"


def regex(sets):
    return b"".join(bracket(s) for s in sets)


def re_positions(data, alts, blocksize, cap=0, served=None):
    """the same answer from re.finditer: per alternative a look-ahead sees overlapping matches, and the served rule is the
    alternative's own; a start counts once"""
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    found = set()
    for sets in alts:
        for hit in re.finditer(b"(?=(" + regex(sets) + b"))", raw, re.DOTALL):
            p = hit.start()
            if all(served[b] for b in range(p // bs, (p + len(sets) - 1) // bs + 1)):
                found.add(p)
    pos, counts = sorted(found), [0] * nb
    for p in pos:
        counts[p // bs] += 1
    written = min(len(pos), cap)
    return pos[:written], counts, [len(pos), written, nb - sum(served), 0]


def re_records(data, alts, delims, blocksize, cap=0, max_len=0, served=None):
    """... and from bytes.split (one delimiter value) or re.split, with re.search of the ALTERNATION a piece"""
    raw, n = bytes(data), len(data)
    delims = sorted(set(bytes(delims)))
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pieces = [raw] if not delims else raw.split(bytes(delims)) if len(delims) == 1 else re.split(bracket(delims), raw, flags=re.DOTALL)
    want = re.compile(b"|".join(b"(?:" + regex(sets) + b")" for sets in alts), re.DOTALL)
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

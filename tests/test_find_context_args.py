"""hufgpu_find_records_context: the symbol, its declaration, its argument checks, the NumPy model of its results
(tests/find_context_model.py) and the `before` / `after` / `context` keywords of GpuCodec (no GPU needed).

As for the older find calls argument errors are found before anything is enqueued and before the context is looked at, so
they can be provoked with a NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which
check spoke.  Every argument case of hufgpu_find_records_select (tests/test_find_select_args.py) is repeated here with the
`find_records_context:` wording, for distances of 0 and others.  The model is checked against plain Python over
`bytes.split`: the indices of the selected pieces, a window around each, the union, the empty pieces dropped.
"""
import inspect
import os
import re

import numpy as np
import pytest

from find_context_model import find_context_model
from find_model import byte_set
from find_select_model import NO_UNKNOWN, find_select_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec
from test_find_any_args import ALTS, DEFAULT, EMPTY, FULL, LAYOUTS, NEWLINE, alts_of, regex
from test_find_select_args import random_case

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, INDEX, SUB, POS, LEN, NO, SEL, COUNTS, TOTALS, ERRS = (0x10000, 0x20000, 0x30008, 0x40000, 0x48000, 0x4c000, 0x4e000, 0x50000,
                                                               0x60000, 0x70000)
WHO = "find_records_context:"
AnyOf = GpuCodec.AnyOf
FAR = 2**32 - 1
DISTANCES = [(0, 1), (1, 0), (2, 2), (0, 5), (7, 0), (3, 40), (FAR, FAR)]
WINDOWS = pytest.mark.parametrize("ba", [(0, 0), (2, 3), (FAR, FAR)], ids=["select", "2-3", "all"])


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, delims=NEWLINE,
         alts=ALTS, cls=DEFAULT, lens=DEFAULT, n=DEFAULT, select=0, ba=(2, 3), pos=POS, rlens=LEN, no=NO, sel=SEL, cap=16, max_len=128,
         counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    cls, lens, n = (alts[0] if cls is DEFAULT else cls, alts[1] if lens is DEFAULT else lens, alts[2] if n is DEFAULT else n)
    rc = lib.hufgpu_find_records_context(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, delims, cls, lens, n, select,
                                         ba[0], ba[1], pos, rlens, no, sel, cap, max_len, counts, totals, errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


def select_call(lib, stream=STREAM, index=INDEX, sub=SUB, raw_size=4 * 4096, delims=NEWLINE, alts=ALTS, cls=DEFAULT, n=DEFAULT, select=0,
                pos=POS):
    """hufgpu_find_records_select with what `call` passes for the same keywords"""
    cls, n = (alts[0] if cls is DEFAULT else cls, alts[2] if n is DEFAULT else n)
    return lib.hufgpu_find_records_select(None, stream, 1000, index, 4, sub, raw_size, 4096, delims, cls, alts[1], n, select, pos, LEN, NO, 16,
                                          128, COUNTS, TOTALS, ERRS, 0, None)


def valid(rc, msg):
    """every check but the last has passed"""
    return rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith(WHO)


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
            assert valid(*call(lib, select=select, ba=ba, **out, **kw)), (out, kw)
        rc, msg = call(lib, select=select, ba=ba, pos=None, **out)      # neither stands in for one of the two other outputs
        assert rc == HUFE_ARGUMENT and "needs d_rec_pos and d_rec_len" in msg and msg.startswith(WHO)


@pytest.mark.parametrize("ba", [(0, 0), (0, 1), (1, 0), (0x80000000, 5), (FAR, 0), (0, FAR), (FAR, FAR)])
def test_any_distance_is_valid(lib, ba):
    for select in (0, 1):
        assert valid(*call(lib, select=select, ba=ba))


# ---- every argument case of hufgpu_find_records_select, with no context at all, in the same order ----------------------------
@WINDOWS
def test_null_arrays_and_counts_of_0_and_65(lib, ba):
    for kw in (dict(cls=None), dict(lens=None), dict(cls=None, lens=None), dict(n=0), dict(n=65), dict(n=0xFFFFFFFF),
               dict(alts=alts_of(*[[b"x"]] * 65))):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, ba=ba, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "needs a context" not in msg, (kw, msg)
    for kw in (dict(cls=None), dict(lens=None)):
        assert "classes, alt_lens and d_totals are required" in call(lib, ba=ba, **kw)[1]
    assert "n_alts 0 is not 1 to 64" in call(lib, ba=ba, n=0)[1]
    assert "n_alts 65 is not 1 to 64" in call(lib, ba=ba, alts=alts_of(*[[b"x"]] * 65))[1]
    for alts in (alts_of([b"xy"]), alts_of([b"xy"] * 64), alts_of(*[[b"xy"]] * 64), alts_of([b"x"] * 31, [b"y"] * 33)):
        assert valid(*call(lib, ba=ba, alts=alts))


@WINDOWS
def test_lengths_classes_and_delimiters(lib, ba):
    cls = b"".join([byte_set(b"ab")] * 64)
    for nblocks, raw_size in LAYOUTS:
        kw = dict(nblocks=nblocks, raw_size=raw_size, ba=ba)
        rc, msg = call(lib, cls=cls, lens=np.array([3, 0, 2], np.uint32).tobytes(), n=3, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "alternative 1 has length 0" in msg
        rc, msg = call(lib, cls=cls, lens=np.array([32, 33], np.uint32).tobytes(), n=2, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "sum to 65" in msg and "above 64" in msg
        rc, msg = call(lib, alts=alts_of([b"ab"] * 2, [b"ab", b"ab", b""]), **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "class 2 of alternative 1 is empty" in msg
        for select in (0, 1):
            rc, msg = call(lib, alts=alts_of([b"ab"] * 2, [b"ab", b"a\nz"]), select=select, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "class 1 of alternative 1 holds a delimiter (value 10)" in msg
        rc, msg = call(lib, alts=(FULL + byte_set(b"a"), np.array([1, 1], np.uint32).tobytes(), 2), select=1, **kw)
        assert rc == HUFE_ARGUMENT and "class 0 of alternative 0 holds a delimiter" in msg and "needs a context" not in msg
        rc, msg = call(lib, delims=None, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "delim_set is required" in msg and "needs a context" not in msg
        rc, msg = call(lib, totals=None, **kw)
        assert rc == HUFE_ARGUMENT and "classes, alt_lens and d_totals are required" in msg and msg.startswith(WHO)
    assert valid(*call(lib, alts=(FULL + byte_set(b"a"), np.array([1, 1], np.uint32).tobytes(), 2), delims=EMPTY, ba=ba))
    assert valid(*call(lib, delims=EMPTY, ba=ba))


@WINDOWS
def test_caps_layouts_and_device_arrays(lib, ba):
    for kw in (dict(pos=None), dict(rlens=None), dict(pos=None, rlens=None)):
        for cap in (1, 16):
            rc, msg = call(lib, cap=cap, ba=ba, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(WHO) and "needs d_rec_pos and d_rec_len" in msg, (kw, msg)
            assert f"rec_cap {cap}" in msg and "needs a context" not in msg
        assert valid(*call(lib, cap=0, ba=ba, **kw))
    for missing in ("stream", "index", "errs"):
        rc, msg = call(lib, ba=ba, **{missing: None})
        assert rc == HUFE_ARGUMENT and "are required" in msg and "needs a context" not in msg and msg.startswith(WHO)
    for sub in (None, 0x30004, 0x30001):
        rc, msg = call(lib, sub=sub, ba=ba)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg and msg.startswith(WHO)
    for kw in (dict(raw_size=5 * 4096), dict(raw_size=3 * 4096), dict(raw_size=0), dict(blocksize=0), dict(nblocks=0),
               dict(blocksize=(1 << 38) + 1, raw_size=4 * ((1 << 38) + 1))):
        rc, msg = call(lib, ba=ba, **kw)
        assert rc == HUFE_ARGUMENT and "must be those of the encode" in msg and msg.startswith(WHO)
    for select in (0, 1):
        assert valid(*call(lib, select=select, ba=ba, pos=None, rlens=None, no=None, sel=None, cap=0, counts=None))
        assert valid(*call(lib, select=select, ba=ba, max_len=0))
        assert valid(*call(lib, select=select, ba=ba, blocksize=0, nblocks=1))
        assert valid(*call(lib, select=select, ba=ba, stream=None, index=None, sub=None, errs=None, nblocks=0, raw_size=0))


def test_the_order_of_the_checks_is_the_select_call_s(lib):
    """every pair of mistakes: both calls complain about the same one"""
    mistakes = [dict(select=2), dict(cls=None), dict(n=0), dict(delims=None), dict(pos=None), dict(index=None), dict(sub=0x30004),
                dict(raw_size=5 * 4096), dict(alts=alts_of([b"a\n"]))]
    for i, a in enumerate(mistakes):
        for b in mistakes[i:]:
            kw = {**a, **b}
            rc, msg = call(lib, **kw)
            select_call(lib, **kw)
            other = lib.hufgpu_last_error(None).decode()
            assert rc == HUFE_ARGUMENT and msg == other.replace("find_records_select:", WHO), (kw, msg, other)


def test_the_select_call_keeps_its_wording(lib):
    rc = lib.hufgpu_find_records_select(None, STREAM, 1000, INDEX, 4, SUB, 4 * 4096, 4096, NEWLINE, None, None, 1, 0, POS, LEN, NO, 1, 0,
                                        COUNTS, TOTALS, ERRS, 0, None)
    assert rc == HUFE_ARGUMENT
    assert lib.hufgpu_last_error(None).decode() == "find_records_select: the classes, alt_lens and d_totals are required"


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

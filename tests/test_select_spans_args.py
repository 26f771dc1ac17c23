"""hufgpu_select_spans: its declaration, every argument error that the host finds - each with no context at all, message for
message -, and the model of its result, tests/select_spans_model.py, against two independent truths (no GPU needed).

The truths.  For a pattern and a short text, the span at a start p is the largest L <= 64 for which re.fullmatch takes
text[p:p + L]: a brute-force search, no bit trick and no searchsorted.  What grep -o prints is then a plain loop: at p, a span
is taken and p moves behind it, or p moves on by one.  Where the machine has a grep, `LC_ALL=C grep -a -o -b -E` says the same
on one-line inputs.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from find_args_support import HUFE_ARGUMENT, declaration, lib, valid  # noqa: F401
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec
from select_spans_model import offending_rank, select_model

NAME = "select_spans"
POS, LEN, N, SPOS, SLEN, SRANK, TOTALS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
SLOTS = ("ctx", "pos", "len", "n", "n_cap", "sel_pos", "sel_len", "sel_rank", "sel_cap", "pad_pos", "totals", "flags", "stream")
DEFAULTS = dict(ctx=None, pos=POS, len=LEN, n=N, n_cap=100, sel_pos=SPOS, sel_len=SLEN, sel_rank=SRANK, sel_cap=100, pad_pos=0,
                totals=TOTALS, flags=0, stream=None)


def call(lib, **kw):
    """the call with a NULL context and made-up device pointers, which are never dereferenced: (status, the message)"""
    assert not set(kw) - set(SLOTS), sorted(set(kw) - set(SLOTS))
    values = dict(DEFAULTS, **kw)
    rc = lib.hufgpu_select_spans(*[values[s] for s in SLOTS])
    return rc, lib.hufgpu_last_error(None).decode()


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_declared(lib):
    for name in ("hufgpu_select_spans", "hufgpu_select_geometry"):
        assert name in _native.GPU_EXTRA_SYMBOLS and hasattr(lib, name)
    assert len(lib.hufgpu_select_spans.argtypes) == len(SLOTS)
    header, m = declaration(NAME)
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()              # noqa: E731
    assert m and squeeze(m.group(1)) == (", const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_n, uint64_t n_cap, "
                                         "uint64_t *d_sel_pos, uint32_t *d_sel_len, uint64_t *d_sel_rank, uint64_t sel_cap, "
                                         "uint64_t pad_pos, uint64_t *d_sel_totals, uint32_t flags, void *stream")
    assert re.search(r"#define\s+HUFGPU_SELECT_PAD\s+1u", header) and re.search(r"void\s+hufgpu_select_geometry\(uint32_t out\[2\]\);", header)
    limit = re.search(r"#define\s+HUFGPU_SELECT_MAX\s+\(1ull << (\d+)\)", header)
    assert limit and 1 << int(limit.group(1)) == _native.SELECT_MAX >= 1 << 30 and _native.SELECT_PAD == 1
    about = header[header.index("SELECT SPANS"):header.index("#define HUFGPU_SELECT_PAD")]
    assert "this is the set that grep -o -E prints" in about and "Otherwise it is the greedy selection over what was" in about
    for words in ("records calls", "lengths above", "leftmost-FIRST", "another length", "fused search + select"):
        assert words in about[about.index("OUT OF SCOPE"):], words
    # the span call's own text no longer leaves the selection to nobody
    spans = header[header.index("FIND, MATCH SPANS"):header.index("int hufgpu_find_any_spans")]
    assert "hufgpu_select_spans() selects from them" in spans


def test_the_geometry(lib):
    """ranks a tile, tiles a composition group: the successor window of 64 fits a tile, and four levels reach the maximum"""
    import ctypes
    out = (ctypes.c_uint32 * 2)()
    lib.hufgpu_select_geometry(out)
    tile, fan = int(out[0]), int(out[1])
    assert tile >= 64 and tile % 64 == 0 and fan >= 2 and tile * fan ** 4 >= _native.SELECT_MAX
    lib.hufgpu_select_geometry(None)                                # (nothing to write to: nothing happens)


# ---- the argument errors -------------------------------------------------------------------------------------------------
def test_valid_arguments_still_need_a_context(lib):
    for kw in ({}, {"n": None}, {"sel_rank": None}, {"flags": 1, "pad_pos": 12345}, {"n_cap": 0}, {"n_cap": _native.SELECT_MAX},
               {"sel_cap": 0, "sel_pos": None, "sel_len": None, "sel_rank": None}, {"sel_cap": 1 << 40}, {"n_cap": 0, "sel_cap": 0},
               {"sel_pos": POS + 8}, {"totals": N + 8}):
        rc, msg = call(lib, **kw)
        assert valid(rc, msg, NAME + ":") and msg == "select_spans: needs a context (there is no CPU path)", (kw, msg)


ERRORS = [({"pos": None}, "select_spans: d_pos, d_len and d_sel_totals are required"),
          ({"len": None}, "select_spans: d_pos, d_len and d_sel_totals are required"),
          ({"totals": None}, "select_spans: d_pos, d_len and d_sel_totals are required"),
          ({"pos": None, "n_cap": 0}, "select_spans: d_pos, d_len and d_sel_totals are required"),
          ({"sel_pos": None}, "select_spans: sel_cap 100 needs d_sel_pos and d_sel_len"),
          ({"sel_len": None, "sel_cap": 7}, "select_spans: sel_cap 7 needs d_sel_pos and d_sel_len"),
          ({"n_cap": _native.SELECT_MAX + 1}, "select_spans: n_cap 1073741825 is above HUFGPU_SELECT_MAX, 1073741824"),
          ({"n_cap": 1 << 63}, "select_spans: n_cap 9223372036854775808 is above HUFGPU_SELECT_MAX, 1073741824"),
          ({"flags": 2}, "select_spans: flags 0x2 has a bit other than HUFGPU_SELECT_PAD"),
          ({"flags": 0x80000001}, "select_spans: flags 0x80000001 has a bit other than HUFGPU_SELECT_PAD"),
          ({"sel_pos": POS}, "select_spans: d_sel_pos starts at the address of d_pos"),
          ({"sel_len": LEN}, "select_spans: d_sel_len starts at the address of d_len"),
          ({"sel_rank": POS}, "select_spans: d_sel_rank starts at the address of d_pos"),
          ({"totals": N}, "select_spans: d_sel_totals starts at the address of d_n"),
          ({"sel_pos": LEN}, "select_spans: d_sel_pos starts at the address of d_len"),
          ({"totals": POS}, "select_spans: d_sel_totals starts at the address of d_pos")]


@pytest.mark.parametrize("kw,message", ERRORS, ids=["%d-%s" % (i, "-".join(kw)) for i, (kw, _) in enumerate(ERRORS)])
def test_every_host_error_message_for_message(lib, kw, message):
    rc, msg = call(lib, **kw)
    assert rc == HUFE_ARGUMENT and msg == message, msg


def test_the_order_of_the_checks(lib):
    """the required pointers, the outputs of a cap, n_cap, the flags, the aliases, the context"""
    steps = [({"pos": None}, "are required"), ({"sel_pos": None}, "needs d_sel_pos"), ({"n_cap": 1 << 31}, "is above"),
             ({"flags": 4}, "has a bit"), ({"sel_rank": LEN}, "starts at the address"), ({}, "needs a context")]
    for first in range(len(steps)):
        kw = {}
        for k, _ in steps[first:]:
            kw.update(k)
        rc, msg = call(lib, **kw)
        assert rc == HUFE_ARGUMENT and steps[first][1] in msg, (first, msg)


# ---- the model against re and against grep -----------------------------------------------------------------------------------
ADDRESS = rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"
CASES = [(rb"[0-9]{1,3}", b"1234 x 7 12 123 1234567 99"), (rb"colou?r", b"colour color colou colourcolor ccolor"),
         (rb"GET|GETS", b"GETS GET GETGETS GE GETSGET"), (rb"a{1,64}", b"a" * 200), (rb"a{1,64}", b"b" + b"a" * 64 + b"b" + b"a" * 65 + b"ba"),
         (ADDRESS, b"from 10.0.0.1 to 192.168.100.2554 via 1.2.3.4.5.6.7.8 and 1234.5.6.7"), (rb"ab?", b"abab a b abb aab"),
         (rb"a?b", b"abab a b abb aab"), (rb"x{2,5}", b"x xx xxx xxxxxx xxxxxxxxxxxx"), (rb"req-[0-9a-f]{1,8}", b"req-1 req-0123456789 req- req-abcdefg"),
         (rb"took [0-9]{1,5}ms", b"took 5ms took 123456ms took 12345ms took ms"), (rb"aa|aaa|aaaa", b"aaaaaaaaa aa a aaa"),
         (rb"[a-z]{2,4}", b"abcdefghij k lm nop"), (rb"ab|abab|b", b"ababab bab abb")]


def longest_forms(pattern, text):
    """{start: the longest L <= 64 with a full match of text[start:start + L]}"""
    e = re.compile(pattern)
    out = {}
    for p in range(len(text)):
        for L in range(min(64, len(text) - p), 0, -1):
            if e.fullmatch(text, p, p + L):
                out[p] = L
                break
    return out


def plain_loop(spans, n):
    """what grep -o prints of them: [(start, length)]"""
    out, p = [], 0
    while p < n:
        if p in spans:
            out.append((p, spans[p]))
            p += spans[p]
        else:
            p += 1
    return out


def model_of(spans, **kw):
    pos = np.array(sorted(spans), np.uint64)
    lens = np.array([spans[p] for p in sorted(spans)], np.int32)
    return select_model(pos, lens, **kw), pos, lens


@pytest.mark.parametrize("pattern,text", CASES, ids=[p.decode() + "-%d" % i for i, (p, _) in enumerate(CASES)])
def test_the_model_against_re_and_a_plain_loop(pattern, text):
    spans = longest_forms(pattern, text)
    want = plain_loop(spans, len(text))
    (spos, slens, ranks, totals), pos, lens = model_of(spans)
    assert list(zip(spos.tolist(), slens.tolist())) == want and totals.tolist() == [len(want), len(want), 0, 0]
    assert pos[ranks].tolist() == spos.tolist() and lens[ranks].tolist() == slens.tolist() and ranks[0] == 0
    # the caps: the first rows of the same answer, the count unchanged
    for cap in (0, 1, len(want)):
        (cpos, clens, cranks, ctot), _, _ = model_of(spans, cap=cap)
        assert cpos.tolist() == spos[:cap].tolist() and cranks.tolist() == ranks[:cap].tolist() and ctot.tolist() == [len(want), cap, 0, 0]
    # n below the size: the selection over the first n spans
    n = len(spans) // 2
    (npos, _, _, ntot), _, _ = model_of(spans, n=n)
    first = dict(list(sorted(spans.items()))[:n])
    assert npos.tolist() == [p for p, _ in plain_loop(first, len(text))] and ntot[0] == len(npos)


def test_most_cases_have_overlapping_starts_to_drop():
    dropping = [p for p, t in CASES if len(plain_loop(longest_forms(p, t), len(t))) < len(longest_forms(p, t))]
    assert len(dropping) >= 8 and rb"[0-9]{1,3}" in dropping and rb"a{1,64}" in dropping and ADDRESS in dropping, dropping


def test_the_model_by_hand():
    spans = longest_forms(rb"[0-9]{1,3}", b"1234")
    assert sorted(spans.items()) == [(0, 3), (1, 3), (2, 2), (3, 1)]
    got = select_model([0, 1, 2, 3], [3, 3, 2, 1])
    assert [a.tolist() for a in got] == [[0, 3], [3, 1], [0, 3], [2, 2, 0, 0]]
    assert select_model([], [])[3].tolist() == [0, 0, 0, 0]
    far = 1 << 32
    got = select_model([far - 2, far - 1, far, far + 1], [2, 2, 64, 1])
    assert got[0].tolist() == [far - 2, far] and got[2].tolist() == [0, 2]
    # invalid input: the lowest offending rank, and nothing else
    for pos, lens, rank in (([5, 5, 9], [1, 1, 1], 1), ([5, 9, 7], [1, 1, 1], 2), ([5, 6, 7], [1, 0, 1], 1), ([5, 6, 7], [1, 1, 65], 2),
                            ([5, 6, 7], [65, 0, 1], 0), ([9, 6, 6], [1, 1, 1], 1)):
        assert offending_rank(pos, lens) == rank
        got = select_model(pos, lens)
        assert got[3].tolist() == [0, 0, HUFE_ARGUMENT, rank] and got[0].size == got[1].size == got[2].size == 0
    assert select_model([5, 5, 9], [1, 1, 1], n=1)[3].tolist() == [1, 1, 0, 0]         # (the pair lies behind n)


GREP = shutil.which("grep")


@pytest.mark.skipif(GREP is None, reason="no grep on this machine")
@pytest.mark.parametrize("pattern,text", CASES, ids=[p.decode() + "-%d" % i for i, (p, _) in enumerate(CASES)])
def test_the_model_against_grep(pattern, text):
    assert b"\n" not in text
    run = subprocess.run([GREP, "-a", "-o", "-b", "-E", "-e", pattern.decode()], input=text + b"\n", stdout=subprocess.PIPE,
                         env=dict(os.environ, LC_ALL="C"), check=True)
    want = []
    for line in run.stdout.splitlines():
        at, _, found = line.partition(b":")
        want.append((int(at), len(found)))
        assert text[int(at):int(at) + len(found)] == found
    (spos, slens, _, _), _, _ = model_of(longest_forms(pattern, text))
    assert list(zip(spos.tolist(), slens.tolist())) == want


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_the_keywords_validate_on_a_bare_codec():
    """what raises before the first device call needs no context"""
    bare = GpuCodec.__new__(GpuCodec)
    with pytest.raises(ValueError, match="give spans=True"):
        bare.redact(None, 0, None, 0, None, 100, 10, b"abc", max_matches=4, nonoverlapping=True)
    with pytest.raises(ValueError, match="give one"):
        bare.redact(None, 0, None, 0, None, 100, 10, b"abc", max_matches=4, spans=True, lines=True, nonoverlapping=True, max_len=8)
    for call_ in (bare.find_matches, bare.count_matches):
        with pytest.raises(TypeError, match="selects records"):
            call_(None, 0, None, 0, None, 100, 10, GpuCodec.AllOf(b"a", b"b"), max_positions=4)
    with pytest.raises(TypeError, match="selects records"):
        bare.extract(None, 0, None, 0, None, 100, 10, GpuCodec.AllOf(b"a", b"b"), 4, nonoverlapping=True)
    assert GpuCodec.SELECT_MAX == _native.SELECT_MAX

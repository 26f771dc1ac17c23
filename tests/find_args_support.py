"""Helpers of the argument tests of the search family (tests/test_find_*args.py), once each: made-up device pointers, ONE
caller for the eleven C calls of tests/find_calls.py with a default for every slot, what `valid` means, and the cross-checks
against Python's `re` that several of the models' tests share.  Not a test module.

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked with a
NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.
"""
import os
import re

import numpy as np
import pytest

from find_calls import CALLS, invoke
from find_model import byte_set
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, INDEX, SUB, POS, LEN, NO, SEL, COUNTS, TOTALS, ERRS = (0x10000, 0x20000, 0x30008, 0x40000, 0x48000, 0x4c000, 0x4e000, 0x50000,
                                                               0x60000, 0x70000)
LAYOUTS = ((4, 4 * 4096), (0, 0))                         # (nblocks, raw_size): four blocks, and none
NEWLINE = byte_set(b"\n")
FULL, EMPTY = bytes([255] * 32), bytes(32)
WORDS = byte_set(GpuCodec.WORD_BYTES)
DEFAULT = object()
FAR = 2**32 - 1


def classes_of(*sets):
    """the C array: 32 bytes a class"""
    return b"".join(byte_set(s) for s in sets)


def alts_of(*alternatives):
    """the two C arrays: 32 bytes a class, the alternatives one behind the other, and their lengths"""
    return (b"".join(byte_set(s) for a in alternatives for s in a), np.array([len(a) for a in alternatives], np.uint32).tobytes(),
            len(alternatives))


SET = byte_set([10])
PAT = b"ERROR"
CLS = classes_of(b"eE", b"rR", b"rR", b"oO", b"rR")
ALTS = alts_of([b"eE", b"rR", b"rR"], [b"f", b"a", b"t", b"a", b"l"], [b"pP"])
# slot -> what a call gets when the test says nothing: valid arguments, four blocks of 4 096 bytes
DEFAULTS = dict(ctx=None, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, st=SET,
                pattern=PAT, plen=DEFAULT, delims=NEWLINE, words=WORDS, anchors=4, select=0, before=2, after=3, pos=POS, rlens=LEN, no=NO,
                sel=SEL, cap=16, max_len=128, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0, hip_stream=None)


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call(lib, name, **kw):
    """the C call `name` with a NULL context and DEFAULTS in every slot that `kw` does not name; (status, the message).
    `alts` = (classes, alt_lens, n_alts) stands for the three slots of the any-of table (default: ALTS; a class call gets CLS),
    `ba` = (before, after) for those two; `plen` defaults to the length of the pattern or of the classes given"""
    slots = CALLS[name]
    values = dict(DEFAULTS)
    if "lens" in slots:
        alts = kw.pop("alts", ALTS)
        values.update(cls=alts[0], lens=alts[1], n=alts[2])
    else:
        values.update(cls=CLS)
    if "ba" in kw:
        values["before"], values["after"] = kw.pop("ba")
    unknown = set(kw) - set(slots)
    assert not unknown, (name, "has no", sorted(unknown))
    values.update(kw)
    if values["plen"] is DEFAULT:
        key = values["pattern"] if "pattern" in slots else values["cls"]
        values["plen"] = 5 if key is None else len(key) // (1 if "pattern" in slots else 32)
    rc = invoke(lib, name, values)
    return rc, lib.hufgpu_last_error(None).decode()


def valid(rc, msg, prefix):
    """every check but the last has passed"""
    return rc == HUFE_ARGUMENT and "needs a context" in msg and msg.startswith(prefix)


def declaration(name):
    """(the header's text, the match of the call's declaration in it: group 1 is the arguments behind ctx)"""
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    return header, re.search(r"\bint\s+hufgpu_" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)


# ---- the models' cross-checks against `re` ---------------------------------------------------------------------------------
def members(row):
    return [v for v in range(256) if row[v >> 3] >> (v & 7) & 1]


def bracket(values):
    return b"[" + b"".join(b"\\x%02x" % v for v in sorted(values)) + b"]"


def regex(sets):
    return b"".join(bracket(s) for s in sets)


def re_positions(data, alts, blocksize, cap=0, served=None):
    """the models' positions from re.finditer: per alternative a look-ahead sees overlapping matches, and the served rule is
    the alternative's own; a start counts once"""
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
    """... and the records from bytes.split (one delimiter value) or re.split, with re.search of the ALTERNATION a piece"""
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


def random_case(rng, mix, alphabet, trial):
    """(data, alternatives of the lengths `mix`, n, blocksize): lines of four letters or of all values, the data starting and
    ending with and without a delimiter in turn"""
    values = np.array([97, 98, 99, 10]) if alphabet == "four letters" else np.arange(256)
    n, bs = int(rng.integers(1, 700)), int(rng.integers(0, 90))
    data = (rng.choice(values, n, p=[0.30, 0.30, 0.30, 0.10]) if values.size == 4 else rng.choice(values, n)).astype(np.uint8)
    if values.size == 256:
        data[rng.integers(0, n, n // 6 + 1)] = 10           # lines, and now and then two delimiters in a row
    if trial % 3 == 0:
        data[0] = 10                                        # a delimiter as byte 0
    data[n - 1] = 10 if trial % 2 else 97                   # the data ends with and without one
    alts = []
    wide = trial % 2 == 0
    for m in mix:
        if alphabet == "four letters":
            narrow = rng.integers(0, max(m // 3, 1), m) == 0
            sets = [sorted(set(int(v) for v in rng.choice(values[:3], 1 if m <= 5 and not wide else 2, replace=False))) if narrow[k]
                    else [97, 98, 99] for k in range(m)]
        else:
            sets = [[v for v in range(256) if v != 10 and rng.integers(0, 64 if wide or m > 5 else 2)] or [1] for _ in range(m)]
        alts.append(sets)
    return data, alts, n, bs

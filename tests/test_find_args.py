"""hufgpu_find_bytes: the symbol, its declaration, its argument checks and the NumPy model of its result (no GPU needed).

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked
with a NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from find_model import block_lens, byte_set, find_model
from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM, INDEX, SUB, POS, COUNTS, TOTALS, ERRS = 0x10000, 0x20000, 0x30008, 0x40000, 0x50000, 0x60000, 0x70000
SET = byte_set([10])


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=4, sub=SUB, raw_size=4 * 4096, blocksize=4096, st=SET,
         pos=POS, cap=16, counts=COUNTS, totals=TOTALS, errs=ERRS, flags=0):
    rc = lib.hufgpu_find_bytes(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, st, pos, cap, counts, totals,
                               errs, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_find_bytes" in _native.GPU_SYMBOLS
    assert hasattr(lib, "hufgpu_find_bytes")
    assert len(lib.hufgpu_find_bytes.argtypes) == 16
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    m = re.search(r"\bint\s+hufgpu_find_bytes\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(0).count(",") == 15


def test_valid_arguments_still_need_a_context(lib):
    rc, msg = call(lib)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, pos=None, cap=0, counts=None)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, blocksize=0, nblocks=1)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    # nblocks = 0 is success only with a context to enqueue the zeroing of d_totals on
    rc, msg = call(lib, stream=None, index=None, sub=None, errs=None, nblocks=0, raw_size=0)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


@pytest.mark.parametrize("missing", ["stream", "index", "errs"])
def test_null_device_arrays(lib, missing):
    rc, msg = call(lib, **{missing: None})
    assert rc == HUFE_ARGUMENT and "are required" in msg and "needs a context" not in msg


@pytest.mark.parametrize("missing", ["st", "totals"])
def test_null_set_or_totals(lib, missing):
    for nblocks, raw_size in ((4, 4 * 4096), (0, 0)):
        rc, msg = call(lib, nblocks=nblocks, raw_size=raw_size, **{missing: None})
        assert rc == HUFE_ARGUMENT and "set and d_totals are required" in msg


def test_a_cap_without_positions(lib):
    rc, msg = call(lib, pos=None, cap=1)
    assert rc == HUFE_ARGUMENT and "needs d_pos" in msg


def test_missing_or_misaligned_sub_index(lib):
    for sub in (None, 0x30004, 0x30001):
        rc, msg = call(lib, sub=sub)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg


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
    assert rc == HUFE_ARGUMENT and "must be those of the encode" in msg


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_byte_set_bits():
    assert byte_set([]) == bytes(32)
    assert byte_set(range(256)) == b"\xff" * 32
    s = byte_set([10, 255, 8])
    assert s[1] == 0b101 and s[31] == 0x80 and sum(s) == 5 + 0x80


def test_model_positions_counts_and_caps():
    data = np.array([1, 2, 1, 3, 1, 1, 2], np.uint8)
    assert block_lens(7, 3) == [3, 3, 1] and block_lens(7, 0) == [7] and block_lens(0, 3) == []
    pos, counts, totals = find_model(data, [1], 3, cap=10)
    assert pos.tolist() == [0, 2, 4, 5] and counts.tolist() == [2, 2, 0] and totals.tolist() == [4, 4, 0, 0]
    pos, counts, totals = find_model(data, [1, 2], 3, cap=3)
    assert pos.tolist() == [0, 1, 2] and counts.tolist() == [3, 2, 1] and totals.tolist() == [6, 3, 0, 0]
    pos, counts, totals = find_model(data, [1], 0, cap=0)
    assert pos.size == 0 and counts.tolist() == [4] and totals.tolist() == [4, 0, 0, 0]
    pos, counts, totals = find_model(data, [], 3, cap=5)
    assert pos.size == 0 and counts.tolist() == [0, 0, 0] and totals.tolist() == [0, 0, 0, 0]


def test_model_blocks_that_are_not_served():
    data = np.array([1, 2, 1, 3, 1, 1, 2], np.uint8)
    pos, counts, totals = find_model(data, [1], 3, cap=10, served=[True, False, True])
    assert pos.tolist() == [0, 2] and counts.tolist() == [2, 0, 0] and totals.tolist() == [2, 2, 1, 0]
    pos, counts, totals = find_model(np.zeros(0, np.uint8), [1], 3, cap=10)
    assert pos.size == 0 and counts.size == 0 and totals.tolist() == [0, 0, 0, 0]

"""hufgpu_decode_ranges: the symbol, its declaration and its argument checks (no GPU needed).

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked
with a NULL context and NULL device pointers; hufgpu_last_error(NULL) says which check spoke.
"""
import ctypes as C
import os
import re

import pytest

from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def u64s(values):
    values = [int(v) for v in values]
    return (C.c_uint64 * max(1, len(values)))(*values)


def call(lib, lo, hi, oo, n=None, sub=None, raw_size=0, blocksize=0, nblocks=4, errs=True, raws=True):
    n = len(lo) if n is None else n
    e = (C.c_int32 * max(1, n))() if errs else None
    r = (C.c_uint64 * max(1, n))() if raws else None
    rc = lib.hufgpu_decode_ranges(None, None, 1000, None, nblocks, n, u64s(lo) if lo is not None else None,
                                  u64s(hi) if hi is not None else None, u64s(oo) if oo is not None else None,
                                  sub, raw_size, blocksize, None, 0, e, r, None)
    return rc, lib.hufgpu_last_error(None).decode()


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_decode_ranges" in _native.GPU_SYMBOLS
    assert hasattr(lib, "hufgpu_decode_ranges")
    assert len(lib.hufgpu_decode_ranges.argtypes) == 17
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    assert re.search(r"\bint\s+hufgpu_decode_ranges\s*\(\s*hufgpu_ctx_t\s*\*ctx", header)


def test_no_ranges_is_success(lib):
    rc, _ = call(lib, None, None, None, n=0, errs=False, raws=False)
    assert rc == HUFE_OK


def test_a_range_that_ends_in_front_of_its_start(lib):
    rc, msg = call(lib, [0, 10], [5, 9], [0, 5, 5])
    assert rc == HUFE_ARGUMENT and "range 1 ends in front of its start" in msg


def test_decreasing_out_offsets(lib):
    rc, msg = call(lib, [0, 10], [5, 12], [0, 5, 4])
    assert rc == HUFE_ARGUMENT and "out_offsets must not decrease (range 1)" in msg


@pytest.mark.parametrize("missing", ["lo", "hi", "oo", "errs", "raws"])
def test_null_host_arrays(lib, missing):
    lo, hi, oo = [0], [5], [0, 5]
    rc, msg = call(lib, None if missing == "lo" else lo, None if missing == "hi" else hi, None if missing == "oo" else oo,
                   n=1, errs=missing != "errs", raws=missing != "raws")
    assert rc == HUFE_ARGUMENT and "are required" in msg


def test_misaligned_or_missized_sub_index(lib):
    rc, msg = call(lib, [0], [5], [0, 5], sub=C.c_void_p(0x1004), raw_size=4 * 4096, blocksize=4096)
    assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
    # aligned, but (raw_size, blocksize) do not give the stream's 4 blocks
    rc, msg = call(lib, [0], [5], [0, 5], sub=C.c_void_p(0x1008), raw_size=5 * 4096, blocksize=4096)
    assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
    rc, msg = call(lib, [0], [5], [0, 5], sub=C.c_void_p(0x1008), raw_size=0, blocksize=4096)
    assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg


def test_valid_arguments_still_need_a_context(lib):
    rc, msg = call(lib, [0, 3], [5, 3], [0, 5, 5])
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, [0], [5], [0, 5], sub=C.c_void_p(0x1008), raw_size=4 * 4096, blocksize=4096)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg

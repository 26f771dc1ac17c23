"""hufgpu_update_ranges: the symbol, its declaration and its argument checks (no GPU needed).

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked
with a NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.
"""
import ctypes as C
import os
import re

import pytest

from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STREAM, INDEX, SRC, OUT, OUT_INDEX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # far apart: nothing overlaps


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def u64s(values):
    values = [int(v) for v in values]
    return (C.c_uint64 * max(1, len(values)))(*values)


def call(lib, lo, hi, so=None, n=None, sub=None, out_sub=None, raw_size=0, blocksize=0, nblocks=4, stream=STREAM,
         stream_len=1000, index=INDEX, src=SRC, out=OUT, out_cap=4096, out_index=OUT_INDEX):
    n = len(lo) if n is None else n
    out_len, count = C.c_uint64(77), C.c_uint64(77)
    rc = lib.hufgpu_update_ranges(None, stream, stream_len, index, nblocks, n, u64s(lo) if lo is not None else None,
                                  u64s(hi) if hi is not None else None, u64s(so) if so is not None else None, src,
                                  sub, raw_size, blocksize, out, out_cap, out_index, out_sub, 0,
                                  C.byref(out_len), C.byref(count), None)
    assert (out_len.value, count.value) == (0, 0)          # on any error *out_len = 0
    return rc, lib.hufgpu_last_error(None).decode()


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_update_ranges" in _native.GPU_SYMBOLS
    assert hasattr(lib, "hufgpu_update_ranges")
    assert len(lib.hufgpu_update_ranges.argtypes) == 21
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    assert re.search(r"\bint\s+hufgpu_update_ranges\s*\(\s*hufgpu_ctx_t\s*\*ctx", header)


def test_a_range_that_ends_in_front_of_its_start(lib):
    rc, msg = call(lib, [0, 10], [5, 9])
    assert rc == HUFE_ARGUMENT and "range 1 ends in front of its start" in msg


@pytest.mark.parametrize("missing", ["lo", "hi"])
def test_null_host_arrays(lib, missing):
    rc, msg = call(lib, None if missing == "lo" else [0], None if missing == "hi" else [5], n=1)
    assert rc == HUFE_ARGUMENT and "are required" in msg


@pytest.mark.parametrize("lo, hi, pair", [
    ([0, 4], [5, 9], "0 and 1"),                        # plain overlap
    ([10, 0], [20, 11], "1 and 0"),                     # given in the other order
    ([0, 10], [100, 20], "0 and 1"),                    # nested
    ([7, 7], [9, 9], "0 and 1"),                        # duplicate
    ([0, 50, 3, 49], [10, 60, 3, 51], "3 and 1"),       # an empty range between them does not hide the overlap
])
def test_overlapping_ranges(lib, lo, hi, pair):
    rc, msg = call(lib, lo, hi)
    assert rc == HUFE_ARGUMENT and f"ranges {pair} overlap" in msg


@pytest.mark.parametrize("lo, hi", [
    ([0, 5], [5, 9]),                                   # touching
    ([5, 0], [9, 5]),
    ([0, 3, 3, 3], [10, 3, 3, 3]),                      # empty ranges, also inside another range and on one another
    ([4, 0, 10], [4, 10, 12]),
    ([8], [8]),
])
def test_touching_and_empty_ranges_pass_the_overlap_check(lib, lo, hi):
    rc, msg = call(lib, lo, hi)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_misaligned_or_missized_sub_index(lib):
    for which in ("sub", "out_sub"):
        kw = {which: C.c_void_p(0x61004)}
        rc, msg = call(lib, [0], [5], raw_size=4 * 4096, blocksize=4096, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
        kw = {which: C.c_void_p(0x61008)}
        # aligned, but (raw_size, blocksize) do not give the stream's 4 blocks
        rc, msg = call(lib, [0], [5], raw_size=5 * 4096, blocksize=4096, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
        rc, msg = call(lib, [0], [5], raw_size=0, blocksize=4096, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
    # a new sub-index with rows of the chunked path's blocks, as in hufgpu_encode_batch
    rc, msg = call(lib, [0], [5], out_sub=C.c_void_p(0x61008), raw_size=4 << 21, blocksize=1 << 21)
    assert rc == HUFE_ARGUMENT and "blocks below" in msg
    rc, msg = call(lib, [0], [5], sub=C.c_void_p(0x61008), raw_size=4 << 21, blocksize=1 << 21)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg          # (the OLD one may have them)


@pytest.mark.parametrize("kw", [
    dict(out=STREAM),                                   # in place
    dict(out=STREAM + 996),                             # the last byte of the stream
    dict(out=STREAM - 4092),                            # the first byte of the stream
    dict(out=INDEX + 8 * 4),                            # the old index' last entry
    dict(out=SRC - 4092),                               # the new bytes
    dict(out_index=INDEX),
    dict(out_index=OUT + 4090),
    dict(out_index=STREAM + 500),
    dict(sub=C.c_void_p(0x70000), out_sub=C.c_void_p(0x70000 + 8), raw_size=4 * 4096, blocksize=4096),
    dict(out_sub=C.c_void_p(OUT + 8), raw_size=4 * 4096, blocksize=4096),
])
def test_overlapping_buffers(lib, kw):
    rc, msg = call(lib, [0], [10], **kw)
    assert rc == HUFE_ARGUMENT and "output buffers overlap" in msg


def test_misaligned_output(lib):
    for off in (1, 2, 3):
        rc, msg = call(lib, [0], [10], out=OUT + off)
        assert rc == HUFE_ARGUMENT and "4-byte aligned" in msg


def test_buffers_that_touch_do_not_overlap(lib):
    rc, msg = call(lib, [0], [10], out=STREAM + 1000)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, [0], [10], out=STREAM - 4096)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_valid_arguments_still_need_a_context(lib):
    rc, msg = call(lib, [0, 3], [3, 9])
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, None, None, n=0)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = call(lib, [0], [5], sub=C.c_void_p(0x61008), out_sub=C.c_void_p(0x71008), raw_size=4 * 4096, blocksize=4096)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg

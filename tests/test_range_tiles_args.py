"""HUFGPU_RANGES_TILES and hufgpu_ranges_counters: the flag, the symbol, its declaration and its argument checks (no GPU
needed).

Argument errors are found before a GPU is touched, so they can be provoked with a NULL context and made-up device
pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.
"""
import ctypes as C
import inspect
import os
import re

import pytest

from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, INDEX, SUB, OUT = 0x10000, 0x20000, 0x30000, 0x40000


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def header():
    return open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()


def test_counters_need_a_context_and_an_array(lib):
    counters = (C.c_uint64 * 8)(*([77] * 8))
    assert lib.hufgpu_ranges_counters(None, counters) == HUFE_ARGUMENT
    assert list(counters) == [77] * 8
    assert lib.hufgpu_ranges_counters(C.c_void_p(0x1000), None) == HUFE_ARGUMENT     # (the context is not looked at)
    assert lib.hufgpu_ranges_counters(None, None) == HUFE_ARGUMENT


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_ranges_counters" in _native.GPU_SYMBOLS and hasattr(lib, "hufgpu_ranges_counters")
    assert len(lib.hufgpu_ranges_counters.argtypes) == 2
    assert re.search(r"\bint\s+hufgpu_ranges_counters\s*\(\s*hufgpu_ctx_t\s*\*ctx,\s*uint64_t\s+counters\[8\]\)", header())


def test_the_flag(lib):
    assert _native.RANGES_TILES == 4
    flags = dict(re.findall(r"#define\s+(HUFGPU_(?:STRICT_TREE|RELAXED_TREE|SEQUENTIAL|RANGES_TILES))\s+(\d+)u", header()))
    assert flags == {"HUFGPU_STRICT_TREE": "0", "HUFGPU_RELAXED_TREE": "1", "HUFGPU_SEQUENTIAL": "2", "HUFGPU_RANGES_TILES": "4"}
    assert len({_native.STRICT_TREE, _native.RELAXED_TREE, _native.SEQUENTIAL, _native.RANGES_TILES}) == 4
    assert _native.RANGES_TILES & (_native.RELAXED_TREE | _native.SEQUENTIAL) == 0


def test_the_python_interface():
    from libhuffman_amd.codec import GpuCodec
    for name in ("decode_ranges", "decode_range"):
        p = inspect.signature(getattr(GpuCodec, name)).parameters
        assert "tiles" in p and p["tiles"].default is False
    assert callable(GpuCodec.ranges_counters)


def ranges_call(lib, flags, lo=(0, 10), hi=(5, 20), oo=(0, 5, 15), sub=None, raw_size=0, blocksize=0, nblocks=4):
    n = len(lo)
    errs, raws = (C.c_int32 * n)(*([77] * n)), (C.c_uint64 * n)(*([77] * n))
    rc = lib.hufgpu_decode_ranges(None, STREAM, 1000, INDEX, nblocks, n, (C.c_uint64 * n)(*lo), (C.c_uint64 * n)(*hi),
                                  (C.c_uint64 * (n + 1))(*oo), sub, raw_size, blocksize, OUT, flags, errs, raws, None)
    return rc, lib.hufgpu_last_error(None).decode(), list(errs), list(raws)


@pytest.mark.parametrize("kw", [
    dict(),                                                             # no context: there is no CPU path
    dict(sub=SUB, raw_size=4 * 4096, blocksize=4096),                   # ... with a sub-index that fits
    dict(lo=(9, 10)),                                                   # a range that ends in front of its start
    dict(oo=(0, 5, 4)),                                                 # decreasing slots
    dict(sub=SUB + 4, raw_size=4 * 4096, blocksize=4096),               # a misaligned sub-index
    dict(sub=SUB, raw_size=5 * 4096, blocksize=4096),                   # a sub-index of another layout
], ids=["no-context", "no-context-sub", "lo-gt-hi", "slots-decrease", "sub-misaligned", "sub-layout"])
def test_the_flag_changes_no_argument_check(lib, kw):
    plain = ranges_call(lib, 0, **kw)
    assert plain[0] == HUFE_ARGUMENT
    assert ranges_call(lib, _native.RANGES_TILES, **kw) == plain
    assert ranges_call(lib, _native.RANGES_TILES | _native.RELAXED_TREE, **kw) == plain

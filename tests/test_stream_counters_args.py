"""hufgpu_stream_counters: the symbol, its declaration, its argument checks and its place in the Python interface (no GPU
needed).

Argument errors are found before a GPU is touched, so they can be provoked with a NULL context and a made-up one (never
dereferenced)."""
import ctypes as C
import os
import re

import pytest

from libhuffman_amd import _native

HUFE_ARGUMENT = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def header():
    return open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()


def test_counters_need_a_context_and_an_array(lib):
    counters = (C.c_uint64 * 8)(*([77] * 8))
    assert lib.hufgpu_stream_counters(None, counters) == HUFE_ARGUMENT
    assert list(counters) == [77] * 8
    assert lib.hufgpu_stream_counters(C.c_void_p(0x1000), None) == HUFE_ARGUMENT     # (the context is not looked at)
    assert lib.hufgpu_stream_counters(None, None) == HUFE_ARGUMENT


def test_symbol_is_exported_and_declared(lib):
    assert "hufgpu_stream_counters" in _native.GPU_SYMBOLS and hasattr(lib, "hufgpu_stream_counters")
    assert len(lib.hufgpu_stream_counters.argtypes) == 2
    assert lib.hufgpu_stream_counters.argtypes == lib.hufgpu_ranges_counters.argtypes
    assert re.search(r"\bint\s+hufgpu_stream_counters\s*\(\s*hufgpu_ctx_t\s*\*ctx,\s*uint64_t\s+counters\[8\]\)", header())


def test_the_declaration_says_what_every_word_is():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+hufgpu_stream_counters", header(), re.S)
    assert m
    for word in range(8):
        assert f"[{word}]" in m.group(1), word
    assert "touches no GPU" in m.group(1) and "Results never depend" in m.group(1)


def test_the_python_interface():
    from libhuffman_amd.codec import GpuCodec
    assert callable(GpuCodec.stream_counters)


def test_the_read_out_makes_no_gpu_call():
    """the function's body: two checks and a copy of host values"""
    src = open(os.path.join(ROOT, "libhuffman_amd", "csrc", "host", "stream.hpp")).read()
    m = re.search(r'extern "C" int hufgpu_stream_counters\([^)]*\)\s*\{(.*?)\n\}', src, re.S)
    assert m and "hip" not in m.group(1) and "HIP_OK" not in m.group(1)
    for entry in ("hufgpu_block_index", "hufgpu_decode_stream"):            # both entry points start from zeros
        body = re.search(r'extern "C" int ' + entry + r"\(.*?\n\}", src, re.S).group(0)
        assert "memset(ctx->scounters, 0, sizeof(ctx->scounters));" in body, entry

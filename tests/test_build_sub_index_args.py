"""hufgpu_sub_index_from_raw, hufgpu_decode_build_sub, hufgpu_build_sub_index: the symbols, their declarations and
their argument checks (no GPU needed).

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked
with a NULL context and made-up device pointers; hufgpu_last_error(NULL) says which check spoke.
"""
import ctypes as C
import os
import re

import pytest

from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hufgpu_sub_index_from_raw", "hufgpu_decode_build_sub", "hufgpu_build_sub_index")
P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def call(lib, name, stream=0x10000, offsets=0x20000, raw=0x30000, raw_size=4 * 4096, blocksize=4096, sub=0x40008,
         out_cap=4 * 4096, ctx=None):
    """the call `name` with made-up device pointers (0 = NULL) -> (rc, last error, unbuilt, raw_len)"""
    unbuilt, raw_len = C.c_uint64(77), C.c_uint64(77)
    st, of, sb = P(stream or None), P(offsets or None), P(sub or None)
    if name == "hufgpu_sub_index_from_raw":
        rc = lib.hufgpu_sub_index_from_raw(ctx, st, 1000, of, P(raw or None), raw_size, blocksize, sb, 0, C.byref(unbuilt), None)
    elif name == "hufgpu_decode_build_sub":
        rc = lib.hufgpu_decode_build_sub(ctx, st, 1000, of, raw_size, blocksize, P(raw or None), out_cap, sb, 0,
                                         C.byref(raw_len), C.byref(unbuilt), None)
    else:
        rc = lib.hufgpu_build_sub_index(ctx, st, 1000, of, raw_size, blocksize, sb, 0, C.byref(unbuilt), None)
    return rc, lib.hufgpu_last_error(None).decode(), unbuilt.value, raw_len.value


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_declared(lib, name):
    assert name in _native.GPU_SYMBOLS
    assert hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == {"hufgpu_sub_index_from_raw": 11, "hufgpu_decode_build_sub": 13,
                                                "hufgpu_build_sub_index": 10}[name]
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*hufgpu_ctx_t\s*\*ctx", header)


@pytest.mark.parametrize("name", NAMES)
def test_no_data_is_success(lib, name):
    rc, _, unbuilt, raw_len = call(lib, name, stream=0, offsets=0, raw=0, raw_size=0, sub=0, out_cap=0)
    assert rc == HUFE_OK and unbuilt == 0
    if name == "hufgpu_decode_build_sub":
        assert raw_len == 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("missing", ["stream", "offsets"])
def test_null_stream_or_index(lib, name, missing):
    rc, msg, _, _ = call(lib, name, **{missing: 0})
    assert rc == HUFE_ARGUMENT and "the stream or its block index is missing" in msg and name[len("hufgpu_"):] in msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sub", [0, 0x40004, 0x40001])
def test_missing_or_misaligned_sub_index(lib, name, sub):
    rc, msg, _, _ = call(lib, name, sub=sub)
    assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg


def test_from_raw_needs_the_data(lib):
    rc, msg, _, _ = call(lib, "hufgpu_sub_index_from_raw", raw=0)
    assert rc == HUFE_ARGUMENT and "the decoded data is missing" in msg


def test_decode_build_sub_needs_its_output(lib):
    rc, msg, _, _ = call(lib, "hufgpu_decode_build_sub", raw=0)
    assert rc == HUFE_ARGUMENT and "the output buffer is missing" in msg


@pytest.mark.parametrize("name", NAMES)
def test_blocks_beyond_the_kernel_limit(lib, name):
    rc, msg, _, _ = call(lib, name, raw_size=1 << 40, blocksize=1 << 39)
    assert rc == HUFE_ARGUMENT and "blocks of more than" in msg


@pytest.mark.parametrize("name", NAMES)
def test_valid_arguments_still_need_a_context(lib, name):
    rc, msg, _, _ = call(lib, name)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg

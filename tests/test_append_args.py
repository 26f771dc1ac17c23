"""hufgpu_append and hufgpu_truncate: the symbols, their declarations and their argument checks (no GPU needed).

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

STREAM, INDEX, SRC, SUB, OUT_SUB = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000       # far apart: nothing overlaps
BS = 4096
RAW = 4 * BS + 100                                      # five blocks, a tail of 100 bytes


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def append(lib, stream=STREAM, stream_len=1000, stream_cap=60000, index=INDEX, raw_size=RAW, blocksize=BS, src=SRC,
           src_len=3 * BS, sub=None, out_sub=None):
    out_len = C.c_uint64(77)
    rc = lib.hufgpu_append(None, stream, stream_len, stream_cap, index, raw_size, blocksize, src, src_len, sub, out_sub, 0,
                           C.byref(out_len), None)
    assert out_len.value == 0                           # on any error *out_len = 0
    return rc, lib.hufgpu_last_error(None).decode()


def truncate(lib, stream=STREAM, stream_len=1000, index=INDEX, raw_size=RAW, blocksize=BS, new_raw_size=BS + 5, sub=None,
             out_sub=None):
    out_len = C.c_uint64(77)
    rc = lib.hufgpu_truncate(None, stream, stream_len, index, raw_size, blocksize, new_raw_size, sub, out_sub, 0,
                             C.byref(out_len), None)
    assert out_len.value == 0
    return rc, lib.hufgpu_last_error(None).decode()


def test_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    for name, nargs in (("hufgpu_append", 14), ("hufgpu_truncate", 12)):
        assert name in _native.GPU_SYMBOLS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(\s*hufgpu_ctx_t\s*\*ctx" % name, header)


def test_valid_arguments_still_need_a_context(lib):
    for rc, msg in (append(lib), append(lib, raw_size=0, stream_len=0),
                    append(lib, sub=C.c_void_p(SUB), out_sub=C.c_void_p(OUT_SUB)), truncate(lib),
                    truncate(lib, new_raw_size=0),
                    truncate(lib, sub=C.c_void_p(SUB), out_sub=C.c_void_p(OUT_SUB))):
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_nothing_to_do_is_success_and_needs_no_context(lib):
    out_len = C.c_uint64(77)
    rc = lib.hufgpu_append(None, STREAM, 1000, 60000, INDEX, RAW, BS, None, 0, None, None, 0, C.byref(out_len), None)
    assert (rc, out_len.value) == (HUFE_OK, 1000)       # src_len = 0: *out_len = stream_len
    out_len = C.c_uint64(77)
    rc = lib.hufgpu_truncate(None, STREAM, 1000, INDEX, RAW, BS, RAW, None, None, 0, C.byref(out_len), None)
    assert (rc, out_len.value) == (HUFE_OK, 1000)       # new_raw_size = raw_size
    # the argument checks come first all the same
    rc, msg = append(lib, src_len=0, src=None, stream=STREAM + 2)
    assert rc == HUFE_ARGUMENT and "4-byte aligned" in msg


def test_blocksize_zero(lib):
    for rc, msg in (append(lib, blocksize=0), truncate(lib, blocksize=0)):
        assert rc == HUFE_ARGUMENT and "needs the blocksize" in msg


def test_stream_longer_than_its_buffer(lib):
    rc, msg = append(lib, stream_len=1001, stream_cap=1000)
    assert rc == HUFE_ARGUMENT and "longer than its buffer" in msg
    rc, msg = append(lib, stream_len=1000, stream_cap=1000)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_missing_stream_index_or_new_bytes(lib):
    for kw in (dict(stream=None), dict(index=None)):
        rc, msg = append(lib, **kw)
        assert rc == HUFE_ARGUMENT and "is missing" in msg and "stream or its block index" in msg
        rc, msg = truncate(lib, **kw)
        assert rc == HUFE_ARGUMENT and "stream or its block index" in msg
    rc, msg = append(lib, src=None)
    assert rc == HUFE_ARGUMENT and "new bytes are missing" in msg


def test_truncate_to_more_than_there_is(lib):
    rc, msg = truncate(lib, new_raw_size=RAW + 1)
    assert rc == HUFE_ARGUMENT and "above the old one" in msg


def test_misaligned_stream(lib):
    for off in (1, 2, 3):
        rc, msg = append(lib, stream=STREAM + off)
        assert rc == HUFE_ARGUMENT and "4-byte aligned" in msg
        rc, msg = truncate(lib, stream=STREAM + off)
        assert rc == HUFE_ARGUMENT and "4-byte aligned" in msg


def test_misaligned_sub_index_and_rows_of_the_chunked_route(lib):
    for which in ("sub", "out_sub"):
        kw = {which: C.c_void_p(SUB + 4)}
        rc, msg = append(lib, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
        rc, msg = truncate(lib, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg
    big = dict(raw_size=(3 << 21) + 5, blocksize=1 << 21)
    rc, msg = append(lib, out_sub=C.c_void_p(OUT_SUB), stream_cap=0x80000, src_len=10, **big)
    assert rc == HUFE_ARGUMENT and "blocks below" in msg
    rc, msg = truncate(lib, out_sub=C.c_void_p(OUT_SUB), new_raw_size=77, **big)
    assert rc == HUFE_ARGUMENT and "blocks below" in msg
    rc, msg = append(lib, sub=C.c_void_p(SUB), stream_cap=0x80000, src_len=10, **big)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg          # (the OLD one may have them)


@pytest.mark.parametrize("kw", [
    dict(src=STREAM),                                   # the new bytes inside the stream
    dict(src=STREAM + 59999),                           # the last byte of the stream's buffer, behind stream_len
    dict(src=STREAM - 3 * BS + 1),                      # the first byte of the stream
    dict(src=INDEX + 8 * 8 - 1),                        # the new index' last entry: 4 * 4096 + 100 + 3 * 4096 bytes are 8 blocks
    dict(index=STREAM + 1000),                          # the index inside the stream's buffer
    dict(sub=C.c_void_p(STREAM + 8)),
    dict(out_sub=C.c_void_p(STREAM + 50000)),
    dict(out_sub=C.c_void_p(INDEX + 8)),
    dict(sub=C.c_void_p(SRC + 8)),
    dict(out_sub=C.c_void_p(SRC - 8)),
    dict(sub=C.c_void_p(SUB), out_sub=C.c_void_p(SUB + 8)),
])
def test_overlapping_buffers(lib, kw):
    rc, msg = append(lib, **kw)
    assert rc == HUFE_ARGUMENT and "must not overlap" in msg


@pytest.mark.parametrize("kw", [
    dict(index=STREAM + 992),
    dict(sub=C.c_void_p(STREAM + 8)),
    dict(out_sub=C.c_void_p(INDEX + 8)),
    dict(sub=C.c_void_p(SUB), out_sub=C.c_void_p(SUB + 8)),
])
def test_overlapping_buffers_of_a_truncate(lib, kw):
    rc, msg = truncate(lib, **kw)
    assert rc == HUFE_ARGUMENT and "must not overlap" in msg


def test_buffers_that_touch_do_not_overlap(lib):
    rc, msg = append(lib, src=STREAM + 60000)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = append(lib, src=STREAM - 3 * BS)
    assert rc == HUFE_ARGUMENT and "needs a context" in msg
    rc, msg = append(lib, src=INDEX + 8 * 9)            # behind entry nb_new = 8
    assert rc == HUFE_ARGUMENT and "needs a context" in msg

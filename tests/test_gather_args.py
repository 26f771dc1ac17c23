"""hufgpu_gather: the symbol, its declaration and its argument checks (no GPU needed).

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

STREAM, INDEX, SUB, POS, LEN, OUT, ERRS, RAWS = (0x100000 * k for k in range(1, 9))
BS = 4096
RAW = 4 * BS + 100                                      # five blocks


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def gather(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=5, sub=SUB, raw_size=RAW, blocksize=BS, nrecords=10,
           pos=POS, lens=LEN, max_len=64, out=OUT, stride=64, errs=ERRS, raws=RAWS):
    rc = lib.hufgpu_gather(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, nrecords, pos, lens, max_len,
                           out, stride, errs, raws, 0, None)
    return rc, lib.hufgpu_last_error(None).decode()


def test_symbol_is_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    assert "hufgpu_gather" in _native.GPU_SYMBOLS and hasattr(lib, "hufgpu_gather")
    assert len(lib.hufgpu_gather.argtypes) == 18
    m = re.search(r"\bint\s+hufgpu_gather\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(1).count(",") == 17
    for name in ("d_pos", "d_len", "max_len", "out_stride", "d_errs", "d_raw_lens"):
        assert name in m.group(1)


def test_valid_arguments_still_need_a_context(lib):
    for rc, msg in (gather(lib), gather(lib, lens=None), gather(lib, raws=None), gather(lib, lens=None, raws=None, stride=1000),
                    gather(lib, blocksize=0, raw_size=RAW, nblocks=1), gather(lib, out=OUT + 3, stride=65)):
        assert rc == HUFE_ARGUMENT and "needs a context" in msg


def test_nothing_to_do_is_success_and_needs_no_context(lib):
    assert gather(lib, nrecords=0, pos=None, out=None, errs=None, raws=None, lens=None)[0] == HUFE_OK
    assert gather(lib, max_len=0, stride=0)[0] == HUFE_OK


@pytest.mark.parametrize("what", ["stream", "index", "pos", "out", "errs"])
def test_a_missing_device_array(lib, what):
    rc, msg = gather(lib, **{what: None})
    assert rc == HUFE_ARGUMENT and "are required" in msg


def test_a_stride_below_max_len(lib):
    rc, msg = gather(lib, stride=63)
    assert rc == HUFE_ARGUMENT and "out_stride" in msg


def test_sub_index_missing_or_misaligned(lib):
    for sub in (None, SUB + 4, SUB + 1):
        rc, msg = gather(lib, sub=sub)
        assert rc == HUFE_ARGUMENT and "sub-index" in msg


def test_a_layout_that_does_not_give_nblocks(lib):
    for kw in (dict(nblocks=4), dict(nblocks=6), dict(raw_size=0), dict(blocksize=0), dict(blocksize=BS + 100, nblocks=5),
               dict(raw_size=5 * BS + 1), dict(blocksize=1 << 39, raw_size=1 << 40, nblocks=2)):
        rc, msg = gather(lib, **kw)
        assert rc == HUFE_ARGUMENT and "(raw_size, blocksize)" in msg, kw


def test_more_parts_than_32_bits(lib):
    rc, msg = gather(lib, nrecords=1 << 31)
    assert rc == HUFE_ARGUMENT and "parts" in msg
    rc, msg = gather(lib, nrecords=(1 << 31) - 1, max_len=3 * BS, stride=3 * BS)
    assert rc == HUFE_ARGUMENT and "parts" in msg

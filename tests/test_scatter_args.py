"""hufgpu_scatter: the symbols, their declaration, the argument checks in their documented order, the touched-block bound,
and the Python layer's own validation (no GPU needed).

Argument errors are found before anything is enqueued and before the context is looked at, so they can be provoked with a
NULL context and made-up device pointers (never dereferenced); hufgpu_last_error(NULL) says which check spoke.  The order
is tested by breaking two arguments at once: the earlier check speaks.
"""
import os
import re

import numpy as np
import pytest

import scatter_model as model
from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x100

STREAM, INDEX, SUB, POS, LEN, SRC, OUT, OUT_INDEX, OUT_SUB, RESULT = (0x10000000 * k for k in range(1, 11))
BS = 4096
RAW = 4 * BS + 100                                      # five blocks


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def scatter(lib, stream=STREAM, stream_len=1000, index=INDEX, nblocks=5, sub=SUB, raw_size=RAW, blocksize=BS, nrecords=10,
            pos=POS, lens=LEN, max_len=64, src=SRC, stride=64, fill=0, cap=5, out=OUT, out_cap=4000, out_index=OUT_INDEX,
            out_sub=OUT_SUB, result=RESULT, flags=0):
    rc = lib.hufgpu_scatter(None, stream, stream_len, index, nblocks, sub, raw_size, blocksize, nrecords, pos, lens, max_len,
                            src, stride, fill, cap, out, out_cap, out_index, out_sub, result, flags, None)
    return rc, lib.hufgpu_last_error(None).decode()


# every check in the header's order: (keywords that trip it, a piece of its message)
CHECKS = [
    (dict(stream=None), "are required"),
    (dict(src=None), "d_src is required"),
    (dict(stride=63), "src_stride"),
    (dict(nblocks=4, cap=4), "(raw_size, blocksize)"),
    (dict(blocksize=1 << 21, raw_size=5 << 21), "needs blocks below 2097152"),
    (dict(cap=0), "touched_cap"),
    (dict(nrecords=1 << 31), "parts"),
    (dict(out=OUT + 2), "4-byte aligned"),
    (dict(out_sub=OUT_SUB + 4), "8-byte aligned"),
    (dict(out_index=OUT + 8), "overlap"),
]


def test_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "huffman_gpu.h")).read()
    for name in ("hufgpu_scatter", "hufgpu_scatter_touched_bound"):
        assert name in _native.GPU_SYMBOLS and hasattr(lib, name)
    assert len(lib.hufgpu_scatter.argtypes) == 23
    m = re.search(r"\bint\s+hufgpu_scatter\s*\(\s*hufgpu_ctx_t\s*\*ctx([^;]*)\)\s*;", header)
    assert m and m.group(1).count(",") == 22
    for name in ("d_pos", "d_len", "max_len", "d_src", "src_stride", "fill", "touched_cap", "d_out_block_offsets",
                 "d_out_sub_index", "d_result"):
        assert name in m.group(1)
    m = re.search(r"\buint64_t\s+hufgpu_scatter_touched_bound\s*\(([^;]*)\)\s*;", header)
    assert m and m.group(1).count(",") == 3 and len(lib.hufgpu_scatter_touched_bound.argtypes) == 4
    assert re.search(r"#define\s+HUFGPU_SCATTER_FILL\s+0x100u", header) and _native.SCATTER_FILL == FILL


def test_valid_arguments_still_need_a_context(lib):
    for kw in (dict(), dict(lens=None), dict(sub=None), dict(out_sub=None), dict(sub=None, out_sub=None),
               dict(flags=FILL, src=None, stride=0), dict(flags=FILL | 1), dict(blocksize=0, nblocks=1, cap=1),
               dict(src=SRC + 3, stride=65), dict(cap=1), dict(nrecords=0), dict(max_len=0, stride=0),
               dict(nrecords=0, pos=POS, flags=FILL, src=None)):
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg, (kw, msg)


@pytest.mark.parametrize("what", ["stream", "index", "pos", "out", "out_index", "result"])
def test_a_missing_device_array(lib, what):
    rc, msg = scatter(lib, **{what: None})
    assert rc == HUFE_ARGUMENT and msg.startswith("scatter: ") and "are required" in msg
    rc, msg = scatter(lib, nrecords=0, **{what: None})           # the "no records" case is checked like any other
    assert rc == HUFE_ARGUMENT and "are required" in msg


def test_every_check_speaks_with_its_message(lib):
    for kw, piece in CHECKS:
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith("scatter: ") and piece in msg, (kw, msg)


def test_the_checks_come_in_the_documented_order(lib):
    for i, (first, piece) in enumerate(CHECKS):
        for later, _ in CHECKS[i + 1:]:
            kw = dict(later)
            kw.update(first)                                     # (where both set one keyword, the earlier check's value)
            if set(first) & set(later):
                continue
            rc, msg = scatter(lib, **kw)
            assert rc == HUFE_ARGUMENT and piece in msg, (first, later, msg)
    # and all of them in front of the context
    rc, msg = scatter(lib, out_index=OUT + 8)
    assert "needs a context" not in msg


def test_source_checks_do_not_apply_with_fill(lib):
    for kw in (dict(src=None), dict(stride=0), dict(stride=63)):
        rc, msg = scatter(lib, flags=FILL, **kw)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg, kw


def test_a_layout_that_does_not_give_nblocks(lib):
    for kw in (dict(nblocks=4, cap=4), dict(nblocks=6), dict(raw_size=0), dict(blocksize=0), dict(blocksize=BS + 100),
               dict(raw_size=5 * BS + 1), dict(blocksize=1 << 39, raw_size=1 << 40, nblocks=2, cap=2)):
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and "(raw_size, blocksize)" in msg, kw


def test_blocks_of_the_chunked_encoder_are_not_served(lib):
    for kw in (dict(blocksize=1 << 21, raw_size=5 << 21), dict(blocksize=0, raw_size=1 << 21, nblocks=1, cap=1),
               dict(blocksize=3 << 20, raw_size=15 << 20)):
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and "2097152" in msg and "chunked" in msg, kw
    rc, msg = scatter(lib, blocksize=(1 << 21) - 1, raw_size=5 * ((1 << 21) - 1))
    assert "needs a context" in msg


def test_touched_cap_out_of_range(lib):
    for cap in (0, 6, 1 << 40):
        rc, msg = scatter(lib, cap=cap)
        assert rc == HUFE_ARGUMENT and "touched_cap" in msg, cap


def test_more_parts_than_32_bits(lib):
    rc, msg = scatter(lib, nrecords=1 << 31)
    assert rc == HUFE_ARGUMENT and "parts" in msg
    rc, msg = scatter(lib, nrecords=(1 << 31) - 1, max_len=3 * BS, stride=3 * BS)
    assert rc == HUFE_ARGUMENT and "parts" in msg
    # records of no bytes have no parts: max_len = 0 is the plain copy however many records it names, in blocks of any size
    for kw in (dict(nrecords=1 << 40), dict(nrecords=1 << 40, blocksize=1, raw_size=5, nblocks=5), dict(nrecords=1 << 31, flags=FILL)):
        rc, msg = scatter(lib, max_len=0, stride=0, **kw)
        assert rc == HUFE_ARGUMENT and "needs a context" in msg, (kw, msg)


def test_misaligned_buffers(lib):
    for off in (1, 2, 3):
        rc, msg = scatter(lib, out=OUT + off)
        assert rc == HUFE_ARGUMENT and "4-byte aligned" in msg
    for kw in (dict(sub=SUB + 4), dict(out_sub=OUT_SUB + 1), dict(sub=SUB + 2, out_sub=None)):
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg, kw


def test_a_sub_index_layout_that_cannot_be_held(lib):
    # blocks of 128 KiB have two chunks of 64 Ki symbols: 2^30 + 1 of them are more than 2^31 - 1 rows of chunks
    nb, bs = (1 << 30) + 1, 128 * 1024
    kw = dict(raw_size=nb * bs, blocksize=bs, nblocks=nb, cap=1)
    for subs in (dict(), dict(sub=None), dict(out_sub=None)):
        rc, msg = scatter(lib, **kw, **subs)
        assert rc == HUFE_ARGUMENT and "rows of chunks" in msg, subs
    rc, msg = scatter(lib, sub=None, out_sub=None, **kw)                 # without a sub-index nothing has to hold one
    assert rc == HUFE_ARGUMENT and "rows of chunks" not in msg
    rc, msg = scatter(lib, raw_size=(1 << 31) * bs, blocksize=bs, nblocks=1 << 31, cap=1)
    assert rc == HUFE_ARGUMENT and "(raw_size, blocksize)" in msg        # (more than 2^31 - 1 blocks: the layout check)


def test_out_of_place(lib):
    index_bytes, n = 6 * 8, 10 * 64
    for kw in (dict(out=STREAM + 996), dict(out=INDEX + 4 - 4000 + index_bytes - 4), dict(out=SRC + n - 4),
               dict(out_index=STREAM + 992), dict(out_index=INDEX + 8), dict(out_index=SRC), dict(out_index=OUT + 3992),
               dict(out_sub=SUB + 8), dict(out_sub=STREAM), dict(out_sub=OUT), dict(result=OUT + 8), dict(result=OUT_INDEX + 40),
               dict(result=OUT_SUB)):
        rc, msg = scatter(lib, **kw)
        assert rc == HUFE_ARGUMENT and "overlap" in msg, kw
    # touching is not overlapping, and with FILL d_src is no buffer of the call
    for kw in (dict(out=STREAM + 1000), dict(out=SRC + n), dict(out=SRC, flags=FILL), dict(result=OUT + 4000)):
        rc, msg = scatter(lib, **kw)
        assert "needs a context" in msg, kw


def test_touched_bound_against_a_brute_force_count(lib):
    rng = np.random.default_rng(5)
    bound = lib.hufgpu_scatter_touched_bound
    for bs in (1, 2, 3, 7, 16):
        for n in (1, 5, 16, 33, 100):
            nb = -(-n // bs)
            for max_len in (0, 1, 2, bs - 1, bs, bs + 1, 2 * bs, 2 * bs + 1, 40):
                if max_len < 0:
                    continue
                for nrec in (0, 1, 2, 5):
                    b = bound(nb, bs, nrec, max_len)
                    assert b == model.touched_bound(nb, bs, nrec, max_len), (nb, bs, nrec, max_len)
                    worst = 0
                    for _ in range(20):
                        pos = rng.integers(0, n + 2, nrec)
                        worst = max(worst, len(model.touched_blocks(n, bs, pos, None, max_len)))
                    if nrec == 1:        # every start of one record: the bound is reached where the data has room, never passed
                        worst = max(len(model.touched_blocks(n, bs, [p], None, max_len)) for p in range(n + 1))
                        if max_len and n >= max_len + bs:
                            assert worst == b, (n, bs, max_len, worst, b)
                    assert worst <= b, (n, bs, nrec, max_len, worst, b)
    assert bound(10, 0, 5, 100) == 1 and bound(0, 4096, 5, 100) == 0 and bound(7, 4096, 1 << 62, 1 << 31) == 7


# ---- the Python layer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec_class():
    from libhuffman_amd.codec import GpuCodec
    return GpuCodec


@pytest.fixture()
def bare(codec_class):
    """a GpuCodec without a context: what raises before the first device call needs none"""
    return codec_class.__new__(codec_class)


def redact(bare, pattern, **kw):
    return bare.redact(None, 0, None, 0, None, 100, 10, pattern, max_matches=4, **kw)


def test_redact_refuses_patterns_without_one_match_length(bare, codec_class):
    G = codec_class
    for pattern, word in (([b"a", G.Opt(b"b"), b"c"], "Opt / Rep"), ([G.Rep(b"0123456789", 1, 3)], "Opt / Rep"),
                          (G.regex(rb"colou?r"), "Opt / Rep"), (G.AnyOf(b"GET", b"POST"), "lengths [3, 4]"),
                          (G.egrep(rb"^ab"), "Expr")):
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            redact(bare, pattern)
        assert "lines=True" in str(e.value)
    with pytest.raises(ValueError, match="max_len"):
        redact(bare, b"abc", lines=True)


def test_scatter_validates_data_and_fill(codec_class):
    import torch
    src = codec_class._scatter_source
    slots = torch.zeros((5, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="exactly one"):
        src(None, None, 5, 8)
    with pytest.raises(ValueError, match="exactly one"):
        src(slots, 0x2A, 5, 8)
    for bad in (256, -1, b"", b"ab"):
        with pytest.raises(ValueError, match="fill"):
            src(None, bad, 5, 8)
    assert src(None, b"*", 5, 8) == (None, 0x2A, 8, 0) and src(None, 0, 5, None) == (None, 0, None, 0)
    with pytest.raises(TypeError):
        src(slots.to(torch.int32), None, 5, 8)
    with pytest.raises(TypeError):
        src(np.zeros((5, 8), np.uint8), None, 5, 8)
    with pytest.raises(ValueError, match="max_len"):
        src(torch.zeros(40, dtype=torch.uint8), None, 5, None)
    with pytest.raises(ValueError, match="nrecords x max_len"):
        src(torch.zeros(41, dtype=torch.uint8), None, 5, 8)
    with pytest.raises(ValueError, match="one slot a record"):
        src(slots, None, 4, 8)
    with pytest.raises(ValueError, match="fewer than max_len"):
        src(slots, None, 5, 9)
    with pytest.raises(ValueError, match="contiguous"):
        src(torch.zeros((8, 5), dtype=torch.uint8).t(), None, 5, 8)
    d, f, max_len, stride = src(torch.zeros(40, dtype=torch.uint8), None, 5, 8)
    assert tuple(d.shape) == (5, 8) and f is None and max_len == 8 and stride == 8
    d, f, max_len, stride = src(torch.zeros((5, 32), dtype=torch.uint8)[:, :12], None, 5, None)
    assert max_len == 12 and stride == 32
    d, f, max_len, stride = src(torch.zeros((5, 32), dtype=torch.uint8)[:, :12], None, 5, 7)
    assert max_len == 7 and stride == 32

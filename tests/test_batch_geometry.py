"""hufgpu_batch_geometry and the argument checks of the batch calls (no GPU needed).

The geometry of a batch is plain arithmetic over the single-item helpers: its block count and output bound are sums
of hufgpu_block_count and hufgpu_encode_bound, its row blocksize is the longest block, and its sub-index has one row
of that size per block.
"""
import ctypes as C

import numpy as np
import pytest

from libhuffman_amd import _native

HUFE_OK, HUFE_ARGUMENT = 0, 2
GROUP, TILE, NSYM = 32, 2048, 256


@pytest.fixture(scope="module")
def lib():
    return _native.load()


def u64s(values):
    values = [int(v) for v in values]
    return (C.c_uint64 * max(1, len(values)))(*values)


def geometry(lib, lens, bs):
    out = [C.c_uint64(0) for _ in range(4)]
    rc = lib.hufgpu_batch_geometry(len(lens), u64s(lens), bs, *[C.byref(o) for o in out])
    assert rc == HUFE_OK
    return tuple(int(o.value) for o in out)


def expected(lib, lens, bs):
    nb = sum(int(lib.hufgpu_block_count(n, bs)) for n in lens)
    bound = sum(int(lib.hufgpu_encode_bound(n, bs)) for n in lens)
    longest = max(lens, default=0)
    rbs = min(bs, longest) if bs else longest
    if nb == 0:
        sub = 0
    else:
        tpb = -(-rbs // TILE)
        gpb = (-(-rbs // GROUP) + 7) & ~7
        sub = nb * tpb * 8 + nb * gpb * 2 + nb * NSYM
    return nb, rbs, bound, sub


def item_lists():
    rng = np.random.default_rng(7)
    lists = [[], [0], [0, 0, 0], [1], [5, 0, 7]]
    for bs in (4096, 65536, 131072):
        lists.append([bs - 1, bs, bs + 1, 0, 3 * bs + 17])
    for _ in range(20):
        k = int(rng.integers(1, 200))
        lens = rng.integers(0, 300_000, k).tolist()
        zero_at = rng.integers(0, k, max(1, k // 5))
        for z in zero_at:
            lens[int(z)] = 0
        lists.append(lens)
    return lists


@pytest.mark.parametrize("bs", [0, 1, 4096, 16384, 65536, 131072, 1 << 21, 1 << 22])
def test_geometry_is_the_sum_of_single_items(lib, bs):
    for lens in item_lists():
        assert geometry(lib, lens, bs) == expected(lib, lens, bs), (bs, lens[:8])


def test_geometry_at_blocksize_edges(lib):
    for bs in (4096, 65536, 121392, 131072):
        for n in (bs - 1, bs, bs + 1):
            nb, rbs, bound, sub = geometry(lib, [n, 3], bs)
            assert nb == -(-n // bs) + 1
            assert rbs == min(n, bs)
            assert bound == int(lib.hufgpu_encode_bound(n, bs)) + int(lib.hufgpu_encode_bound(3, bs))
            assert (nb, rbs, bound, sub) == expected(lib, [n, 3], bs)


def test_geometry_row_blocksize_rule(lib):
    assert geometry(lib, [], 4096) == (0, 0, 0, 0)
    assert geometry(lib, [0, 0], 4096) == (0, 0, 32, 0)          # an empty item: no block, hufgpu_encode_bound(0) = 16
    assert geometry(lib, [10, 20000, 7], 0)[:2] == (3, 20000)    # blocksize 0: every item is one block
    assert geometry(lib, [10, 20000, 7], 4096)[:2] == (1 + 5 + 1, 4096)
    assert geometry(lib, [10, 100], 4096)[:2] == (2, 100)         # no block is longer than the longest item


def test_geometry_single_item_matches_sub_index_bytes(lib):
    for n, bs in ((1, 4096), (4097, 4096), (100_000, 65536), (300_000, 0), (131072, 131072)):
        nb, rbs, bound, sub = geometry(lib, [n], bs)
        assert nb == int(lib.hufgpu_block_count(n, bs))
        assert bound == int(lib.hufgpu_encode_bound(n, bs))
        # rows are sized by the longest block, not by the blocksize
        assert rbs == min(n, bs or n)
        assert sub == int(lib.hufgpu_sub_index_bytes(n, rbs))


def test_geometry_outputs_are_optional_and_lengths_required(lib):
    nb = C.c_uint64(0)
    assert lib.hufgpu_batch_geometry(2, u64s([5, 9000]), 4096, C.byref(nb), None, None, None) == HUFE_OK
    assert nb.value == 4
    assert lib.hufgpu_batch_geometry(3, None, 4096, C.byref(nb), None, None, None) == HUFE_ARGUMENT
    assert lib.hufgpu_batch_geometry(0, None, 4096, C.byref(nb), None, None, None) == HUFE_OK
    assert nb.value == 0


def test_batch_calls_need_a_context(lib):
    lens = u64s([10, 20])
    offs = (C.c_uint64 * 3)()
    assert lib.hufgpu_encode_batch(None, None, 2, lens, 4096, None, 0, None, None, None, offs, None) == HUFE_ARGUMENT
    errs = (C.c_int32 * 2)()
    raws = (C.c_uint64 * 2)()
    ib, oo = u64s([0, 1, 2]), u64s([0, 10, 30])
    assert lib.hufgpu_decode_batch(None, None, 100, None, 2, ib, oo, None, 0, None, 0, errs, raws, None) == HUFE_ARGUMENT

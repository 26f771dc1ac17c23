"""GPU test of the three routes that serve straight from the sub-index - decode_ranges(..., tiles=True), gather and
find_bytes - side by side on ONE stream and ONE damaged sub-index: all three take a tile through the same checked item
(kernels/sub_tile.hpp), so a tile one of them refuses must be refused by all.

Bit-exact, no tolerance.  Nothing is asserted here that test_gpu_range_tiles.py, test_gpu_gather.py and test_gpu_find.py
(test_foreign_sub_index / test_sub_index_abuse, and their damage tests) do not assert for their own route; the helpers
are theirs.

The stream: zipf255 in blocks of 6 144 bytes - three tiles a block: a first, a middle and a last one - and
2 x 6 144 + 2 079 bytes, so the last block has two tiles and its last group 31 symbols.  The damage is always in block 1
(offsets from tests/sub_index_ref.py), one entry - or two that cancel - per case:
  a      tile_bits[0] = 1: the block's first tile does not start at payload bit 0                       tile 0 fails
  b      group_bits[g] += 1, group_bits[g + 1] -= 1 in the middle tile: the tile's sum, and with it
         check (c), still holds - only the groups' own decode, check (b), sees it                       tile 1 fails
  c      tile_bits[1] += 1: tile 0 does not end where tile 1 is said to start, nor tile 1 where tile 2  tiles 0, 1 fail
  wild   one group_bits entry of the last tile = 0xffff: more than 32 codes can have                    tile 2 fails
"""
import numpy as np
import pytest

import sub_index_ref
from find_model import find_model
from test_gpu_find import find, only_this_block, value_sets
from test_gpu_gather import check_good, check_guards, cut, gather
from test_gpu_range_tiles import call, encode, model
from test_gpu_ranges import check_all_good, slots_for

pytestmark = pytest.mark.gpu

TILE, GROUP = 2048, 32
OK, RW = 0, 3
BS = 6144
N = 2 * BS + 2079
LN = 100                                                # bytes a record, a range


def set_tile0(tiles, groups, lay):
    tiles[1 * lay.tpb + 0] = 1


def shift_a_bit(tiles, groups, lay):
    g = 1 * lay.gpb + 64 + 10
    assert groups[g + 1] >= 1
    groups[g] += 1
    groups[g + 1] -= 1


def move_tile1(tiles, groups, lay):
    tiles[1 * lay.tpb + 1] += 1


def wild_group(tiles, groups, lay):
    groups[1 * lay.gpb + 128 + 5] = 0xffff


# name -> (the change, the tiles of block 1 that fail their checks)
DAMAGE = {"a": (set_tile0, {0}), "b": (shift_a_bit, {1}), "c": (move_tile1, {0, 1}), "wild": (wild_group, {2})}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def enc(torch_mod, codec):
    """one encode for the whole module; the tests never change it"""
    e = encode(torch_mod, codec, "zipf255", N, BS)
    assert e.nb == 3 and list(e.block_lens) == [BS, BS, 2079] and 2079 % TILE == 31
    return e


def damaged_sub(torch, enc, name):
    lay = sub_index_ref.layout(enc.n, enc.bs)
    assert (lay.nb, lay.tpb) == (3, 3)
    raw = enc.sub.cpu().numpy().copy()
    tiles, groups, _ = sub_index_ref.views(raw.view(np.uint8), lay)
    DAMAGE[name][0](tiles, groups, lay)
    sub = torch.from_numpy(raw).cuda()
    assert not torch.equal(sub, enc.sub)
    return sub


# records: in every tile of block 1, across its tile and block borders, in the other blocks, cut by the end of the data
POS = [BS + 100, BS + TILE + 300, BS + 2 * TILE + 200, BS + TILE - 50, BS + 2 * TILE - 50, BS - 50, 2 * BS - 50,
       10, TILE + 5, 2 * TILE + 50, 2 * BS + 7, 2 * BS + TILE - 50, N - 31]


def tiles_in_block_1(p, c):
    """the tiles of block 1 that bytes [p, p + c) lie in"""
    lo, hi = max(p, BS), min(p + c, 2 * BS)
    return set(range((lo - BS) // TILE, (hi - 1 - BS) // TILE + 1)) if lo < hi else set()


@pytest.mark.parametrize("name", list(DAMAGE))
def test_a_damaged_tile_is_refused_by_every_route(torch_mod, codec, enc, name):
    torch = torch_mod
    sub = damaged_sub(torch, enc, name)
    failing = DAMAGE[name][1]

    # find_bytes: block 1 is not served, the other blocks' counts and positions are numpy's
    values = value_sets(enc.data)["frequent"] + [41, 0]
    cap = int(find_model(enc.data, values, enc.bs)[2][0]) + 3
    only_this_block(enc, find(torch, codec, enc, values, cap, sub=sub), values, cap, 1)

    # gather: a record with bytes in a failing tile is not served; every other record is exact
    got, errs, raws, stride = gather(torch, codec, enc, POS, LN, sub=sub)
    check_guards(enc, got, POS, LN, stride)
    hit = [i for i, p in enumerate(POS) if tiles_in_block_1(p, cut(enc, p, LN)) & failing]
    assert hit and len(hit) < len(POS)
    for i, p in enumerate(POS):
        assert raws[i] == cut(enc, p, LN) and errs[i] == (RW if i in hit else OK), (name, i, p, errs[i])
    check_good(enc, got, errs, raws, POS, LN, stride, only=[i for i in range(len(POS)) if i not in hit])

    # decode_ranges with the flag: a range that cuts block 1 in a failing tile, one in block 0 - the block fails over
    # to the staged route and the bytes are exact
    p = BS + min(failing) * TILE + 100
    ranges = [(p, p + LN), (TILE + 5, TILE + 5 + LN)]
    oo = slots_for(ranges, enc.n)
    _, _, tiles, items = model(enc, ranges, oo)
    assert (tiles, items) == (2, 2)
    got = call(torch, codec, enc, ranges, oo, True, sub_index=sub)
    cnt = codec.ranges_counters()
    check_all_good(enc, ranges, got[0], got[1], got[2], oo)
    assert cnt[2:5] == (0, items, 1), (name, cnt)


def test_the_own_sub_index_serves_all_of_it(torch_mod, codec, enc):
    """the same calls with the encoder's sub-index: nothing is refused (the damage above is what is refused)"""
    torch = torch_mod
    values = value_sets(enc.data)["frequent"] + [41, 0]
    cap = int(find_model(enc.data, values, enc.bs)[2][0]) + 3
    res = find(torch, codec, enc, values, cap)
    assert not res[2].any()
    got, errs, raws, stride = gather(torch, codec, enc, POS, LN)
    check_good(enc, got, errs, raws, POS, LN, stride)
    ranges = [(BS + 100, BS + 100 + LN), (TILE + 5, TILE + 5 + LN)]
    oo = slots_for(ranges, enc.n)
    got = call(torch, codec, enc, ranges, oo, True)
    check_all_good(enc, ranges, got[0], got[1], got[2], oo)
    assert codec.ranges_counters()[2:5] == (2, 2, 0)

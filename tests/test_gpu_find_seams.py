"""The seam kernels of the search family (libhuffman_amd/csrc/kernels/find.hpp) share ONE walk over the layout's tiles: the same
literal goes through every route that ends in one of them - the literal call, the class call with classes of one value, the
any-of call with that one alternative and with a second one of two bytes, and find_records(line_numbers=True), the select
call - on inputs whose matches cross every kind of seam, once with all blocks served and once with a middle block that is not.
Every route must give what its model gives, and the first three must give the same.  (The lengths of an AnyOf sum to at most
64, so a literal of 64 bytes leaves no room for a second alternative: there the route with two alternatives gets the
literal's first 62 bytes, still a candidate that crosses 21 blocks of 3 bytes.)"""
import numpy as np
import pytest

from find_any_model import find_any_model, find_any_records_model
from find_classes_model import find_classes_model
from find_pattern_model import find_pattern_model
from find_select_model import find_select_model
from find_support import OK, RW, TILE, AnyOf, check, codec, damaged, encode, numbered, payload_start, psearch, torch_mod

pytestmark = pytest.mark.gpu

A, B = 7, 207               # the data's two byte values (codes 00 and 01: a 1 at an even payload bit leaves the tree);
DELIMS = bytes([B])         # the literal is a run of A, so B may end the records
LENGTHS = [2, 4, 64]
# shape -> (blocksize, blocks, the block that is damaged and the payload bit that is, the starts of the planted runs of 64 A,
# the starts of the planted B A)
SHAPES = {
    # every block is a tile shorter than 64 - 1: a candidate of 64 bytes crosses 22 of them
    "200x3": (3, 200, 100, 0, [10, 250, 400], [5, 500]),
    # tile seams at 2048 and 4096, a last tile of 3 bytes, then the block seam: runs of A over each of them in the blocks 0, 1
    # and 3 (the last one reaches into the damaged block), B A over each of them in and in front of block 4
    "5x4099": (4099, 5, 2, 2 * 3000, [b * 4099 + TILE - 32 for b in (0, 1, 3)] + [2 * TILE - 1, 4099 + 4098],
               [4 * 4099 + TILE - 1, 4 * 4099 + 2 * TILE - 1, 4 * 4099 - 1]),
}


@pytest.fixture(scope="module")
def inputs(torch_mod, codec):
    """(shape, damaged) -> the encoded input; the data is random over A and B with runs of exactly 64 A planted"""
    made = {}
    for shape, (bs, nb, bad, bit, runs, pairs) in SHAPES.items():
        enc = encode(torch_mod, codec, planted_data(shape), bs)
        made[shape, False] = enc
        made[shape, True] = damaged(enc, payload_start(enc, bad) + bit // 8, 0x80 >> (bit % 8))
    return made


def planted_data(shape):
    bs, nb, _, _, runs, pairs = SHAPES[shape]
    data = (np.random.default_rng(nb).integers(0, 2, bs * nb) * (B - A) + A).astype(np.uint8)
    for s in runs:
        data[s - 1], data[s + 64] = B, B
        data[s:s + 64] = A
    for s in pairs:
        data[s], data[s + 1] = B, A
    return data


def seams(n, bs):
    """kind of seam -> the positions at which a tile of the layout starts behind another one"""
    kinds = {}
    for b0 in range(0, n, bs):
        blen = min(bs, n - b0)
        if b0:
            kinds.setdefault("block", []).append(b0)
        for t in range(TILE, blen, TILE):
            kinds.setdefault("tile" if blen - t >= TILE else "short last tile", []).append(b0 + t)
    return kinds


def crossed(pos, length, n, bs):
    """the model's matches cross a seam of every kind that the layout has"""
    for kind, at in seams(n, bs).items():
        assert any(np.any((pos < s) & (pos + length > s)) for s in at), ("no match of", length, "bytes crosses a seam of kind", kind)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("damage", [False, True], ids=["served", "damaged"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_literal_through_every_route(torch_mod, codec, inputs, shape, damage, length):
    torch = torch_mod
    enc = inputs[shape, damage]
    bs, nb, bad = SHAPES[shape][:3]
    n = bs * nb
    lit = bytes([A]) * length
    one = lit[:62]                                              # the literal, as long as an AnyOf has room for it next to ...
    two = [one, bytes([B, A])]                                  # ... the second alternative, of length 2
    status = np.array([RW if damage and b == bad else OK for b in range(nb)], np.int32)
    served = status == OK
    what = (shape, damage, length)

    # the models' answers first: they have matches over every kind of seam, with the damaged block as without it
    pos, _, totals = find_pattern_model(enc.data, lit, bs, n, served=served)
    total = int(totals[0])
    assert 0 < total < n, (what, total)
    crossed(pos, length, n, bs)
    pos1 = find_pattern_model(enc.data, one, bs, n, served=served)[0]
    crossed(pos1, len(one), n, bs)
    pos2, _, totals2 = find_any_model(enc.data, two, bs, n, served=served)
    assert int(totals2[0]) > pos1.size, what
    crossed(pos2[~np.isin(pos2, pos1)], 2, n, bs)                # ... the second alternative's own matches too
    recs = int(find_select_model(enc.data, [lit], DELIMS, bs, n, served=served)[3][0])
    assert recs > 0, what

    cap = total + 5
    routes = [(lit, find_pattern_model(enc.data, lit, bs, cap, served=served)),
              ([bytes([A])] * length, find_classes_model(enc.data, [bytes([A])] * length, bs, cap, served=served)),
              (AnyOf(lit), find_any_model(enc.data, [lit], bs, cap, served=served))]
    answers = []
    for pattern, want in routes:
        res = psearch(torch, codec, enc, pattern, cap)
        assert np.array_equal(res[2], status), (what, pattern, np.flatnonzero(res[2] != status)[:8])
        check(res, want, cap, (what, pattern))
        answers.append(res)
    for res in answers[1:]:                                     # seam identity: one walk, three callers
        assert all(np.array_equal(x, y) for x, y in zip(res, answers[0])), what

    cap2 = int(totals2[0]) + 5
    res = psearch(torch, codec, enc, AnyOf(*two), cap2)
    assert np.array_equal(res[2], status), (what, "two alternatives")
    check(res, find_any_model(enc.data, two, bs, cap2, served=served), cap2, (what, "two alternatives"))

    rcap = recs + 5
    res = numbered(torch, codec, enc, lit, DELIMS, rcap)
    assert np.array_equal(res[3], status), (what, "records")
    want = find_select_model(enc.data, [lit], DELIMS, bs, rcap, served=served)
    assert all(np.array_equal(x, y) for x, y in zip(want[:4], find_any_records_model(enc.data, [lit], DELIMS, bs, rcap, served=served))), what
    check(res, want, rcap, (what, "records"))

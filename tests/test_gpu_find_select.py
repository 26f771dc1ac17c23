"""GPU tests of hufgpu_find_records_select (GpuCodec.find_records / count_records / grep with `invert` and `line_numbers`):
grep -v and grep -n - the non-empty records WITHOUT a match of any alternative, and for either answer the number of
delimiters in front of each record - from the two masks of the one walk, enqueue-only.

Bit-exact, no tolerance.  Expected values come from tests/find_select_model.py (itself checked against `re` / split over
`bytes` in tests/test_find_select_args.py).  As in tests/test_gpu_find.py every output buffer - starts, lengths and numbers -
has guard words in front and behind and is filled with the guard first: the words beyond totals[1] must still hold it.  The
four shapes are those of tests/test_gpu_find_classes.py: five blocks of 4 099 bytes (tiles of 2 048, 2 048 and 3 symbols),
300 blocks of 64 bytes (300 tiles: two scan groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes (three chunks).
"""
import re

import numpy as np
import pytest

from find_any_model import find_any_records_model
from find_model import find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from find_select_model import NO_UNKNOWN, find_select_model
from find_support import (CHUNK, FOUR_SHAPES, GUARD32, GUARD64, LEAD, NL, OK, RW, SEAMS, TAIL, TILE, AnyOf, base_without, check, codec,
                          damaged, encode, exact_answer, mixed_blocks, pattern_below_255, payload_start, planted, rsearch, runs_input,
                          same_arrays, select, torch_mod, with_delimiters)
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu


# ---- the checks --------------------------------------------------------------------------------------------------------------
def both_answers(torch, codec, enc, alts, delims=b"\n", room=5, max_len=0, what="", sub=None, all_served=True):
    """the plain and the inverted answer with their numbers, each equal to the model's for the blocks with status 0; returns
    (the model's plain answer, its inverted one, the statuses) at a cap that holds every record"""
    out = []
    for invert in (False, True):
        full, _, errs = exact_answer(lambda cap: select(torch, codec, enc, alts, delims, cap, max_len, invert=invert, sub=sub),
                              lambda cap, served: find_select_model(enc.data, alts, delims, enc.bs, cap, max_len, served, invert),
                              enc.n, room=room, what=(what, invert), all_served=all_served,
                              probe=lambda: select(torch, codec, enc, alts, delims, 0, invert=invert, numbers=False, sub=sub))
        out.append(full)
    return out[0], out[1], errs


def nonempty_records(data, delims=b"\n"):
    """[(s, e)] of the data's non-empty pieces, from bytes.split"""
    out, s = [], 0
    for piece in (bytes(data).split(bytes(delims)) if delims else [bytes(data)]):
        if piece:
            out.append((s, s + len(piece)))
        s += len(piece) + 1
    return out


def partition(plain, inverted, data, delims=b"\n"):
    """plain and inverted are disjoint and together every non-empty record; the totals sum accordingly"""
    a, b = set(plain[0].tolist()), set(inverted[0].tolist())
    assert not a & b
    recs = nonempty_records(data, delims)
    got = sorted(zip(plain[0].tolist() + inverted[0].tolist(), (plain[0] + plain[1]).tolist() + (inverted[0] + inverted[1]).tolist()))
    assert got == recs
    assert int(plain[3][0]) + int(inverted[3][0]) == len(recs)


# ---- 1: the identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_select_0_without_numbers_is_find_records_any(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    words = [pattern_below_255(5, 301), pattern_below_255(2, 302)]
    data = with_delimiters(base_without(n, 81), [p - 1 for p in SEAMS[shape]] + [n - 1])
    for i, s in enumerate(SEAMS[shape]):                    # (every third seam's record holds neither word)
        data = planted(data, words[i % 2], [s + 2 + i % 3] if i % 3 and s + 10 < n else [])
    enc = encode(torch, codec, data, bs)
    alts = [[bytes([v]) for v in w] for w in words]
    for cap, max_len, counts in ((n, 0, True), (3, 7, False), (0, 0, True)):
        got = select(torch, codec, enc, alts, b"\n", cap, max_len, numbers=False, counts=counts)
        assert got[5] is None
        older = rsearch(torch, codec, enc, AnyOf(*alts), b"\n", cap, max_len, counts=counts)
        assert same_arrays(got[:5], older), (shape, cap, "differs from find_records_any")
        check(got[:5], find_any_records_model(data, alts, b"\n", bs, cap, max_len), cap, (shape, cap))
        one = select(torch, codec, enc, alts[:1], b"\n", cap, max_len, numbers=False, counts=counts)
        assert same_arrays(one[:5], rsearch(torch, codec, enc, words[0], b"\n", cap, max_len, counts=counts)), (shape, "find_records")
        assert same_arrays(one[:5], rsearch(torch, codec, enc, alts[0], b"\n", cap, max_len, counts=counts)), (shape, "find_records_classes")
        assert int(one[2][0]) > 0


# ---- 2: invert at the seams, 6: numbers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_records_at_the_seams(torch_mod, codec, shape):
    """a record start at every seam p of the shape, four ways that rotate through the seams: one delimiter at p - 1; two in a
    row in front of the seam (p - 2, p - 1); two in a row behind it (p, p + 1: the record over the seam ends AT it and the
    next starts at p + 2); one on each side (p - 1, p: an empty record at the seam).  The first record has no delimiter in
    front; the last has one behind it in every other rotation.  A word lies in every other seam record, so both answers
    have records at the seams; the numbers come with both, empty records in front included."""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    word = pattern_below_255(2 if shape == "200x3" else 4, 310)
    ways = [(-1,), (-2, -1), (0, 1), (-1, 0)]
    first = [0, 0, 2, 1]                                   # where the seam's record starts, from p
    for rot in range(4):
        nl, at, seam_starts = [], [], []
        for k, p in enumerate(SEAMS[shape]):
            w = (k + rot) % 4
            nl += [p + o for o in ways[w] if p + o < n]
            s = p + first[w]
            if s < n:
                seam_starts.append(s)
                if k % 2 and s + 3 + len(word) < n:
                    at.append(s + 3)
        data = planted(with_delimiters(base_without(n, 82 + rot), nl + ([n - 1] if rot % 2 else [])), word, at)
        assert data[0] != NL and (data[n - 1] == NL) == bool(rot % 2 or n - 1 in nl)
        enc = encode(torch, codec, data, bs)
        plain, inverted, _ = both_answers(torch, codec, enc, [word], what=(shape, rot))
        partition(plain, inverted, data)
        a, b = set(plain[0].tolist()), set(inverted[0].tolist())
        assert a and b and 0 in a | b
        assert set(seam_starts) <= a | b, (shape, rot, sorted(set(seam_starts) - (a | b)))
        assert {s - 3 for s in at} <= a and set(seam_starts) - {s - 3 for s in at} <= b
        for ans in (plain, inverted):                      # the numbers are the indices in the split, empty pieces counted
            assert ans[4].tolist() == [bytes(data[:s]).count(b"\n") for s in ans[0].tolist()]
        assert inverted[4].size > np.unique(inverted[4]).size - 1 and int(inverted[4].max()) >= len(nonempty_records(data)) - 1


@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_the_only_match_three_tiles_on(torch_mod, codec, shape):
    """a record that starts in one tile and has its only match three tiles on is absent from the inverted answer (mark sets the
    bit in the START's tile); the same record without the match is present"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    tile = min(bs or TILE, TILE)
    s0 = {"5x4099": 4099 + 1000, "300x64": 254 * 64 + 9, "3chunks": CHUNK - TILE + 77}[shape]
    hit = s0 + 3 * tile + tile // 2
    end = hit + tile
    word = pattern_below_255(5, 320)
    base = with_delimiters(base_without(n, 86), [s0 - 1, end, end + 50])
    assert s0 // tile + 3 <= hit // tile and not (base[s0:end] == NL).any()
    for with_match in (True, False):
        data = planted(base, word, [hit] if with_match else [])
        enc = encode(torch, codec, data, bs)
        plain, inverted, _ = both_answers(torch, codec, enc, [word], what=(shape, with_match))
        partition(plain, inverted, data)
        assert (s0 in plain[0].tolist()) == with_match and (s0 in inverted[0].tolist()) == (not with_match)
        assert {0, end + 1, end + 51} <= set(inverted[0].tolist())


# ---- 3: the partition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_the_partition_on_dense_random_data(torch_mod, codec, shape):
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(78)
    letters = np.frombuffer(b"abc", np.uint8)
    data = rng.choice(np.frombuffer(b"abc\n", np.uint8), n, p=[0.31, 0.31, 0.31, 0.07]).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    sizes = []
    for trial in range(6):
        alts = [[bytes(rng.choice(letters, int(rng.integers(1, 3)), replace=False).astype(np.uint8)) for _ in range(int(rng.integers(2, 7)))]
                for _ in range(int(rng.integers(1, 7)))]
        plain, inverted, _ = both_answers(torch_mod, codec, enc, alts, what=(shape, trial, alts))
        partition(plain, inverted, data)
        sizes.append((int(plain[3][0]), int(inverted[3][0])))
    assert any(a and b for a, b in sizes), sizes


# ---- 4: one record over all blocks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_one_record_over_all_blocks(torch_mod, codec, shape):
    """the empty delimiter set and a delimiter that never occurs: ONE record, (0, n).  It is the inverted answer when no match
    lies in it, and absent from it with a match in every tile and with a single match in the last tile"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    tile = min(bs or TILE, TILE)
    word = pattern_below_255(2, 330)
    base = base_without(n, 87)
    every = [t for t in range(0, n - 1, tile) if (t % (bs or n)) + 2 <= min(bs or n, n - t // (bs or n) * (bs or n))]
    for plants, matched in (([], False), (every, True), ([n - 2], True)):
        data = planted(base, word, plants)
        enc = encode(torch, codec, data, bs)
        for delims in (b"", b"\n"):
            plain, inverted, _ = both_answers(torch, codec, enc, [word], delims, what=(shape, len(plants), delims))
            one, none = (plain, inverted) if matched else (inverted, plain)
            assert one[0].tolist() == [0] and one[1].tolist() == [n] and one[4].tolist() == [0] and one[2].tolist() == [1] + [0] * (enc.nb - 1)
            assert none[3].tolist() == [0, 0, 0, 0]


# ---- 5: one-symbol blocks ----------------------------------------------------------------------------------------------------
def test_one_symbol_blocks_of_delimiters(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    enc = encode(torch, codec, np.full(n, 41, np.uint8), bs)
    plain, inverted, _ = both_answers(torch, codec, enc, [b"("], b")", what="all delimiters")
    assert plain[3].tolist() == inverted[3].tolist() == [0, 0, 0, 0]
    plain, inverted, _ = both_answers(torch, codec, enc, [b"(*"], b"\n", what="one record of a leaf that is in no class")
    assert inverted[0].tolist() == [0] and inverted[1].tolist() == [n] and plain[3][0] == 0
    plain, inverted, _ = both_answers(torch, codec, enc, [[b")("] * 7], b"\n", what="... and in every class")
    assert plain[0].tolist() == [0] and inverted[3][0] == 0


@pytest.mark.parametrize("bs", [4096, 4099])
@pytest.mark.parametrize("leaf", [41, NL])
def test_one_symbol_and_ordinary_blocks_alternate(torch_mod, codec, bs, leaf):
    """blocks of one value - a delimiter: thousands of empty records; a non-delimiter that is in no class: part of one reported
    record - between ordinary blocks whose records run into and out of them"""
    torch = torch_mod
    data = mixed_blocks(bs, 6, 48)
    data[data == NL] = NL + 1
    for b in (0, 2, 4):
        data[b * bs:(b + 1) * bs] = leaf
    word = pattern_below_255(5, 340)
    data = with_delimiters(data, [bs + 50, bs + 51, 2 * bs - 20, 3 * bs, 3 * bs + 2047, 3 * bs + 2048, 4 * bs - 1, 5 * bs + 1, 6 * bs - 1])
    data = planted(data, word, [bs + 10, 3 * bs + 3000])
    assert [np.unique(data[o:o + bs]).size == 1 for o in range(0, data.size, bs)] == [True, False] * 3
    enc = encode(torch, codec, data, bs)
    plain, inverted, _ = both_answers(torch, codec, enc, [word], what=(bs, leaf))
    partition(plain, inverted, data)
    for ans in (plain, inverted):
        assert ans[4].tolist() == [bytes(data[:s]).count(b"\n") for s in ans[0].tolist()]
    if leaf == 41:
        assert plain[0].tolist() == [0, 3 * bs + 2049] and plain[1][0] == bs + 50       # out of block 0, which holds no match itself
        assert {bs + 52, 2 * bs - 19, 4 * bs, 5 * bs + 2} <= set(inverted[0].tolist())
        assert inverted[1][inverted[0].tolist().index(2 * bs - 19)] == bs + 19         # through all of block 2
    else:
        assert plain[0].tolist() == [bs, 3 * bs + 2049] and plain[4][0] == bs           # a block of empty records in front
        assert inverted[0].tolist() == [bs + 52, 2 * bs - 19, 3 * bs + 1, 5 * bs, 5 * bs + 2]


# ---- 6: the numbers ----------------------------------------------------------------------------------------------------------
def test_numbers_across_a_scan_group_edge(torch_mod, codec):
    """300 tiles: records that start on both sides of tile 256, with empty records in front; and the same call without
    d_rec_no gives the same starts and lengths"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["300x64"]
    edge = 256 * 64
    nl = [3, 4, 5, 64 * 100, 64 * 100 + 1, edge - 70, edge - 2, edge - 1, edge + 10, edge + 11, edge + 12, edge + 64, edge + 300, n - 1]
    word = pattern_below_255(3, 350)
    data = planted(with_delimiters(base_without(n, 88), nl), word, [edge - 60, edge + 2, edge + 100])
    enc = encode(torch, codec, data, bs)
    plain, inverted, _ = both_answers(torch, codec, enc, [word], what="edge")
    assert plain[0].tolist() == [edge - 69, edge, edge + 65] and plain[4].tolist() == [6, 8, 12]
    assert inverted[0].tolist() == [0, 6, 64 * 100 + 2, edge + 13, edge + 301] and inverted[4].tolist() == [0, 3, 5, 11, 13]
    for invert in (False, True):
        cap = 9
        with_no = select(torch, codec, enc, [word], b"\n", cap, invert=invert)
        without = select(torch, codec, enc, [word], b"\n", cap, invert=invert, numbers=False)
        assert without[5] is None and same_arrays(with_no[:5], without[:5])


# ---- 7: blocks that are not served -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """records into, out of and next to the block are absent from BOTH answers, all others present in one; numbers are exact in
    front of the block and unknown from the block behind it on; totals[2] is find_records_any's"""
    torch = torch_mod
    enc, delim, alts = runs_input(torch, codec)
    bs, n = enc.bs, enc.n
    plain, inverted, _ = both_answers(torch, codec, enc, alts, delim, what="undamaged")
    partition(plain, inverted, enc.data, delim)
    assert plain[0].size > 20 and inverted[0].size > 20
    recs = nonempty_records(enc.data, delim)
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        p, v, errs = both_answers(torch, codec, bad, alts, delim, what=(damage, b), all_served=False)
        assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
        assert int(p[3][2]) == int(v[3][2]) == 1 == int(rsearch(torch, codec, bad, AnyOf(*alts), delim, 0)[2][2])
        got = sorted(p[0].tolist() + v[0].tolist())
        assert got == [s for s, e in recs if not max(s - 1, 0) // bs <= b <= min(e, n - 1) // bs], (damage, b)
        assert set(p[0].tolist()) <= set(plain[0].tolist()) and set(v[0].tolist()) <= set(inverted[0].tolist())
        for ans in (p, v):
            front = ans[0] < b * bs
            assert front.any() == (b > 0) and (~front).any() == (b < 4)
            assert ans[4][front].tolist() == [bytes(enc.data[:s]).count(delim) for s in ans[0][front].tolist()]
            assert (ans[4][~front] == NO_UNKNOWN).all()


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    word = pattern_below_255(6, 360)
    data = planted(base_without(5 * bs + 1500, 89), word, [100, bs - 3, 2 * bs + 2045, 5 * bs + 1494])
    data = with_delimiters(data, np.arange(37, data.size, 601))
    enc = encode(torch, codec, data, bs)
    rng = np.random.default_rng(34)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    _, _, errs = both_answers(torch, codec, enc, [word, word[:2]], what="own")
    _, _, errs = both_answers(torch, codec, enc, [word, word[:2]], sub=other, max_len=9, what=sub, all_served=False)
    assert sub == "random" or errs.all()                # (a bit count of 0 cannot be that of 32 codewords)
    bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    both_answers(torch, codec, bad, [word], sub=other, what=(sub, "and a damaged block"), all_served=False)


# ---- 8: caps and lengths -----------------------------------------------------------------------------------------------------
def test_caps_and_lengths(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    word = pattern_below_255(5, 370)
    nl = [99, 2047, bs - 1, bs + 3000, 2 * bs + 4096, 3 * bs + 10, 4 * bs + 4000]
    data = planted(with_delimiters(base_without(n, 90), nl), word, [0, 2100, 2 * bs + 4097, n - 5])
    enc = encode(torch, codec, data, bs)
    for invert, lens in ((False, [99, 2050, 12, 98]), (True, [1947, 3000, 5194, 8088])):
        total = len(lens)
        assert find_select_model(data, [word], b"\n", bs, n, invert=invert)[1].tolist() == lens
        for cap in (0, 1, total - 1, total):
            for counts in (True, False):
                for numbers in (True, False):
                    res = select(torch, codec, enc, [word], b"\n", cap, invert=invert, numbers=numbers, counts=counts)
                    assert int(res[2][0]) == total and not res[3].any()
                    check(res, find_select_model(data, [word], b"\n", bs, cap, invert=invert), cap, (invert, cap, counts, numbers))
        for max_len in sorted({1, 0} | {m + d for m in lens for d in (-1, 0, 1)}):        # below, at and above every length
            for cap in (total, 2):
                res = select(torch, codec, enc, [word], b"\n", cap, max_len, invert=invert)
                check(res, find_select_model(data, [word], b"\n", bs, cap, max_len, invert=invert), cap, (invert, max_len, cap))
                if cap == total:
                    assert int(res[2][3]) == sum(l > max_len for l in lens) * bool(max_len)


# ---- 9: one context, call after call -----------------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """find_records, a select call with invert, find_pattern, a select call with numbers only, find_bytes, and the first two
    again, without a synchronise in between: each gives its own model's answer"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    word = pattern_below_255(6, 380)
    nl = [40, 1500, 2046, bs, 2 * bs + 2100, 2 * bs + 4090, 3 * bs + 3000]
    data = planted(with_delimiters(base_without(n, 91), nl), word, starts)
    enc = encode(torch, codec, data, bs)
    v = int(np.bincount(data).argmax())
    jobs = ["records", "invert", "pattern", "numbers", "bytes", "records", "invert"]

    def model(kind, cap):
        if kind == "records":
            return find_records_model(data, word, b"\n", bs, cap)
        if kind == "pattern":
            return find_pattern_model(data, word, bs, cap)
        if kind == "bytes":
            return find_model(data, [v], bs, cap)
        return find_select_model(data, [word], b"\n", bs, cap, invert=kind == "invert")

    bufs = []
    for kind in jobs:
        want = model(kind, n)
        total = int(want[3 if kind in ("invert", "numbers") else -1][0])
        assert total > 0, kind
        cap = total + 2
        bufs.append((cap, [torch.full((LEAD + cap + TAIL,), g, dtype=t, device="cuda")
                           for g, t in ((GUARD64, torch.int64), (GUARD32, torch.int32), (GUARD64, torch.int64))]))
    torch.cuda.synchronize()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    res = []
    for kind, (cap, (pbuf, lbuf, nbuf)) in zip(jobs, bufs):
        out = (pbuf[LEAD:LEAD + cap], lbuf[LEAD:LEAD + cap], nbuf[LEAD:LEAD + cap])
        if kind == "records":
            res.append(codec.find_records(*args, word, b"\n", max_records=cap, block_counts=True, out=out[:2]))
        elif kind == "invert":
            res.append(codec.find_records(*args, word, b"\n", max_records=cap, block_counts=True, out=out, invert=True, line_numbers=True))
        elif kind == "numbers":
            res.append(codec.find_records(*args, word, b"\n", max_records=cap, block_counts=True, out=out, line_numbers=True))
        elif kind == "bytes":
            res.append(codec.find_bytes(*args, [v], max_positions=cap, block_counts=True, out=out[0]))
        else:
            res.append(codec.find_pattern(*args, word, max_positions=cap, block_counts=True, out=out[0]))
    torch.cuda.synchronize()
    host = []
    for kind, (cap, (pbuf, lbuf, nbuf)), r in zip(jobs, bufs, res):
        if kind in ("invert", "numbers"):
            assert len(r) == 6 and r[5].data_ptr() == nbuf[LEAD:].data_ptr()
            got = (pbuf.cpu().numpy(), lbuf.cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy(), r[4].cpu().numpy(), nbuf.cpu().numpy())
            check(got, model(kind, cap), cap, kind)
        elif kind == "records":
            assert len(r) == 5
            got = (pbuf.cpu().numpy(), lbuf.cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy(), r[4].cpu().numpy())
            check(got, model(kind, cap), cap, kind)
            assert (nbuf.cpu().numpy() == GUARD64).all()
        else:
            got = (pbuf.cpu().numpy(), r[1].cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy())
            check(got, model(kind, cap), cap, kind)
        host.append(got)
    assert same_arrays(host[0], host[5]) and same_arrays(host[1], host[6])
    assert same_arrays(host[3][:5], host[0])                # numbers only: the plain answer


# ---- 10: Python ----------------------------------------------------------------------------------------------------------------
def test_grep_invert_with_line_numbers(torch_mod, codec):
    """grep(AnyOf(b"DEBUG", b"heartbeat"), invert=True, line_numbers=True) without a synchronisation, against an `re` filter
    over data.split(b"\\n"): the numbers are the indices in that split"""
    torch = torch_mod
    n, bs = (1 << 18) + 1, 65536
    data = datagen.logtext(n)
    lines = bytes(data).split(b"\n")
    want = [(i, l) for i, l in enumerate(lines) if l and not re.search(rb"DEBUG|heartbeat", l)]
    assert 0 < len(want) < sum(1 for l in lines if l)
    enc = encode(torch, codec, data, bs)
    cap, width = len(want) + 5, 256
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    out = codec.grep(*args, AnyOf(b"DEBUG", b"heartbeat"), cap, width, invert=True, line_numbers=True)
    assert len(out) == 6
    rows, raws, gerrs, totals, block_errs, numbers = (x.cpu().numpy() for x in out)
    assert totals.tolist() == [len(want), len(want), 0, sum(len(l) > width for _, l in want)] and not block_errs.any() and not gerrs.any()
    assert not raws[len(want):].any() and (numbers[len(want):] == -1).all() and numbers.dtype == np.int64
    assert numbers[:len(want)].tolist() == [i for i, _ in want]
    for k, (_, line) in enumerate(want):
        assert raws[k] == min(len(line), width) and bytes(rows[k, :raws[k]]) == line[:width], k
    plain = codec.grep(*args, AnyOf(b"DEBUG", b"heartbeat"), cap, width)
    assert len(plain) == 5                                   # as it always was
    kept = [(i, l) for i, l in enumerate(lines) if re.search(rb"DEBUG|heartbeat", l)]
    assert plain[3].cpu().tolist()[:2] == [len(kept), min(len(kept), cap)]
    totals, errs, numbers = codec.count_records(*args, b"DEBUG", invert=True, line_numbers=True)
    assert totals.cpu().tolist() == [sum(1 for l in lines if l and b"DEBUG" not in l), 0, 0, 0] and numbers.numel() == 0
    totals, errs = codec.count_records(*args, [b"Dd", b"E", b"B", b"U", b"G"], invert=True)
    assert totals.cpu().tolist() == [sum(1 for l in lines if l and not re.search(rb"[Dd]EBUG", l)), 0, 0, 0]
    _, _, totals, _, _, numbers = codec.find_records(*args, b"ERROR", max_records=cap, line_numbers=True)
    kept = [i for i, l in enumerate(lines) if b"ERROR" in l]
    assert numbers.cpu().tolist()[:len(kept)] == kept and int(totals[0]) == len(kept) <= cap
    for bad in (b"", b"x" * 65, b"a\nb", AnyOf(), AnyOf(b"x", b"")):
        with pytest.raises(ValueError):
            codec.find_records(*args, bad, invert=True)
        with pytest.raises(ValueError):
            codec.grep(*args, bad, 4, 16, line_numbers=True)


# ---- 11: no blocks -------------------------------------------------------------------------------------------------------------
def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    nbuf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    for kw in (dict(invert=True), dict(line_numbers=True), dict(invert=True, line_numbers=True)):
        res = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, AnyOf(b"error", b"x"), max_records=4, block_counts=True,
                                 out=(buf, lbuf, nbuf), **kw)
        assert res[2].cpu().tolist() == [0, 0, 0, 0] and res[3].numel() == 0 and res[4].numel() == 0
        assert len(res) == 5 + bool(kw.get("line_numbers"))
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4 and nbuf.cpu().tolist() == [GUARD64] * 4

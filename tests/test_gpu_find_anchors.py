"""GPU tests of hufgpu_find_any_anchored and hufgpu_find_records_anchored (GpuCodec.find_pattern / find_records / grep with
`bol`, `eol`, `whole_line`, `word`): grep -w, -x, '^' and '$' - the occurrences whose neighbours allow it - in one walk,
enqueue-only.

Bit-exact, no tolerance.  Expected values come from tests/find_anchor_model.py (itself checked against Python's `re` in
tests/test_find_anchor_args.py).  As in tests/test_gpu_find_context.py every output buffer has guard words in front and behind
and is filled with the guard first.  The four shapes are those of tests/test_gpu_find_classes.py: five blocks of 4 099 bytes
(tiles of 2 048, 2 048 and 3 symbols), 300 blocks of 64 bytes (two scan groups of tiles), 200 blocks of 3 bytes, one block of
3 x 65 536 + 77 bytes (three chunks).
"""
import re

import numpy as np
import pytest

from find_anchor_model import BOL, EOL, WORD, find_any_anchored_model, find_records_anchored_model
from find_any_model import find_any_model
from find_context_model import find_context_model
from find_support import (FOUR_SHAPES, GUARD32, GUARD64, OK, RW, SEAMS, AnyOf, W, check, codec, context, damaged, encode, exact_answer,
                          literal, payload_start, positions, psearch, records, runs_input, same_arrays, torch_mod)

pytestmark = pytest.mark.gpu

ANCHORS = [BOL, EOL, WORD, BOL | EOL, BOL | WORD, EOL | WORD, 7]
NAMES = {BOL: "bol", EOL: "eol", WORD: "word", BOL | EOL: "x", BOL | WORD: "bol-word", EOL | WORD: "eol-word", 7: "all"}
EVERY = pytest.mark.parametrize("anchors", ANCHORS, ids=[NAMES[a] for a in ANCHORS])
FILL = np.frombuffer(b". -", np.uint8)                   # neither a word byte nor a delimiter
NEIGHBOURS = b"\n x"                                       # a delimiter, a boundary byte that is none, a word byte


# ---- the checks --------------------------------------------------------------------------------------------------------------
def pos_exact(torch, codec, enc, alts, anchors, delims=b"\n", words=W, room=5, what="", sub=None, all_served=True):
    """the count alone and the positions, each the model's for the blocks with status 0; returns (the model's positions, statuses)"""
    full, _, errs = exact_answer(lambda cap: positions(torch, codec, enc, alts, anchors, cap, delims, words, sub=sub),
                          lambda cap, served: find_any_anchored_model(enc.data, alts, delims, words, anchors, enc.bs, cap, served),
                          enc.n, room=room, what=(what, "positions", anchors), all_served=all_served,
                          probe=lambda: positions(torch, codec, enc, alts, anchors, 0, delims, words, sub=sub))
    return full[0], errs


def rec_exact(torch, codec, enc, alts, anchors, delims=b"\n", words=W, before=0, after=0, invert=False, room=5, max_len=0, what="",
              sub=None, all_served=True):
    """... and the records call's four outputs; returns (the model's answer at a cap that holds every record, the statuses)"""
    kw = dict(invert=invert, before=before, after=after)
    full, _, errs = exact_answer(lambda cap: records(torch, codec, enc, alts, anchors, cap, delims, words, max_len, sub=sub, **kw),
                          lambda cap, served: find_records_anchored_model(enc.data, alts, delims, words, anchors, enc.bs, cap, max_len,
                                                                          served, **kw),
                          enc.n, room=room, what=(what, "records", anchors, before, after, invert), all_served=all_served,
                          probe=lambda: records(torch, codec, enc, alts, anchors, 0, delims, words, numbers=False, flags=False, sub=sub, **kw))
    return full, errs


def filler(n, seed):
    return np.random.default_rng(seed).choice(FILL, n).astype(np.uint8)


def put(data, at, word, left, right):
    """`word` at `at` with the neighbours `left` and `right` where the data has them"""
    data[at:at + len(word)] = np.frombuffer(bytes(word), np.uint8)
    if at > 0:
        data[at - 1] = left
    if at + len(word) < data.size:
        data[at + len(word)] = right


# ---- 1: the identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_no_anchor_is_the_older_call_word_for_word(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    data = filler(n, 500)
    for i, s in enumerate(starts + SEAMS[shape]):
        if 0 < s and s + 4 < n:
            put(data, s, b"abc" if i % 2 else b"ab", NEIGHBOURS[i % 3], NEIGHBOURS[(i // 3) % 3])
    enc = encode(torch, codec, data, bs)
    alts = [literal(b"abc"), literal(b"ab")]
    for cap, counts in ((n, True), (3, False), (0, True)):
        for sets in ((b"\n", W), (None, None)):             # the sets are not looked at
            got = positions(torch, codec, enc, alts, 0, cap, *sets, counts=counts)
            assert same_arrays(got, psearch(torch, codec, enc, AnyOf(*alts), cap, counts=counts)), (shape, cap)
        check(got, find_any_model(data, alts, bs, cap), cap, shape)
        for kw in (dict(), dict(invert=True, numbers=False), dict(before=1, after=2), dict(flags=False, max_len=3)):
            for words in (W, None):
                got = records(torch, codec, enc, alts, 0, cap, b"\n", words, counts=counts, **kw)
                assert same_arrays(got, context(torch, codec, enc, alts, b"\n", cap, counts=counts, **kw)), (shape, cap, kw)
    assert int(got[2][0]) > 0
    check(records(torch, codec, enc, alts, 0, n), find_context_model(data, alts, b"\n", bs, n), n, shape)


# ---- 2: dense random data, every anchor ----------------------------------------------------------------------------------------
@EVERY
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_dense_random_data(torch_mod, codec, shape, anchors):
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(510 + anchors)
    data = rng.choice(np.frombuffer(b"abc\n x_", np.uint8), n, p=[0.2, 0.2, 0.2, 0.1, 0.15, 0.1, 0.05]).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    newlines = np.concatenate([[0], np.cumsum(data == 10)])  # in front of every byte
    letters = np.frombuffer(b"abc", np.uint8)
    seen = []
    for trial in range(2):
        alts = [[bytes(rng.choice(letters, int(rng.integers(1, 3)), replace=False).astype(np.uint8)) for _ in range(int(rng.integers(1, 5)))]
                for _ in range(int(rng.integers(1, 5)))]
        got, _ = pos_exact(torch_mod, codec, enc, alts, anchors, what=(shape, trial, alts))
        plain = find_any_model(data, alts, bs, n)[0]
        seen.append((got.size, plain.size))
        assert set(got.tolist()) <= set(plain.tolist())
        for invert, ba in ((False, (0, 0)), (True, (0, 0)), (False, (2, 2)), (True, (1, 0))):
            full, _ = rec_exact(torch_mod, codec, enc, alts, anchors, before=ba[0], after=ba[1], invert=invert, max_len=trial * 5,
                                what=(shape, trial, alts))
            assert np.array_equal(full[4], newlines[full[0]])
    assert any(a < b for a, b in seen) and (n < 1000 or any(a > 0 for a, _ in seen)), seen


def test_word_bytes_and_delimiters_of_the_caller(torch_mod, codec):
    """a delimiter that is a word byte, D and the bytes that are no word byte without a byte in common, no word bytes at all,
    every byte a word byte, two delimiters"""
    bs, n, _ = FOUR_SHAPES["5x4099"]
    rng = np.random.default_rng(520)
    data = rng.choice(np.frombuffer(b"abc\n x_", np.uint8), n, p=[0.2, 0.2, 0.2, 0.1, 0.15, 0.1, 0.05]).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    alts = [literal(b"ab"), literal(b"c"), literal(b"bca")]
    for delims, words in ((b"_", b"abcx_"), (b"\n", bytes(v for v in range(256) if v != 32)), (b"\n", b""), (b"\n", bytes(range(256))),
                          (b"\n ", b"x_\n")):
        for anchors in ANCHORS:
            pos_exact(torch_mod, codec, enc, alts, anchors, delims, words, what=(delims, len(words)))
            rec_exact(torch_mod, codec, enc, alts, anchors, delims, words, what=(delims, len(words)))
            rec_exact(torch_mod, codec, enc, alts, anchors, delims, words, invert=True, before=1, after=1, what=(delims, len(words)))


# ---- 3: a hit and its neighbours at every seam ---------------------------------------------------------------------------------
@pytest.mark.parametrize("place", [1, 0, -2, -3], ids=["left-neighbour", "first-byte", "last-byte", "right-neighbour"])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_a_hit_and_its_neighbours_at_every_seam(torch_mod, codec, shape, place):
    """the hit's left neighbour, its first byte, its last byte or its right neighbour is the first byte of a lane's word, a
    tile, a chunk, a block, a scan group; the two neighbours rotate through a delimiter, a boundary byte that is none and a
    word byte"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    word = b"abc"
    for rot in range(3):
        data = filler(n, 530 + rot)
        at = [p + place for p in SEAMS[shape] if p + place >= 1 and p + place + 4 <= n]
        for i, s in enumerate(at):
            put(data, s, word, NEIGHBOURS[(i + rot) % 3], NEIGHBOURS[(i // 3 + rot) % 3])
        enc = encode(torch, codec, data, bs)
        for anchors in ANCHORS:
            got, _ = pos_exact(torch, codec, enc, [literal(word)], anchors, what=(shape, place, rot))
            assert set(got.tolist()) <= set(at)
            rec_exact(torch, codec, enc, [literal(word)], anchors, what=(shape, place, rot))
        every = [pos_exact(torch, codec, enc, [literal(word)], a, what=shape)[0].size for a in (BOL, EOL, WORD)]
        assert all(k < len(at) for k in every) and (len(at) < 7 or all(k > 0 for k in every)), (shape, place, rot, every)


# ---- 4: the data's two ends ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_hits_at_byte_0_and_at_the_data_s_end(torch_mod, codec, shape):
    """no byte in front of byte 0 and none behind the last one: neither stands in the way.  The word of five bytes that ends
    the data starts in front of the last tile where that one is shorter (3 symbols, 2 bytes of the last block of 200 x 3)"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    word, short = b"abcab", b"q"
    for last in (word, short, b"x" + short):                # ... and a word byte in front of the last byte
        data = filler(n, 540)
        put(data, 0, word, 0, ord("x"))
        put(data, 40, word, ord(" "), ord(" "))
        data[n - len(last):] = np.frombuffer(last, np.uint8)
        enc = encode(torch, codec, data, bs)
        alts = [literal(word), literal(short)]
        for anchors in ANCHORS:
            got, _ = pos_exact(torch, codec, enc, alts, anchors, what=(shape, last))
            assert (0 in got) == (anchors & (EOL | WORD) == 0) and (n - len(last) in got) == (last != b"x" + short and not anchors & BOL)
            assert (n - 1 in got) == (last == short and not anchors & BOL or last == b"x" + short and anchors in (EOL,))
            for invert in (False, True):
                rec_exact(torch, codec, enc, alts, anchors, invert=invert, what=(shape, last))
        data[:] = np.frombuffer((word * (n // 5 + 1))[:n], np.uint8)       # the word, over and over: one record, word bytes all around
        enc = encode(torch, codec, data, bs)
        got, _ = pos_exact(torch, codec, enc, [literal(word)], WORD, what=(shape, "all"))
        assert got.tolist() == ([0] if n == 5 else [])
        got, _ = pos_exact(torch, codec, enc, [literal(word)], BOL, what=(shape, "all"))
        assert got.tolist() == [0]
        got, _ = pos_exact(torch, codec, enc, [literal(word)], EOL, what=(shape, "all"))
        assert got.tolist() == ([n - 5] if n % 5 == 0 else [])


# ---- 5: the shortest and the longest alternatives ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_alternatives_of_1_2_and_63_positions(torch_mod, codec, shape):
    """63 positions and the boundary's: the 64 bits of the state, 63 edge bytes a tile"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    long = bytes(np.random.default_rng(550).choice(np.frombuffer(b"abc", np.uint8), 63).astype(np.uint8))
    data = filler(n, 551)
    at = [p - 31 for p in SEAMS[shape] if p - 31 >= 1 and p + 33 <= n] + [n - 63]
    for i, s in enumerate(at):
        put(data, s, long, NEIGHBOURS[i % 3], NEIGHBOURS[(i // 3) % 3])
    enc = encode(torch, codec, data, bs)
    for anchors in ANCHORS:
        got, _ = pos_exact(torch, codec, enc, [literal(long)], anchors, what=(shape, 63))
        assert set(got.tolist()) <= set(at) and (anchors != EOL or n - 63 in got)
        rec_exact(torch, codec, enc, [literal(long)], anchors, before=1, after=1, what=(shape, 63))
    data = filler(n, 552)
    for i, s in enumerate(p + d for p in SEAMS[shape] for d in (-2, 0) if 1 <= p + d and p + d + 3 <= n):
        put(data, s, b"q" if i % 2 else b"zq", NEIGHBOURS[i % 3], NEIGHBOURS[(i // 2) % 3])
    enc = encode(torch, codec, data, bs)
    for anchors in ANCHORS:
        got, _ = pos_exact(torch, codec, enc, [literal(b"q"), literal(b"zq")], anchors, what=(shape, 12))
        rec_exact(torch, codec, enc, [literal(b"q"), literal(b"zq")], anchors, invert=bool(anchors & 1), what=(shape, 12))
        single, _ = pos_exact(torch, codec, enc, [literal(b"q")], anchors, what=(shape, 1))       # BOL alone: no seam kernel at all
        assert set(single.tolist()) <= set(np.flatnonzero(data == ord("q")).tolist())


# ---- 6: one-symbol blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["200x3", "5x4099", "300x64"])
def test_one_symbol_blocks_next_to_ordinary_ones(torch_mod, codec, shape):
    """blocks of a word byte, of a boundary byte that is no delimiter and of the delimiter, each with a hit that ends just in
    front of it and one that starts just behind it; the alternatives of one byte lie INSIDE such blocks, where the one value is
    then its own neighbour"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    nb = (n + bs - 1) // bs
    data = filler(n, 560)
    for k, b in enumerate(range(1, nb - 1, 2 if nb < 10 else 7)):
        leaf = b"x \n"[k % 3]
        data[b * bs - 3:b * bs] = np.frombuffer(b"abc", np.uint8)
        data[(b + 1) * bs:(b + 1) * bs + 3] = np.frombuffer(b"abc", np.uint8)
        data[b * bs:(b + 1) * bs] = leaf
    assert sum(np.unique(data[o:o + bs]).size == 1 for o in range(0, n - bs, bs)) >= 2
    enc = encode(torch, codec, data, bs)
    for anchors in ANCHORS:
        for alts in ([literal(b"abc")], [literal(b"abc"), literal(b" ")], [literal(b"x")], [literal(b"xx"), literal(b"  ")]):
            pos_exact(torch, codec, enc, alts, anchors, what=(shape, alts))
            rec_exact(torch, codec, enc, alts, anchors, what=(shape, alts))
            rec_exact(torch, codec, enc, alts, anchors, invert=True, before=1, after=1, what=(shape, alts))
        pos_exact(torch, codec, enc, [literal(b"\n")], anchors, what=(shape, "the delimiter"))     # (the positions call may look for it)
    assert pos_exact(torch, codec, enc, [literal(b"x")], WORD, what=shape)[0].size == 0 or bs == 1
    assert pos_exact(torch, codec, enc, [literal(b" ")], WORD, what=shape)[0].size >= bs


# ---- 7: blocks that are not served -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """runs of 207 between 7s: with 207 the one word byte, or 7 the delimiter on both sides, the runs of exactly nine bytes.  A
    hit next to the block is dropped only when the anchor looks at a neighbour in it"""
    torch = torch_mod
    enc, delim, alts = runs_input(torch, codec)
    bs = enc.bs
    whole = {a: pos_exact(torch, codec, enc, alts, a, delim, bytes([207]), what="undamaged")[0] for a in ANCHORS}
    assert whole[WORD].size > 5 and np.array_equal(whole[WORD], whole[BOL | EOL]) and whole[BOL].size > whole[WORD].size
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for anchors in ANCHORS:
            got, errs = pos_exact(torch, codec, bad, alts, anchors, delim, bytes([207]), what=(damage, b), all_served=False)
            assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
            lo = whole[anchors] - (1 if anchors & (BOL | WORD) else 0)
            hi = whole[anchors] + (9 if anchors & (EOL | WORD) else 8)
            keep = (np.maximum(lo, 0) // bs > b) | (np.minimum(hi, enc.n - 1) // bs < b)
            assert np.array_equal(got, whole[anchors][keep]), (damage, b, anchors)
            for invert in (False, True):
                full, _ = rec_exact(torch, codec, bad, alts, anchors, delim, bytes([207]), invert=invert, before=invert, what=(damage, b),
                                    all_served=False)
                assert int(full[3][2]) == 1


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    n = 5 * bs + 1500
    data = filler(n, 570)
    for i, s in enumerate([100, bs - 3, bs, 2 * bs + 2045, 3 * bs - 4, 5 * bs + 1494]):
        put(data, s, b"abc", NEIGHBOURS[i % 3], NEIGHBOURS[(i + 1) % 3])
    enc = encode(torch, codec, data, bs)
    rng = np.random.default_rng(571)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    for anchors in (WORD, BOL | EOL, 7):
        _, errs = pos_exact(torch, codec, enc, [literal(b"abc")], anchors, sub=other, what=sub, all_served=False)
        assert sub == "random" or errs.all()
        rec_exact(torch, codec, enc, [literal(b"abc")], anchors, sub=other, before=1, after=1, what=sub, all_served=False)
        bad = damaged(enc, int(enc.h_offs[1]), 0x01)
        pos_exact(torch, codec, bad, [literal(b"abc")], anchors, sub=other, what=(sub, "and a damaged block"), all_served=False)
        rec_exact(torch, codec, bad, [literal(b"abc")], anchors, sub=other, what=(sub, "and a damaged block"), all_served=False)


# ---- 8: caps ---------------------------------------------------------------------------------------------------------------------
def test_caps(torch_mod, codec):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    data = filler(n, 580)
    for i, s in enumerate(starts[1:]):
        put(data, s, b"abc", NEIGHBOURS[i % 2], NEIGHBOURS[(i // 2) % 2])
    data[[500, 2 * bs + 7, 4 * bs]] = 10
    enc = encode(torch, codec, data, bs)
    alts = [literal(b"abc")]
    total = int(find_any_anchored_model(data, alts, b"\n", W, WORD, bs, n)[2][0])
    assert 4 <= total <= len(starts) - 1
    for cap in (0, 1, total - 1, total):
        for counts in (True, False):
            res = positions(torch, codec, enc, alts, WORD, cap, counts=counts)
            check(res, find_any_anchored_model(data, alts, b"\n", W, WORD, bs, cap), cap, (cap, counts))
    for invert in (False, True):
        kw = dict(invert=invert, before=1, after=0)
        total = int(find_records_anchored_model(data, alts, b"\n", W, BOL, bs, n, **kw)[3][0])
        assert total >= 2
        for cap in (0, 1, total - 1, total):
            for numbers, flags, max_len in ((True, True, 0), (False, True, 7), (True, False, 1), (False, False, 0)):
                res = records(torch, codec, enc, alts, BOL, cap, max_len=max_len, numbers=numbers, flags=flags, **kw)
                check(res, find_records_anchored_model(data, alts, b"\n", W, BOL, bs, cap, max_len, **kw), cap, (invert, cap, numbers, flags))


# ---- 9: one context, call after call ---------------------------------------------------------------------------------------------
def test_eight_calls_back_to_back(torch_mod, codec):
    """anchored and older calls alternate without a synchronise in between: each gives its own model's answer, and the third
    mask, the boundary mask in the delimiters' place and the longer table of one call leave nothing behind for the next"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    data = filler(n, 590)
    for i, s in enumerate(starts[1:] + SEAMS["5x4099"]):
        put(data, s, b"abc", NEIGHBOURS[i % 3], NEIGHBOURS[(i // 3) % 3])
    enc = encode(torch, codec, data, bs)
    alts = [literal(b"abc")]
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    jobs = [("r", WORD), ("r", 0), ("p", WORD), ("p", 0), ("r", BOL | EOL), ("p", BOL), ("r", 0), ("p", EOL)]
    kws = {0: dict(), WORD: dict(word=True), BOL | EOL: dict(whole_line=True), BOL: dict(bol=True), EOL: dict(eol=True)}
    out = []
    for kind, anchors in jobs:
        if kind == "r":
            out.append(codec.find_records(*args, b"abc", max_records=n, block_counts=True, **kws[anchors]))
        else:
            out.append(codec.find_pattern(*args, b"abc", max_positions=n, block_counts=True, **kws[anchors]))
    torch.cuda.synchronize()
    for (kind, anchors), res in zip(jobs, out):
        if kind == "r":
            want = find_records_anchored_model(data, alts, b"\n", W, anchors, bs, n)
            total = int(want[3][0])
            assert len(res) == 5 and res[2].cpu().tolist() == want[3].tolist() and total > 0, (kind, anchors)
            assert res[0].cpu().numpy()[:total].tolist() == want[0].tolist() and res[1].cpu().numpy()[:total].tolist() == want[1].tolist()
            assert np.array_equal(res[4].cpu().numpy(), want[2]) and not res[3].cpu().numpy().any()
        else:
            want = find_any_anchored_model(data, alts, b"\n", W, anchors, bs, n)
            total = int(want[2][0])
            assert res[1].cpu().tolist() == want[2].tolist() and total > 0, (kind, anchors)
            assert res[0].cpu().numpy()[:total].tolist() == want[0].tolist() and np.array_equal(res[3].cpu().numpy(), want[1])


# ---- 10: Python ------------------------------------------------------------------------------------------------------------------
def test_grep_word_ignore_case(torch_mod, codec):
    """grep(b"error", word=True, ignore_case=True) without a synchronisation, against an `re` filter over data.split(b"\\n")"""
    torch = torch_mod
    rng = np.random.default_rng(600)
    pool = [b"an error here", b"errors galore", b"stderror: 5", b"ERROR: disk", b"all is well", b"error", b"Error_code 7", b"x=error;", b"",
            b"terror", b"no Error.", b"error2", b"(eRRor)", b"errorerror error"]
    lines = [pool[i] for i in rng.integers(0, len(pool), 3000)]
    raw = b"\n".join(lines)
    data = np.frombuffer(raw, np.uint8)
    n, bs = data.size, 4096
    want = [(i, l) for i, l in enumerate(lines) if re.search(rb"(?<![A-Za-z0-9_])error(?![A-Za-z0-9_])", l, re.I)]
    assert 0 < len(want) < sum(1 for l in lines if re.search(rb"error", l, re.I))
    enc = encode(torch, codec, data, bs)
    cap, width = len(want) + 5, 32
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    out = codec.grep(*args, b"error", cap, width, word=True, ignore_case=True, line_numbers=True)
    assert len(out) == 6
    rows, raws, gerrs, totals, block_errs, numbers = (x.cpu().numpy() for x in out)
    assert totals.tolist() == [len(want), len(want), 0, 0] and not block_errs.any() and not gerrs.any()
    assert numbers[:len(want)].tolist() == [i for i, _ in want]
    for k, (_, line) in enumerate(want):
        assert raws[k] == len(line) and bytes(rows[k, :raws[k]]) == line, k
    totals, _ = codec.count_records(*args, b"error", whole_line=True)
    assert totals.cpu().tolist() == [lines.count(b"error"), 0, 0, 0]
    totals, _ = codec.count_records(*args, b"error", bol=True, ignore_case=True)
    assert totals.cpu().tolist() == [sum(1 for l in lines if re.match(rb"error", l, re.I)), 0, 0, 0]
    totals, _ = codec.count_records(*args, AnyOf(b"well", b"here"), eol=True, invert=True)
    assert totals.cpu().tolist() == [sum(1 for l in lines if l and not re.search(rb"(well|here)$", l)), 0, 0, 0]
    totals, _ = codec.count_pattern(*args, b"error", word=True)
    assert totals.cpu().tolist() == [len(re.findall(rb"(?<![A-Za-z0-9_])error(?![A-Za-z0-9_])", raw)), 0, 0, 0]
    totals, _ = codec.count_pattern(*args, b"error", word=True, word_bytes=b"abcdefghijklmnopqrstuvwxyz")
    assert totals.cpu().tolist() == [len(re.findall(rb"(?<![a-z])error(?![a-z])", raw)), 0, 0, 0]
    totals, _ = codec.count_pattern(*args, b"error", bol=True, delimiters=b" \n")
    assert totals.cpu().tolist() == [len(re.findall(rb"(?:^|(?<=[ \n]))error", raw)), 0, 0, 0]
    assert len(codec.grep(*args, b"error", cap, width)) == 5         # as it always was
    for kw in (dict(word_bytes=b"abc"), dict(word=True, word_bytes=[256])):
        with pytest.raises(ValueError):
            codec.grep(*args, b"error", cap, width, **kw)
    with pytest.raises(ValueError, match="sum to 65"):
        codec.find_pattern(*args, b"e" * 64, eol=True)


# ---- 11: no blocks ---------------------------------------------------------------------------------------------------------------
def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    for kw in (dict(word=True), dict(whole_line=True), dict(bol=True, word=True)):
        res = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, AnyOf(b"error", b"x"), max_records=4, block_counts=True,
                                 out=(buf, lbuf), invert=True, **kw)
        assert res[2].cpu().tolist() == [0, 0, 0, 0] and res[3].numel() == 0 and res[4].numel() == 0 and len(res) == 5
        res = codec.find_pattern(empty, 0, offsets, 0, sub, 0, 4096, AnyOf(b"error", b"x"), max_positions=4, block_counts=True, out=buf, **kw)
        assert res[1].cpu().tolist() == [0, 0, 0, 0] and res[2].numel() == 0 and res[3].numel() == 0
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4

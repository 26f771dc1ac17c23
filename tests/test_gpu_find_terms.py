"""GPU tests of hufgpu_find_records_terms (GpuCodec.find_records / count_records / grep with GpuCodec.AllOf and GpuCodec.Seq):
the records that hold all of several terms, or all of them one behind the other, from one walk of the stream.

Bit-exact, no tolerance.  Expected values come from tests/find_terms_model.py (a brute force over all occurrences a record,
itself checked against Python's `re` in tests/test_find_terms_args.py).  Every output buffer - starts, lengths, numbers and
flags - has guard words in front and behind and is filled with the guard first, as in tests/test_gpu_find_context.py, and
every block of an intact stream must be served (totals[2] == 0), so "not served" cannot hide a wrong answer.  The shapes are
tests/find_support.py's: five blocks of 4 099 bytes, 300 blocks of 64 bytes (two scan groups of tiles), 200 blocks of 3 bytes,
one block of three chunks.
"""
import re

import numpy as np
import pytest

import find_support
from find_any_model import find_any_records_model
from find_context_model import find_context_model
from find_support import (CHUNK, FOUR_SHAPES, GUARD8, GUARD32, GUARD64, LEAD, NL, OK, RW, SEAMS, TILE, AnyOf, base_without, check, codec,  # noqa: F401
                          context, damaged, encode, literal, mixed_blocks, pattern_below_255, payload_start, planted, planted_each,
                          runs_input, same_arrays, seven, torch_mod, with_delimiters)
from find_terms_model import ALL, ORDERED, find_terms_model
from find_terms_support import terms_call
from libhuffman_amd import datagen
from libhuffman_amd.codec import GpuCodec

pytestmark = pytest.mark.gpu

AllOf, Seq = GpuCodec.AllOf, GpuCodec.Seq
MODES = ((ALL, "all"), (ORDERED, "ordered"))


# ---- the check ---------------------------------------------------------------------------------------------------------------
def terms_exact(torch, codec, enc, terms, mode, delims=b"\n", before=0, after=0, invert=False, room=5, max_len=0, what="", sub=None,
                all_served=True, must=(), must_not=()):
    """the answer without outputs and with all four, each equal to the model's for the blocks with status 0; returns (the
    model's answer at a cap that holds every record, the statuses)"""
    kw = dict(invert=invert, before=before, after=after)
    full, _, errs = find_support.exact_answer(lambda cap: terms_call(torch, codec, enc, terms, mode, cap, delims, max_len, sub=sub, **kw),
                                              lambda cap, served: find_terms_model(enc.data, terms, delims, enc.bs, cap, max_len, served, mode=mode, **kw),
                                              enc.n, must, must_not, room=room, what=(what, mode, before, after, invert), all_served=all_served,
                                              probe=lambda: terms_call(torch, codec, enc, terms, mode, 0, delims, numbers=False, flags=False, sub=sub, **kw))
    return full, errs


def fenced(n, spans, step=97):
    """delimiter positions: one in front of and one behind every span [lo, hi) - those inside the data -, and one every `step`
    bytes outside the spans, so that the rest of the data is records as well"""
    inside = np.zeros(n + 1, bool)
    at = set()
    for lo, hi in spans:
        inside[max(lo - 1, 0):hi + 1] = True
        at |= {q for q in (lo - 1, hi) if 0 <= q < n}
    return sorted(at | {q for q in range(step - 1, n, step) if not inside[q]})


# ---- 1: the identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_one_term_is_the_context_call(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    words = [pattern_below_255(5, 501), pattern_below_255(5, 502)]      # (one length: an ordered term's)
    data = with_delimiters(base_without(n, 281), [p - 1 for p in SEAMS[shape]] + [n - 1])
    for i, s in enumerate(SEAMS[shape]):
        data = planted(data, words[i % 2], [s + 2 + i % 3] if i % 3 and s + 10 < n else [])
    enc = encode(torch, codec, data, bs)
    alts = [literal(w) for w in words]
    for mode, _ in MODES:
        for kw in (dict(), dict(invert=True), dict(before=1, after=2), dict(invert=True, before=2), dict(numbers=False), dict(flags=False),
                   dict(numbers=False, flags=False, counts=False)):
            for cap, max_len in ((n, 0), (3, 7), (0, 0)):
                got = terms_call(torch, codec, enc, [words], mode, cap, b"\n", max_len, **kw)
                older = context(torch, codec, enc, alts, b"\n", cap, max_len, **kw)
                assert same_arrays(got, older) and [x is None for x in got] == [x is None for x in older], (shape, mode, kw, cap)
                assert int(got[2][0]) > 0 and int(got[2][2]) == 0


# ---- 2: dense random data ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nterms", [2, 3, 4])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_dense_random_data(torch_mod, codec, shape, nterms):
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(278 + nterms)
    letters = np.frombuffer(b"abcd"[:3 + nterms % 2], np.uint8)
    p = [0.93 / letters.size] * letters.size + [0.07]
    data = rng.choice(np.concatenate([letters, [NL]]).astype(np.uint8), n, p=p).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    sizes = []
    for trial, (before, after) in enumerate(((0, 0), (1, 2), (2, 0), (0, 1))):
        terms = []
        for _ in range(nterms):                             # one to three bytes, one length a term, one or two alternatives
            m = int(rng.integers(1, 4))
            terms.append([bytes(rng.choice(letters, m).astype(np.uint8)) for _ in range(int(rng.integers(1, 3)))])
        for mode, _ in MODES:
            invert = bool((trial + mode) & 1)
            full, _ = terms_exact(torch_mod, codec, enc, terms, mode, before=before, after=after, invert=invert, what=(shape, terms))
            sizes.append((mode, int(full[5].sum())))
    assert any(k for m, k in sizes if m == ALL) and any(k for m, k in sizes if m == ORDERED), sizes


# ---- 3: the second term in every place behind the first ------------------------------------------------------------------------
def places(shape):
    """name -> (where the first word starts, how far behind it the second one starts), the whole span inside one block's row
    of tiles or across the seam that the name says"""
    bs, n, _ = FOUR_SHAPES[shape]
    tile = min(bs or TILE, TILE)
    if shape == "3chunks":
        return {"the same word": (TILE + 2, 8), "the next lane": (TILE + 2, 32), "the next tile": (TILE + 40, TILE),
                "an empty tile between": (TILE + 40, 3 * TILE), "the next chunk": (CHUNK - 3 * TILE + 9, CHUNK),
                "the look-up across chunks": (5 * TILE + 9, 2 * CHUNK + 7 * TILE)}
    if shape == "5x4099":
        return {"the same word": (bs + 2, 8), "the next lane": (bs + 2, 32), "the next tile": (bs + 40, tile),
                "the next block": (bs + 2 * TILE - 20, bs), "an empty tile between": (20, 3 * bs + 100)}
    return {"the same word": (10 * 64 + 2, 8), "the next lane": (10 * 64 + 2, 32), "the next tile": (10 * 64 + 40, 64),
            "an empty tile between": (20 * 64 + 5, 3 * 64), "across the scan groups": (250 * 64 + 5, 12 * 64)}


@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_the_second_term_in_every_place(torch_mod, codec, shape):
    """two words in one record, the second one in the same mask word, the next lane's, the next tile, a tile with empty tiles
    between (the look-up), the next chunk, the next block: ALL does not mind the order, ORDERED does"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    a, b = pattern_below_255(5, 511), pattern_below_255(5, 512)
    base = base_without(n, 282)
    for name, (p0, gap) in places(shape).items():
        lo, hi = p0 - 3, p0 + gap + 9
        assert 0 < lo and hi < n, (shape, name)
        data = planted_each(with_delimiters(base, fenced(n, [(lo, hi)])), [a, b], [p0, p0 + gap])
        enc = encode(torch, codec, data, bs)
        for terms, ordered in (([[a], [b]], True), ([[b], [a]], False)):
            terms_exact(torch, codec, enc, terms, ALL, must=[lo], what=(shape, name))
            terms_exact(torch, codec, enc, terms, ORDERED, must=[lo] if ordered else [], must_not=[] if ordered else [lo], what=(shape, name))
            full, _ = terms_exact(torch, codec, enc, terms, ORDERED, invert=True, what=(shape, name))
            assert (lo in full[0].tolist()) != ordered


# ---- 4: adjacency and overlap at every seam ------------------------------------------------------------------------------------
CASES = [(b"abc", [[b"ab"], [b"bc"]], True, False), (b"abbc", [[b"ab"], [b"bc"]], True, True), (b"aaa", [[b"aa"], [b"aa"]], True, False),
         (b"aaaa", [[b"aa"], [b"aa"]], True, True), (b"abc", [[b"ab"], [b"abc"]], True, False)]


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_adjacent_and_overlapping_occurrences_at_every_seam(torch_mod, codec, shape):
    """a record that is exactly the string, its third byte on the seam: the two pieces meet at the edge of a lane's word, a
    tile, a chunk, a block and a scan group"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    base = base_without(n, 283)
    base[np.isin(base, np.frombuffer(b"abc", np.uint8))] = ord("z")     # (so nothing but the planted strings holds a term)
    for string, terms, in_all, in_order in CASES:
        at = [q - 2 for q in SEAMS[shape] if q - 2 + len(string) <= n]
        data = planted_each(with_delimiters(base, fenced(n, [(s, s + len(string)) for s in at])), [string] * len(at), at)
        enc = encode(torch, codec, data, bs)
        for mode, holds in ((ALL, in_all), (ORDERED, in_order)):
            full, _ = terms_exact(torch, codec, enc, terms, mode, must=at if holds else [], must_not=[] if holds else at, what=(shape, string))
            assert full[0].tolist() == (at if holds else [])


# ---- 5: nothing is borrowed across a delimiter ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_no_term_is_borrowed_from_the_next_record(torch_mod, codec, shape):
    """"B A" and then "B" in the record behind, the delimiter between them on the seam: (A, B) in order nowhere, ALL in the first
    record only"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    a, b = b"\xf1\xf2", b"\xf3\xf4"
    base = base_without(n, 284)
    base[base >= 0xf1] = 0x30
    seams = [q for q in SEAMS[shape] if q >= 8 and q + 3 <= n]
    first = [q - 7 for q in seams]                          # B at q - 7, A at q - 4, the delimiter at q - 1, B at q
    data = with_delimiters(base, fenced(n, [(s, s + 6) for s in first] + [(q, q + 2) for q in seams]))
    data = planted_each(data, [b] * len(seams) + [a] * len(seams) + [b] * len(seams), first + [q - 4 for q in seams] + seams)
    enc = encode(torch, codec, data, bs)
    full, _ = terms_exact(torch, codec, enc, [[a], [b]], ORDERED, what=shape)
    assert full[0].size == 0
    full, _ = terms_exact(torch, codec, enc, [[a], [b]], ALL, must=first, must_not=seams, what=shape)
    assert full[0].tolist() == first
    full, _ = terms_exact(torch, codec, enc, [[b], [a]], ORDERED, must=first, must_not=seams, what=shape)


# ---- 6: three terms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_three_terms_and_a_second_alternative(torch_mod, codec, shape):
    """"A C B C" holds (A, B, C) in order, "A C B" does not; a term of two alternatives of which only the second lies there"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    a, b, c, never = b"\xf1\xf2", b"\xf3\xf4", b"\xf5\xf6", b"\xf7\xf8"
    base = base_without(n, 285)
    base[base >= 0xf1] = 0x30
    yes, no = a + b"-" + c + b"-" + b + b"-" + c, a + b"-" + c + b"-" + b
    seams = [q for q in SEAMS[shape] if q >= 6 and q + 12 <= n]
    at = [q - 4 for q in seams]                             # the seam inside the string, in front of B
    strings = [yes if i % 2 == 0 else no for i in range(len(at))]
    data = planted_each(with_delimiters(base, fenced(n, [(s, s + len(w)) for s, w in zip(at, strings)])), strings, at)
    enc = encode(torch, codec, data, bs)
    for terms in ([[a], [b], [c]], [[never, a], [never, b], [never, c]], [[a], [b], [never, c]]):
        full, _ = terms_exact(torch, codec, enc, terms, ORDERED, must=at[0::2], must_not=at[1::2], what=shape)
        assert full[0].tolist() == at[0::2]
        full, _ = terms_exact(torch, codec, enc, terms, ALL, must=at, what=shape)
        assert full[0].tolist() == at
    full, _ = terms_exact(torch, codec, enc, [[a], [b], [c], [never]], ALL, what=shape)
    assert full[0].size == 0


# ---- 7: each term's only occurrence across every seam ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_term_k_straddles_every_start(torch_mod, codec, shape, k):
    """four terms in order in one record, 8 bytes apart; term k - five bytes - starts at the shape's starts, which reach the
    seams of a lane, a tile, a chunk, a block and a scan group: its bit and its count are the seam kernel's, term by term"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    words = [pattern_below_255(5 if j == k else 3, 520 + j) for j in range(4)]
    starts = [s for s in starts if s - 8 * k - 1 >= 0 and s + 8 * (3 - k) + 6 <= n]
    assert len(starts) >= 2
    spans = [(s - 8 * k, s + 8 * (3 - k) + 5) for s in starts]
    data = with_delimiters(base_without(n, 286), fenced(n, spans))
    for j in range(4):
        data = planted(data, words[j], [s + 8 * (j - k) for s in starts])
    enc = encode(torch, codec, data, bs)
    terms = [[w] for w in words]
    want = [lo for lo, _ in spans]
    for mode, _ in MODES:
        full, _ = terms_exact(torch, codec, enc, terms, mode, must=want, what=(shape, k))
        assert full[0].tolist() == want
    swapped = terms[1:] + terms[:1]
    full, _ = terms_exact(torch, codec, enc, swapped, ORDERED, must_not=want, what=(shape, k))
    assert full[0].size == 0


# ---- 8: one record over three chunks -----------------------------------------------------------------------------------------
def test_one_record_without_a_delimiter(torch_mod, codec):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["3chunks"]
    words = [pattern_below_255(4, 531), pattern_below_255(6, 532), pattern_below_255(3, 533)]
    data = planted_each(base_without(n, 287), words, [100, CHUNK + 5 * TILE + 2046, n - 40])    # the first tile, ..., the last tile
    enc = encode(torch, codec, data, bs)
    for delims in (b"\n", b""):
        for terms, ordered in (([[w] for w in words], True), ([[w] for w in reversed(words)], False), ([[words[0]], [words[2]]], True),
                               ([[words[2]], [words[0]]], False)):
            full, _ = terms_exact(torch, codec, enc, terms, ALL, delims, what="all")
            assert [x.tolist() for x in full[:2]] == [[0], [n]] and int(full[3][0]) == 1
            full, _ = terms_exact(torch, codec, enc, terms, ORDERED, delims, what="ordered")
            assert int(full[3][0]) == int(ordered)
            full, _ = terms_exact(torch, codec, enc, terms, ORDERED, delims, invert=True, what="ordered, inverted")
            assert int(full[3][0]) == int(not ordered)


# ---- 9: one-symbol blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["200x3", "5x4099", "300x64"])
def test_one_symbol_blocks_next_to_ordinary_ones(torch_mod, codec, shape):
    """every second block is the one value 41: a leaf that is in one term's classes and not in the other's, in both, and in a
    pattern of two positions, whose occurrences run across the blocks' ends"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    nblocks = (n + bs - 1) // bs
    data = mixed_blocks(bs, nblocks, 288)[:n]
    odd = np.flatnonzero((np.arange(n) // bs) % 2 == 1)     # delimiters and the other term's byte in the ordinary blocks only
    rng = np.random.default_rng(289)
    data[data == NL] = 0x31
    data[rng.choice(odd, odd.size // 9, replace=False)] = NL
    data[rng.choice(odd, odd.size // 7, replace=False)] = 0xf2
    assert sum(np.unique(data[o:o + bs]).size == 1 for o in range(0, n - bs + 1, bs)) >= nblocks // 2 - 1
    enc = encode(torch, codec, data, bs)
    leaf, other = [b")\xf1"], [b"\xf2"]
    for terms in ([[leaf], [other]], [[other], [leaf]], [[leaf], [b")\xf2"]], [[[b")", b")"]], [other]], [[other], [[b")\xf2", b")"]]],
                  [[leaf], [other], [[b")", b")\xf2"]]]):
        found = []
        for mode, _ in MODES:
            for invert in (False, True):
                full, _ = terms_exact(torch, codec, enc, terms, mode, invert=invert, before=mode, what=(shape, terms))
                found.append(int(full[5].sum()))
        assert found[0] > 0 and found[1] > 0 and found[3] >= found[1], (shape, terms, found)


# ---- 10: blocks that are not served --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """totals[2] is 1, a record that touches the block is in neither the plain nor the inverted answer, every other record of
    known extent is in exactly one of them"""
    torch = torch_mod
    enc, delim, alts = runs_input(torch, codec)
    bs, n = enc.bs, enc.n
    terms = [[alts[0]], [[bytes([207])] * 4]]                # a run of nine holds both; thirteen hold them in order
    for mode, _ in MODES:
        whole = terms_exact(torch, codec, enc, terms, mode, delim, what="undamaged")[0]
        every = terms_exact(torch, codec, enc, terms, mode, delim, invert=True, what="undamaged")[0]
        records = sorted(zip(whole[0].tolist() + every[0].tolist(), whole[1].tolist() + every[1].tolist()))
        for b in range(5):
            if damage == "a payload bit":
                bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
            else:
                bad = damaged(enc, int(enc.h_offs[b]), 0x01)
            got = []
            for invert in (False, True):
                full, errs = terms_exact(torch, codec, bad, terms, mode, delim, invert=invert, before=1, what=(damage, b), all_served=False)
                assert errs.tolist() == [RW if j == b else OK for j in range(5)] and int(full[3][2]) == 1
                plain, _ = terms_exact(torch, codec, bad, terms, mode, delim, invert=invert, what=(damage, b), all_served=False)
                for s, ln in zip(plain[0].tolist(), plain[1].tolist()):
                    assert not max(s - 1, 0) // bs <= b <= min(s + ln, n - 1) // bs, (b, s, ln)
                got.append(plain[0].tolist())
            away = [s for s, ln in records if not max(s - 1, 0) // bs <= b <= min(s + ln, n - 1) // bs]     # every other record: in exactly one
            assert not set(got[0]) & set(got[1]) and sorted(got[0] + got[1]) == away and 0 < len(away) < len(records)
            assert set(got[0]) <= set(whole[0].tolist()) and set(got[1]) <= set(every[0].tolist())


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    a, b = pattern_below_255(6, 560), pattern_below_255(4, 561)
    data = base_without(5 * bs + 1500, 290)
    data = with_delimiters(data, np.arange(37, data.size, 601))
    data = planted_each(data, [a, b, b, a, a, b], [100, 140, bs - 3, bs + 40, 5 * bs + 1400, 5 * bs + 1494])
    enc = encode(torch, codec, data, bs)
    rng = np.random.default_rng(234)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    for mode, _ in MODES:
        terms_exact(torch, codec, enc, [[a], [b]], mode, before=1, after=1, what="own")
        _, errs = terms_exact(torch, codec, enc, [[a], [b]], mode, before=1, after=1, sub=other, max_len=9, what=sub, all_served=False)
        assert sub == "random" or errs.all()
        bad = damaged(enc, int(enc.h_offs[1]), 0x01)
        terms_exact(torch, codec, bad, [[a], [b]], mode, after=2, sub=other, what=(sub, "and a damaged block"), all_served=False)


# ---- 11: caps ------------------------------------------------------------------------------------------------------------------
def test_caps_and_lengths(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    a, b = pattern_below_255(5, 570), pattern_below_255(3, 571)
    nl = [99, 2047, bs - 1, bs + 3000, 2 * bs + 4096, 3 * bs + 10, 4 * bs + 4000]
    data = planted_each(with_delimiters(base_without(n, 291), nl), [a, b, b, a, a, b], [2100, 2200, bs + 5, bs + 2500, n - 60, n - 5])
    enc = encode(torch, codec, data, bs)
    terms = [[a], [b]]
    for mode, total in ((ALL, 3), (ORDERED, 2)):
        for kw in (dict(), dict(invert=True), dict(before=1, after=1)):
            full = find_terms_model(data, terms, b"\n", bs, n, mode=mode, **kw)
            found = int(full[3][0])
            assert kw or found == total
            for cap in (0, 1, found - 1, found, found + 3):
                for numbers, flags, counts in ((True, True, True), (False, True, False), (True, False, True), (False, False, False)):
                    res = terms_call(torch, codec, enc, terms, mode, cap, numbers=numbers, flags=flags, counts=counts, **kw)
                    assert int(res[2][0]) == found and not res[3].any()
                    check(res, find_terms_model(data, terms, b"\n", bs, cap, mode=mode, **kw), cap, (mode, kw, cap, numbers, flags))
            for max_len in (1, 2046, 2047, 2048):
                res = terms_call(torch, codec, enc, terms, mode, found, max_len=max_len, **kw)
                check(res, find_terms_model(data, terms, b"\n", bs, found, max_len, mode=mode, **kw), found, (mode, kw, max_len))


# ---- 12: one context, call after call ------------------------------------------------------------------------------------------
def test_calls_back_to_back():
    """a context of its own, so that the terms' workspaces grow from nothing: four terms on the large shape, two on a small one
    (stale masks of the larger call lie behind them), the any-of records' call, three terms in order - each its model's answer"""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    own = GpuCodec(0)
    try:
        words = [pattern_below_255(3 + j, 580 + j) for j in range(4)]
        big_bs, big_n, starts = FOUR_SHAPES["3chunks"]
        at = [s for s in starts if s + 40 < big_n]
        data = with_delimiters(base_without(big_n, 292), fenced(big_n, [(s - 2, s + 38) for s in at], step=211))
        for j, w in enumerate(words):
            data = planted(data, w, [s + 9 * j for s in at[j % 2::2] + at[:2]])
        big = encode(torch, own, data, big_bs)
        small_bs, small_n, _ = FOUR_SHAPES["200x3"]
        small_data = with_delimiters(base_without(small_n, 293), [50, 120, 300, 420])
        small_data = planted_each(small_data, [words[0], words[1], words[1], words[0], words[0]], [60, 80, 130, 200, 430])
        small = encode(torch, own, small_data, small_bs)
        for _ in range(2):                                  # the second round finds every workspace in place
            full, _ = terms_exact(torch, own, big, [[w] for w in words], ALL, before=1, what="four terms")
            assert int(full[5].sum()) >= 2
            full, _ = terms_exact(torch, own, small, [[words[0]], [words[1]]], ORDERED, what="two terms")
            assert full[0].tolist() == [51]
            full, _ = terms_exact(torch, own, small, [[words[0]], [words[1]]], ALL, invert=True, what="two terms")
            assert full[0].tolist() == [0, 301, 421]              # (the record at 121 holds both, the second word first)
            res = find_support.rsearch(torch, own, big, AnyOf(*words[:2]), b"\n", big_n)
            check(res, find_any_records_model(data, [literal(w) for w in words[:2]], b"\n", big_bs, big_n), big_n, "any-of")
            full, _ = terms_exact(torch, own, big, [[w] for w in words[:3]], ORDERED, after=1, what="three terms")
            assert int(full[5].sum()) >= 2
            res = context(torch, own, big, [literal(words[3])], b"\n", big_n, before=1)
            check(res, find_context_model(data, [literal(words[3])], b"\n", big_bs, big_n, before=1), big_n, "context")
    finally:
        own.close()


# ---- 13: Python ----------------------------------------------------------------------------------------------------------------
def test_grep_with_allof_and_seq(torch_mod, codec):
    """a few KiB of log text against `re` over the decoded lines"""
    torch = torch_mod
    n, bs = 24 * 1024 + 77, 4096
    data = datagen.logtext(n)
    lines = bytes(data).split(b"\n")
    enc = encode(torch, codec, data, bs)
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    width = 200
    jobs = [(AllOf(b"ERROR", b"cache"), dict(), lambda l: b"ERROR" in l and b"cache" in l),
            (AllOf(b"cache", b"ERROR"), dict(), lambda l: b"ERROR" in l and b"cache" in l),
            (Seq(b"ERROR", b"cache"), dict(), lambda l: re.search(rb"ERROR.*cache", l)),
            (Seq(b"cache", b"ERROR"), dict(), lambda l: re.search(rb"cache.*ERROR", l)),        # (no line: the level comes first)
            (Seq(b"cache", b"cache"), dict(), lambda l: re.search(rb"cache.*cache", l)),
            (Seq(AnyOf(b"ERROR", b"TRACE"), b"ed", AnyOf(b"0x", b"us")), dict(), lambda l: re.search(rb"(?:ERROR|TRACE).*ed.*(?:0x|us)", l)),
            (AllOf(b"error", b"KERNEL", b"miss"), dict(ignore_case=True), lambda l: all(re.search(w, l, re.I) for w in (b"error", b"kernel", b"miss"))),
            (Seq(b"warn", [b"gG", b"cC", b":"]), dict(ignore_case=True), lambda l: re.search(rb"warn.*gc:", l, re.I)),
            (AllOf(b"WARN", AnyOf(b"auth", b"gc"), b"seq=", b"ms"), dict(), lambda l: b"WARN" in l and re.search(rb"auth|gc", l) and b"seq=" in l and b"ms" in l),
            (AllOf(b"INFO", b"status=2"), dict(invert=True), lambda l: not (b"INFO" in l and b"status=2" in l))]
    for pattern, kw, holds in jobs:
        want = [i for i, l in enumerate(lines) if l and holds(l)]
        assert len(want) < sum(1 for l in lines if l) and (len(want) > 0 or pattern.items == (b"cache", b"ERROR")), (pattern, len(want))
        cap = len(want) + 3
        out = codec.grep(*args, pattern, cap, width, line_numbers=True, **kw)
        rows, raws, gerrs, totals, block_errs, numbers = (x.cpu().numpy() for x in out)
        k = len(want)
        assert totals.tolist()[:3] == [k, k, 0] and not block_errs.any() and not gerrs.any(), pattern
        assert numbers[:k].tolist() == want and (numbers[k:] == -1).all(), pattern
        for j, i in enumerate(want):
            assert bytes(rows[j, :raws[j]]) == lines[i][:width], (pattern, j)
        totals, errs = codec.count_records(*args, pattern, **kw)
        assert totals.cpu().tolist() == [k, 0, 0, 0]
    one = codec.find_records(*args, AllOf(b"ERROR"), max_records=n)          # one item: the call of the item alone
    lit = codec.find_records(*args, b"ERROR", max_records=n)
    k = int(lit[2][1])
    assert len(one) == len(lit) == 5 and k > 0 and torch.equal(one[2], lit[2]) and torch.equal(one[3], lit[3])
    assert torch.equal(one[0][:k], lit[0][:k]) and torch.equal(one[1][:k], lit[1][:k])
    near = codec.find_records(*args, Seq(b"ERROR", b"cache"), max_records=n, context=1, line_numbers=True)
    assert len(near) == 7 and int(near[2][0]) == int(near[2][1]) > int(near[6][:int(near[2][1])].sum()) > 0
    with pytest.raises(TypeError):
        codec.find_pattern(*args, AllOf(b"ERROR", b"cache"))
    with pytest.raises(ValueError):
        codec.grep(*args, Seq(b"ERROR", b"cache"), 4, 16, word=True)


# ---- 14: no blocks -------------------------------------------------------------------------------------------------------------
def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    nbuf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    sbuf = torch.full((4,), GUARD8, dtype=torch.uint8, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    for pattern in (AllOf(b"error", b"x"), Seq(b"error", AnyOf(b"x", b"y"), b"zz")):
        for kw in (dict(), dict(context=2), dict(before=1, invert=True), dict(after=1, line_numbers=True)):
            widens = any(k in kw for k in ("context", "before", "after"))
            out = (buf, lbuf) + ((nbuf,) if kw.get("line_numbers") else ()) + ((sbuf,) if widens else ())
            res = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, pattern, max_records=4, block_counts=True, out=out, **kw)
            assert res[2].cpu().tolist() == [0, 0, 0, 0] and res[3].numel() == 0 and res[4].numel() == 0
            assert len(res) == 5 + bool(kw.get("line_numbers")) + widens
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4 and nbuf.cpu().tolist() == [GUARD64] * 4
    assert sbuf.cpu().tolist() == [GUARD8] * 4

"""GPU tests of hufgpu_find_records_context (GpuCodec.find_records / count_records / grep with `before`, `after`, `context`):
grep -A / -B / -C - the records around the selected ones - from the masks of the one walk, enqueue-only.

Bit-exact, no tolerance.  Expected values come from tests/find_context_model.py (itself checked against plain Python over
`bytes.split` in tests/test_find_context_args.py).  As in tests/test_gpu_find_select.py every output buffer - starts, lengths,
numbers and flags - has guard words in front and behind and is filled with the guard first: the words beyond totals[1] must
still hold it.  The four shapes are those of tests/test_gpu_find_classes.py: five blocks of 4 099 bytes (tiles of 2 048, 2 048
and 3 symbols), 300 blocks of 64 bytes (300 tiles: two scan groups), 200 blocks of 3 bytes, one block of 3 x 65 536 + 77 bytes
(three chunks).
"""
import re

import numpy as np
import pytest

import find_support
from find_context_model import find_context_model
from find_records_model import find_records_model
from find_select_model import NO_UNKNOWN, find_select_model
from find_support import (CHUNK, FOUR_SHAPES, GUARD8, GUARD32, GUARD64, LEAD, NL, OK, RW, SEAMS, TAIL, TILE, AnyOf, base_without, check,
                          codec, context, damaged, encode, literal, pattern_below_255, payload_start, planted, runs_input, same_arrays,
                          select, torch_mod, with_delimiters)
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

FAR = 2**32 - 1
DISTANCES = [(0, 1), (1, 0), (2, 2), (0, 5), (7, 0), (3, 40), (FAR, FAR)]


# ---- the checks --------------------------------------------------------------------------------------------------------------
def context_exact(torch, codec, enc, alts, delims=b"\n", before=0, after=0, invert=False, room=5, max_len=0, what="", sub=None, all_served=True):
    """the answer without outputs and with all four, each equal to the model's for the blocks with status 0; returns (the
    model's answer at a cap that holds every record, the statuses)"""
    kw = dict(invert=invert, before=before, after=after)
    full, _, errs = find_support.exact_answer(lambda cap: context(torch, codec, enc, alts, delims, cap, max_len, sub=sub, **kw),
                                       lambda cap, served: find_context_model(enc.data, alts, delims, enc.bs, cap, max_len, served, **kw),
                                       enc.n, room=room, what=(what, before, after, invert), all_served=all_served,
                                       probe=lambda: context(torch, codec, enc, alts, delims, 0, numbers=False, flags=False, sub=sub, **kw))
    return full, errs


# ---- 1: the identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_no_distance_and_no_flags_is_the_select_call(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES[shape]
    words = [pattern_below_255(5, 401), pattern_below_255(2, 402)]
    data = with_delimiters(base_without(n, 181), [p - 1 for p in SEAMS[shape]] + [n - 1])
    for i, s in enumerate(SEAMS[shape]):                    # (every third seam's record holds neither word)
        data = planted(data, words[i % 2], [s + 2 + i % 3] if i % 3 and s + 10 < n else [])
    enc = encode(torch, codec, data, bs)
    alts = [literal(w) for w in words]
    for invert in (False, True):
        for numbers in (True, False):
            for cap, max_len, counts in ((n, 0, True), (3, 7, False), (0, 0, True)):
                got = context(torch, codec, enc, alts, b"\n", cap, max_len, invert=invert, numbers=numbers, flags=False, counts=counts)
                older = select(torch, codec, enc, alts, b"\n", cap, max_len, invert=invert, numbers=numbers, counts=counts)
                assert got[6] is None and same_arrays(got[:6], older), (shape, invert, numbers, cap)
                assert int(got[2][0]) > 0
    res = context(torch, codec, enc, alts, b"\n", n)        # no distance, but the flags: every reported record is selected
    check(res, find_context_model(data, alts, b"\n", bs, n), n, shape)
    total = int(res[2][0])
    assert total > 0 and res[6][LEAD:LEAD + total].all()


# ---- 2: one selected record at every seam ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ba", [(1, 1), (3, 3)], ids=["1-1", "3-3"])
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_a_window_across_every_seam(torch_mod, codec, shape, ba):
    """a record of four bytes that holds the word starts at every seam p of the shape, records of four bytes on both sides:
    the window crosses the edge of a lane's word, a tile, a chunk, a block and a scan group.  Three ways that rotate through
    the seams: plain; a second delimiter at p - 2 (an empty record just in front of the seam: it is counted, so the window
    reaches one record less far); one at p + 5 (an empty record just behind)"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    word = pattern_below_255(2, 410)
    for rot in range(3):
        nl, at = [], []
        for k, p in enumerate(SEAMS[shape]):
            nl += [q for q in [p - 1 - 5 * j for j in range(5)] + [p + 4 + 5 * j for j in range(5)] if 0 <= q < n]
            way = (k + rot) % 3
            if way == 1 and p >= 2:
                nl.append(p - 2)
            if way == 2 and p + 5 < n:
                nl.append(p + 5)
            if p + 3 < n:
                at.append(p + 1)
        data = planted(with_delimiters(base_without(n, 182 + rot), nl), word, at)
        enc = encode(torch, codec, data, bs)
        full, _ = context_exact(torch, codec, enc, [literal(word)], before=ba[0], after=ba[1], what=(shape, rot))
        sel = set(full[0][full[5] == 1].tolist())
        assert {a - 1 for a in at} <= sel and int(full[3][0]) > len(sel) > 0, (shape, rot)
        assert full[4].tolist() == [bytes(data[:s]).count(b"\n") for s in full[0].tolist()]


# ---- 3: distances through tiles without a selected record --------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_context_three_tiles_away(torch_mod, codec, shape):
    """long records: the hit's neighbours start three tiles in front of it and end three tiles behind it, and no tile between
    holds a selected record"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    tile = min(bs or TILE, TILE)
    a0 = {"5x4099": 1000, "300x64": 250 * 64 + 9, "3chunks": CHUNK - 3 * TILE - 500}[shape]
    h0 = a0 + 3 * tile + 10
    b0 = h0 + 30
    b1 = b0 + 3 * tile + 20
    word = pattern_below_255(5, 420)
    data = planted(with_delimiters(base_without(n, 186), [a0 - 1, h0 - 1, b0 - 1, b1, b1 + 50]), word, [h0 + 7])
    enc = encode(torch, codec, data, bs)
    for ba, want in (((1, 1), [a0, h0, b0]), ((1, 0), [a0, h0]), ((0, 1), [h0, b0]), ((0, 2), [h0, b0, b1 + 1]), ((2, 0), [0, a0, h0])):
        full, _ = context_exact(torch, codec, enc, [literal(word)], before=ba[0], after=ba[1], what=shape)
        assert full[0].tolist() == want and full[5].tolist() == [int(s == h0) for s in want], (shape, ba)


@pytest.mark.parametrize("shape", ["5x4099", "300x64", "3chunks"])
def test_a_window_of_forty_records_over_several_tiles(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    step = 7 if shape == "300x64" else 150                  # 40 records: 280 bytes of 64-byte tiles, 6 000 of 2 048-byte ones
    word = pattern_below_255(3, 430)
    nl = np.arange(step - 1, n, step)
    hits = [step * 70 + 2, step * 100 + 2, n - step * 20 + 2 - n % step]
    data = planted(with_delimiters(base_without(n, 187), nl), word, hits)
    enc = encode(torch, codec, data, bs)
    for ba in ((40, 40), (3, 40), (40, 0)):
        full, _ = context_exact(torch, codec, enc, [literal(word)], before=ba[0], after=ba[1], what=shape)
        assert int(full[3][0]) > 40 and int(full[5].sum()) == 3


@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_one_record_over_all_blocks(torch_mod, codec, shape):
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES[shape]
    word = pattern_below_255(2, 440)
    for plants in ([], [n - 2]):
        enc = encode(torch, codec, planted(base_without(n, 188), word, plants), bs)
        for delims in (b"", b"\n"):
            for ba in ((1, 1), (FAR, FAR)):
                for invert in (False, True):
                    full, _ = context_exact(torch, codec, enc, [literal(word)], delims, ba[0], ba[1], invert, what=(shape, len(plants)))
                    if bool(plants) != invert:
                        assert [x.tolist() for x in full[:2]] == [[0], [n]] and full[4].tolist() == [0] and full[5].tolist() == [1]
                    else:
                        assert full[3].tolist() == [0, 0, 0, 0]


# ---- 4: dense random data ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ba", DISTANCES, ids=lambda ba: "%d-%d" % ba if ba[0] < FAR else "all")
@pytest.mark.parametrize("shape", list(FOUR_SHAPES))
def test_dense_random_data(torch_mod, codec, shape, ba):
    bs, n, _ = FOUR_SHAPES[shape]
    rng = np.random.default_rng(178)
    letters = np.frombuffer(b"abc", np.uint8)
    data = rng.choice(np.frombuffer(b"abc\n", np.uint8), n, p=[0.31, 0.31, 0.31, 0.07]).astype(np.uint8)
    enc = encode(torch_mod, codec, data, bs)
    every = find_select_model(data, [[b"abc"]], b"\n", bs, n)[0]       # every non-empty record
    sizes = []
    for trial in range(3):
        alts = [[bytes(rng.choice(letters, int(rng.integers(1, 3)), replace=False).astype(np.uint8)) for _ in range(int(rng.integers(3, 7)))]
                for _ in range(int(rng.integers(1, 7)))]
        for invert in (False, True):
            full, _ = context_exact(torch_mod, codec, enc, alts, before=ba[0], after=ba[1], invert=invert, what=(shape, trial, alts))
            sizes.append((int(full[3][0]), int(full[5].sum())))
            if ba == (FAR, FAR) and sizes[-1][1]:
                assert np.array_equal(full[0], every)
    assert any(t > s > 0 for t, s in sizes), sizes


# ---- 5: one-symbol blocks ----------------------------------------------------------------------------------------------------
def test_one_symbol_blocks_between_ordinary_ones(torch_mod, codec):
    """200 x 3: blocks of three delimiters - three empty records each, counted and not reported - and of a leaf that is in no
    class, between ordinary blocks"""
    torch = torch_mod
    bs, n, _ = FOUR_SHAPES["200x3"]
    data = base_without(n, 189)
    data[data == 41] = 42
    data = with_delimiters(data, np.arange(4, n, 9))        # (the one-symbol blocks below overwrite what falls into them)
    for b in range(5, 190, 20):
        data[b * bs:(b + 1) * bs] = NL                      # three empty records
        data[(b + 7) * bs:(b + 8) * bs] = 41                # a leaf that is in no class
    word = pattern_below_255(2, 450)
    data = planted(data, word, [3 * 40 + 1 + 60 * k for k in range(8)])     # blocks 40, 60, ...: none of those
    assert sum(np.unique(data[o:o + bs]).size == 1 for o in range(0, n - 2, bs)) >= 20
    enc = encode(torch, codec, data, bs)
    for ba in ((1, 1), (2, 2), (0, 5), (7, 0)):
        for invert in (False, True):
            full, _ = context_exact(torch, codec, enc, [literal(word)], before=ba[0], after=ba[1], invert=invert, what="200x3")
            assert full[4].tolist() == [bytes(data[:s]).count(b"\n") for s in full[0].tolist()]
            assert (full[1] > 0).all() and 0 < int(full[5].sum()) < full[5].size
    narrow = find_context_model(data, [literal(word)], b"\n", bs, n, before=2, after=2)
    assert np.diff(narrow[4]).max() > 3                     # the numbers jump over the empty records


# ---- 6: blocks that are not served -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["a payload bit", "block_len"])
def test_a_block_that_is_not_served(torch_mod, codec, damage):
    """S is what the select call gives, no context is reported across the block, numbers are exact in front of it and unknown
    behind, totals[2] is as before"""
    torch = torch_mod
    enc, delim, alts = runs_input(torch, codec)
    bs, n = enc.bs, enc.n
    whole = {ba: context_exact(torch, codec, enc, alts, delim, ba[0], ba[1], what="undamaged")[0] for ba in ((2, 2), (0, 5), (7, 0))}
    for b in range(5):
        if damage == "a payload bit":
            bad = damaged(enc, payload_start(enc, b) + (2 * 3000) // 8, 0x80 >> ((2 * 3000) % 8))
        else:
            bad = damaged(enc, int(enc.h_offs[b]), 0x01)
        for ba in whole:
            for invert in (False, True):
                full, errs = context_exact(torch, codec, bad, alts, delim, ba[0], ba[1], invert, what=(damage, b), all_served=False)
                assert errs.tolist() == [RW if j == b else OK for j in range(5)], (damage, b, errs)
                sel = select(torch, codec, bad, alts, delim, n, invert=invert)
                k = int(sel[2][0])
                assert int(full[3][2]) == 1 == int(sel[2][2])
                assert full[0][full[5] == 1].tolist() == sel[0][LEAD:LEAD + k].tolist()
                front = full[0] < b * bs
                assert full[4][front].tolist() == [bytes(enc.data[:s]).count(delim) for s in full[0][front].tolist()]
                assert (full[4][~front] == NO_UNKNOWN).all()
                if not invert:
                    assert set(full[0].tolist()) <= set(whole[ba][0].tolist())
                for s, f in zip(full[0].tolist(), full[5].tolist()):      # a context record has a selected one on its side
                    assert f or any((m < b * bs) == (s < b * bs) for m in full[0][full[5] == 1].tolist()), (b, ba, s)


@pytest.mark.parametrize("sub", ["zeros", "random"])
def test_sub_index_abuse(torch_mod, codec, sub):
    torch = torch_mod
    bs = 4096
    word = pattern_below_255(6, 460)
    data = planted(base_without(5 * bs + 1500, 190), word, [100, bs - 3, 2 * bs + 2045, 5 * bs + 1494])
    data = with_delimiters(data, np.arange(37, data.size, 601))
    enc = encode(torch, codec, data, bs)
    rng = np.random.default_rng(134)
    other = torch.zeros_like(enc.sub) if sub == "zeros" else torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()
    alts = [literal(word), literal(word[:2])]
    context_exact(torch, codec, enc, alts, before=2, after=2, what="own")
    _, errs = context_exact(torch, codec, enc, alts, before=2, after=2, sub=other, max_len=9, what=sub, all_served=False)
    assert sub == "random" or errs.all()
    bad = damaged(enc, int(enc.h_offs[1]), 0x01)
    context_exact(torch, codec, bad, [literal(word)], before=3, after=1, sub=other, what=(sub, "and a damaged block"), all_served=False)
    context_exact(torch, codec, bad, [literal(word)], before=FAR, after=FAR, what="a damaged block, every distance", all_served=False)


# ---- 7: caps and lengths -----------------------------------------------------------------------------------------------------
def test_caps_and_lengths(torch_mod, codec):
    torch = torch_mod
    bs, n = 4099, 5 * 4099
    word = pattern_below_255(5, 470)
    nl = [99, 2047, bs - 1, bs + 3000, 2 * bs + 4096, 3 * bs + 10, 4 * bs + 4000]
    data = planted(with_delimiters(base_without(n, 191), nl), word, [2100, n - 5])
    enc = encode(torch, codec, data, bs)
    alts = [literal(word)]
    for invert in (False, True):
        kw = dict(invert=invert, before=1, after=1)
        full = find_context_model(data, alts, b"\n", bs, n, **kw)
        total, lens = int(full[3][0]), full[1].tolist()
        assert 2 < total and 0 < int(full[5].sum()) < total
        for cap in (0, 1, total - 1, total):
            for counts in (True, False):
                for numbers in (True, False):
                    for flags in (True, False):             # d_rec_sel without d_rec_no, and the reverse
                        res = context(torch, codec, enc, alts, b"\n", cap, numbers=numbers, flags=flags, counts=counts, **kw)
                        assert int(res[2][0]) == total and not res[3].any()
                        check(res, find_context_model(data, alts, b"\n", bs, cap, **kw), cap, (invert, cap, counts, numbers, flags))
        for max_len in sorted({1, 0} | {m + d for m in lens for d in (-1, 0, 1)}):        # below, at and above every length
            for cap in (total, 2):
                res = context(torch, codec, enc, alts, b"\n", cap, max_len, **kw)
                check(res, find_context_model(data, alts, b"\n", bs, cap, max_len, **kw), cap, (invert, max_len, cap))
                if cap == total:
                    assert int(res[2][3]) == sum(l > max_len for l in lens) * bool(max_len)


# ---- 8: one context, call after call -----------------------------------------------------------------------------------------
def test_calls_back_to_back(torch_mod, codec):
    """context, select, find_records, context with other distances, ... without a synchronise in between: each gives its own
    model's answer, so the second mask and its scan are the call's own each time"""
    torch = torch_mod
    bs, n, starts = FOUR_SHAPES["5x4099"]
    word = pattern_below_255(6, 480)
    nl = sorted(set(range(40, n, 333)) | {bs, 2 * bs + 2100})
    data = planted(with_delimiters(base_without(n, 192), nl), word, [s for s in starts if s + 6 < n])
    enc = encode(torch, codec, data, bs)
    jobs = [dict(context=2), dict(invert=True), dict(), dict(before=1, after=5, invert=True, line_numbers=True), dict(line_numbers=True),
            dict(context=2), dict(), dict(before=7)]

    def model(kw, cap):
        if not kw:
            return find_records_model(data, word, b"\n", bs, cap)
        b, a = (kw["context"],) * 2 if "context" in kw else (kw.get("before", 0), kw.get("after", 0))
        return find_context_model(data, [literal(word)], b"\n", bs, cap, 0, None, kw.get("invert", False), b, a)

    bufs = []
    for kw in jobs:
        want = model(kw, n)
        cap = int(want[3][0]) + 2
        assert cap > 2
        bufs.append((cap, [torch.full((LEAD + cap + TAIL,), g, dtype=t, device="cuda")
                           for g, t in ((GUARD64, torch.int64), (GUARD32, torch.int32), (GUARD64, torch.int64), (GUARD8, torch.uint8))]))
    torch.cuda.synchronize()
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    res = []
    for kw, (cap, (pbuf, lbuf, nbuf, sbuf)) in zip(jobs, bufs):
        widens = any(k in kw for k in ("context", "before", "after"))
        out = [pbuf[LEAD:LEAD + cap], lbuf[LEAD:LEAD + cap]] + ([nbuf[LEAD:LEAD + cap]] if kw.get("line_numbers") else []) + \
              ([sbuf[LEAD:LEAD + cap]] if widens else [])
        res.append(codec.find_records(*args, word, b"\n", max_records=cap, block_counts=True, out=out, **kw))
    torch.cuda.synchronize()
    host = []
    for kw, (cap, (pbuf, lbuf, nbuf, sbuf)), r in zip(jobs, bufs, res):
        widens = any(k in kw for k in ("context", "before", "after"))
        numbers = bool(kw.get("line_numbers"))
        assert len(r) == 5 + numbers + widens
        got = (pbuf.cpu().numpy(), lbuf.cpu().numpy(), r[2].cpu().numpy(), r[3].cpu().numpy(), r[4].cpu().numpy(),
               nbuf.cpu().numpy() if numbers else None, sbuf.cpu().numpy() if widens else None)
        if kw:
            if widens:
                assert r[-1].data_ptr() == sbuf[LEAD:].data_ptr() and r[-1].dtype == torch.uint8
            check(got, model(kw, cap), cap, kw)
        else:
            check(got[:5], model(kw, cap), cap, kw)
        if not numbers:
            assert (nbuf.cpu().numpy() == GUARD64).all()
        if not widens:
            assert (sbuf.cpu().numpy() == GUARD8).all()
        host.append(got)
    assert same_arrays(host[0], host[5]) and same_arrays(host[2], host[6])


# ---- 9: Python ---------------------------------------------------------------------------------------------------------------
def test_grep_with_context_and_line_numbers(torch_mod, codec):
    """grep(b"ERROR", ..., context=2, line_numbers=True) without a synchronisation, against an `re` filter over
    data.split(b"\\n"): rows, numbers and flags"""
    torch = torch_mod
    n, bs = (1 << 18) + 1, 65536
    data = datagen.logtext(n)
    lines = bytes(data).split(b"\n")
    hits = [i for i, l in enumerate(lines) if re.search(rb"ERROR", l)]
    near = sorted({j for i in hits for j in range(max(i - 2, 0), min(i + 2, len(lines) - 1) + 1) if lines[j]})
    assert 0 < len(hits) < len(near) < sum(1 for l in lines if l)
    enc = encode(torch, codec, data, bs)
    cap, width = len(near) + 5, 256
    args = (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs)
    out = codec.grep(*args, b"ERROR", cap, width, context=2, line_numbers=True)
    assert len(out) == 7
    rows, raws, gerrs, totals, block_errs, numbers, selected = (x.cpu().numpy() for x in out)
    k = len(near)
    assert totals.tolist() == [k, k, 0, sum(len(lines[i]) > width for i in near)] and not block_errs.any() and not gerrs.any()
    assert numbers[:k].tolist() == near and (numbers[k:] == -1).all() and numbers.dtype == np.int64
    assert selected.dtype == np.uint8 and selected[:k].tolist() == [int(i in set(hits)) for i in near] and not selected[k:].any()
    for j, i in enumerate(near):
        assert raws[j] == min(len(lines[i]), width) and bytes(rows[j, :raws[j]]) == lines[i][:width], j
    assert not raws[k:].any()
    assert len(codec.grep(*args, b"ERROR", cap, width)) == 5 and len(codec.grep(*args, b"ERROR", cap, width, context=0)) == 5
    after = sorted({j for i in hits for j in range(i, min(i + 3, len(lines) - 1) + 1) if lines[j]})
    rows, raws, gerrs, totals, block_errs, selected = (x.cpu().numpy() for x in codec.grep(*args, b"ERROR", cap + 50, width, after=3))
    assert int(totals[0]) == len(after) and int(selected.sum()) == len(hits)
    totals, errs, selected = codec.count_records(*args, b"ERROR", before=1)
    before = {j for i in hits for j in (i - 1, i) if j >= 0 and lines[j]}
    assert totals.cpu().tolist() == [len(before), 0, 0, 0] and selected.numel() == 0
    quiet = [i for i, l in enumerate(lines) if l and not re.search(rb"INFO|DEBUG", l)]
    want = sorted({j for i in quiet for j in range(max(i - 1, 0), min(i + 1, len(lines) - 1) + 1) if lines[j]})
    pos, lens, totals, errs, _, numbers, selected = codec.find_records(*args, AnyOf(b"INFO", b"DEBUG"), max_records=len(want), context=1,
                                                                       invert=True, line_numbers=True)
    assert numbers.cpu().tolist() == want and selected.cpu().tolist() == [int(i in set(quiet)) for i in want]
    for kw in (dict(context=1, before=1), dict(after=-1), dict(context=2**32)):
        with pytest.raises(ValueError):
            codec.grep(*args, b"ERROR", 4, 16, **kw)


# ---- 10: no blocks -----------------------------------------------------------------------------------------------------------
def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    lbuf = torch.full((4,), GUARD32, dtype=torch.int32, device="cuda")
    nbuf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    sbuf = torch.full((4,), GUARD8, dtype=torch.uint8, device="cuda")
    sub = codec.new_sub_index(0, 4096)
    for kw in (dict(context=2), dict(before=FAR, invert=True), dict(after=1, line_numbers=True)):
        out = (buf, lbuf, nbuf, sbuf) if kw.get("line_numbers") else (buf, lbuf, sbuf)
        res = codec.find_records(empty, 0, offsets, 0, sub, 0, 4096, AnyOf(b"error", b"x"), max_records=4, block_counts=True, out=out, **kw)
        assert res[2].cpu().tolist() == [0, 0, 0, 0] and res[3].numel() == 0 and res[4].numel() == 0
        assert len(res) == 6 + bool(kw.get("line_numbers")) and res[-1].data_ptr() == sbuf.data_ptr()
    assert buf.cpu().tolist() == [GUARD64] * 4 and lbuf.cpu().tolist() == [GUARD32] * 4 and nbuf.cpu().tolist() == [GUARD64] * 4
    assert sbuf.cpu().tolist() == [GUARD8] * 4

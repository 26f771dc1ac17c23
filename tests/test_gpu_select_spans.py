"""GPU tests of hufgpu_select_spans and of GpuCodec.select_spans / find_matches / count_matches / extract and
redact(nonoverlapping=True): every case bit for bit against tests/select_spans_model.py, with guard words around d_sel_pos,
d_sel_len, d_sel_rank, the totals and the count word.  The sizes come from hufgpu_select_geometry: with T ranks a tile and F
tiles a composition group they lie at the successor window (63, 64, 65), around one tile (T - 1 ... T + 64: the halo), two
tiles, one group of tiles (F T - 1 ... F T + 1: a second map on level 1) and F F + 1 tiles (a second map on level 2).
"""
import ctypes as C
import re

import numpy as np
import pytest

from find_expr_support import arrays, lit, rep
from find_model import byte_set
from find_spans_model import find_spans_model
from find_support import CHUNK, GUARD8, GUARD32, GUARD64, LEAD, OK, TAIL, TILE, W, codec, damaged, encode, payload_start, torch_mod  # noqa: F401
from libhuffman_amd import _native, datagen
from libhuffman_amd.codec import GpuCodec, HuffmanGpuError
from select_spans_model import HUFE_ARGUMENT, select_model
from test_select_spans_args import plain_loop

pytestmark = pytest.mark.gpu
PAD = _native.SELECT_PAD
NLB = b"\n"


def geometry(codec):
    return codec.select_geometry()


def dev64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.uint64).view(np.int64))).cuda()


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()


def select_enqueue(torch, codec, pos, lens, sel_cap, n=None, pad=None, ranks=True, stream=None, d_in=None):
    """one call with guarded buffers; the device tensors, without a wait.  `n`: the value of the count word (None: d_n is
    NULL); `pad`: pad_pos, with the flag (None: no flag); `d_in`: (d_pos, d_len) already on the device"""
    n_cap = len(pos)
    d_pos, d_len = d_in or (dev64(torch, pos if n_cap else [0]), dev32(torch, lens if n_cap else [0]))
    full = lambda g, dt: torch.full((LEAD + sel_cap + TAIL,), g, dtype=dt, device="cuda")        # noqa: E731
    pbuf, lbuf, rbuf = full(GUARD64, torch.int64), full(GUARD32, torch.int32), full(GUARD64, torch.int64)
    totals = torch.full((4 + 2,), GUARD64, dtype=torch.int64, device="cuda")
    word = None if n is None else torch.tensor([GUARD64, n, GUARD64], dtype=torch.int64, device="cuda")
    at = lambda b: b[LEAD:].data_ptr() if sel_cap else None          # noqa: E731
    rc = codec.lib.hufgpu_select_spans(codec._ctx, d_pos.data_ptr(), d_len.data_ptr(), None if word is None else word[1:].data_ptr(), n_cap,
                                       at(pbuf), at(lbuf), at(rbuf) if ranks else None, sel_cap, pad or 0, totals[1:].data_ptr(),
                                       PAD if pad is not None else 0, C.c_void_p(stream.cuda_stream) if stream is not None else codec._stream())
    codec._check(rc, "Failed to enqueue the selection")
    return pbuf, lbuf, rbuf, totals, word, (d_pos, d_len)


def check(res, want, sel_cap, pad=None, ranks=True, what=""):
    """every output and every guard word against the model's (positions, lengths, ranks, totals)"""
    pbuf, lbuf, rbuf, totals, word = (None if t is None else t.cpu().numpy() for t in res[:5])
    pos, lens, rk, tot = want
    assert totals[[0, 5]].tolist() == [GUARD64] * 2 and totals[1:5].tolist() == tot.tolist(), (what, totals, tot)
    assert word is None or word[[0, 2]].tolist() == [GUARD64] * 2, what
    w = int(tot[1])
    assert w == len(pos) <= sel_cap
    rows = {"pos": (pbuf, GUARD64, pos.view(np.int64), pad), "len": (lbuf, GUARD32, lens, 0), "rank": (rbuf, GUARD64, rk if ranks else rk[:0], None)}
    for name, (buf, guard, model, padding) in rows.items():
        expect = np.full(buf.size, guard, buf.dtype)
        expect[LEAD:LEAD + len(model)] = model
        if pad is not None and padding is not None:
            expect[LEAD + w:LEAD + sel_cap] = padding
        bad = np.flatnonzero(buf != expect)
        assert bad.size == 0, (what, name, "differ at", bad[:8] - LEAD, buf[bad[:8]], expect[bad[:8]])


KINDS = ("ones", "all-64", "all-63", "random", "gaps", "mixed", "cross-2^32")


def spans_of(kind, n, seed=0):
    """(positions uint64, lengths int32) of n spans"""
    rng = np.random.default_rng(1000 * seed + n % 997 + len(kind))
    step = np.ones(n, np.uint64)
    if kind == "gaps":                                              # every rank is selected
        step = rng.integers(64, 200, n).astype(np.uint64)
    elif kind in ("mixed", "cross-2^32"):                           # runs of neighbours and gaps
        step = np.where(rng.integers(0, 5, n) == 0, rng.integers(2, 300, n), 1).astype(np.uint64)
    base = (1 << 32) - n // 2 - 3 if kind == "cross-2^32" else 7
    pos = np.uint64(base) + np.cumsum(step) - step[:1] if n else np.zeros(0, np.uint64)
    lens = {"ones": np.ones(n), "all-64": np.full(n, 64), "all-63": np.full(n, 63), "33-64": rng.integers(33, 65, n)}.get(kind)
    lens = rng.integers(1, 65, n) if lens is None else lens
    return pos.astype(np.uint64), lens.astype(np.int32)


def sizes(codec):
    T, F = geometry(codec)
    return [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, T + 63, T + 64, 2 * T + 1, F * T - 1, F * T, F * T + 1]


@pytest.mark.parametrize("kind", KINDS)
def test_the_selection_against_the_model(torch_mod, codec, kind):
    """every size, d_n NULL; pads and ranks in turn"""
    for k, n in enumerate(sizes(codec)):
        pos, lens = spans_of(kind, n)
        want = select_model(pos, lens)
        selected = int(want[3][0])
        if kind in ("ones", "gaps"):
            assert selected == n
        if kind == "cross-2^32" and n > 8:
            assert pos[0] < 1 << 32 < pos[-1]
        cap = selected + 3
        pad, ranks = (pos[-1] + 100 if n else 5) if k % 2 else None, k % 3 != 0
        res = select_enqueue(torch_mod, codec, pos, lens, cap, pad=None if pad is None else int(pad), ranks=ranks)
        check(res, want, cap, None if pad is None else int(pad), ranks, (kind, n))


def test_all_63_cycles_through_the_entry_offsets(codec):
    """the model's own answer: with 63 bytes a span on consecutive positions the tiles are entered at every residue"""
    T, F = geometry(codec)
    pos, lens = spans_of("all-63", F * T + 1)
    ranks = select_model(pos, lens)[2]
    entries = {int(r[0]) % T for r in np.split(ranks, np.searchsorted(ranks, np.arange(T, F * T + 1, T))) if r.size}
    assert len(entries) >= min(63, F) - 1 and max(entries) <= 63


def test_more_tiles_than_two_levels_of_groups(torch_mod, codec):
    """(F F + 1) T ranks: a second map on the third level.  Lengths 33 to 64 on consecutive positions keep the model's walk short"""
    T, F = geometry(codec)
    n = (F * F + 1) * T
    pos, lens = spans_of("33-64", n)
    want = select_model(pos, lens)
    cap = int(want[3][0]) + 3
    assert n // 64 <= cap <= n // 33 + 4
    check(select_enqueue(torch_mod, codec, pos, lens, cap, pad=int(pos[-1]) + 1), want, cap, int(pos[-1]) + 1, True, "three levels")


def test_the_count_word(torch_mod, codec):
    """*d_n below n_cap with garbage behind rank n that breaks order and lengths: it is not read and raises no status; *d_n
    above n_cap counts as n_cap; *d_n = 0"""
    T, _ = geometry(codec)
    for n_cap, n in ((T + 100, T + 7), (T + 100, T), (2 * T + 5, 3), (3 * T, T + 64), (T, 0), (T + 9, T + 9 + 1000), (70, 69)):
        pos, lens = spans_of("mixed", n_cap, seed=3)
        live = min(n, n_cap)
        pos[live:] = np.arange(n_cap - live, 0, -1, dtype=np.uint64)          # descending, below everything in front
        lens[live:] = np.where(np.arange(n_cap - live) % 2, 0, 999)
        want = select_model(pos, lens, n=n)
        assert want[3][2] == 0
        cap = int(want[3][0]) + 2
        check(select_enqueue(torch_mod, codec, pos, lens, cap, n=n, pad=12345), want, cap, 12345, True, ("d_n", n_cap, n))


def test_caps_pads_and_ranks(torch_mod, codec):
    T, _ = geometry(codec)
    pos, lens = spans_of("mixed", 2 * T + 77, seed=5)
    selected = int(select_model(pos, lens)[3][0])
    assert selected > 100
    for cap in (0, 1, selected - 1, selected, selected + 6):
        want = select_model(pos, lens, cap=cap)
        for pad in (None, 1 << 40):
            for ranks in (True, False):
                check(select_enqueue(torch_mod, codec, pos, lens, cap, pad=pad, ranks=ranks), want, cap, pad, ranks, ("cap", cap, pad, ranks))


def test_invalid_input_raises_the_status_and_writes_no_row(torch_mod, codec):
    T, _ = geometry(codec)
    n = 2 * T + 50

    def broken(change):
        pos, lens = spans_of("mixed", n, seed=9)
        change(pos, lens)
        return pos, lens

    def equal(at):
        return lambda pos, lens: pos.__setitem__(at, pos[at - 1])

    def lower(at):
        return lambda pos, lens: pos.__setitem__(slice(at, None), pos[at:] - (pos[at] - pos[at - 1]) - np.uint64(5))

    def length(at, value):
        return lambda pos, lens: lens.__setitem__(at, value)

    def several(pos, lens):
        lens[T + 300], lens[5] = 0, 65
        pos[T + 3] = pos[T + 2]

    cases = {"equal neighbours": (equal(700), 700), "equal at rank 1": (equal(1), 1), "descending across a tile edge": (lower(T), T),
             "equal across a tile edge": (equal(T), T), "length 0": (length(T + 9, 0), T + 9), "length 65": (length(3, 65), 3),
             "length 0 at rank 0": (length(0, 0), 0), "a huge length": (length(n - 1, -1), n - 1), "several: the lowest": (several, 5)}
    for what, (change, rank) in cases.items():
        pos, lens = broken(change)
        want = select_model(pos, lens)
        assert want[3].tolist() == [0, 0, HUFE_ARGUMENT, rank], (what, want[3])
        for pad in (None, 999):
            check(select_enqueue(torch_mod, codec, pos, lens, 40, pad=pad), want, 40, pad, True, (what, pad))
    # the offender behind the count word is nobody's business
    pos, lens = broken(equal(T + 5))
    check(select_enqueue(torch_mod, codec, pos, lens, n, n=T + 5), select_model(pos, lens, n=T + 5), n, None, True, "behind n")
    # the Python layer names the rank
    p, l, _, totals = codec.select_spans(dev64(torch_mod, pos), dev32(torch_mod, lens))
    with pytest.raises(HuffmanGpuError, match="rank %d" % (T + 5)):
        codec.select_result(totals)


# ---- end to end through the codec ----------------------------------------------------------------------------------------------
def truth(pattern, data):
    """{start: longest length} by re.fullmatch, length by length, at every start where `re` sees a form at all; then the plain
    loop of tests/test_select_spans_args.py"""
    text, e = bytes(data), re.compile(pattern)
    spans = {}
    for p in range(len(text)):
        if e.match(text, p) is None:
            continue
        for L in range(min(64, len(text) - p), 0, -1):
            if e.fullmatch(text, p, p + L):
                spans[p] = L
                break
    return spans, plain_loop(spans, len(text))


def plant(data, pieces):
    data = np.array(data, np.uint8)
    for at, s in pieces:
        if 0 <= at and at + len(s) <= data.size:
            data[at:at + len(s)] = np.frombuffer(s, np.uint8)
    return data


LAYOUTS = {"3B": (3, 200 * 3 - 1), "4K": (4096, 5 * 4096 + 100), "chunk": (0, 2 * CHUNK + 100)}
_made = {}


def text_of(torch, codec, name):
    """digits, 'colour' / 'color' and GET / GETS at byte 0, at the end and across tile, chunk and block seams"""
    if name not in _made:
        bs, n = LAYOUTS[name]
        data = datagen.zipf255(n, seed=17).copy()
        data[(data >= ord("0")) & (data <= ord("9"))] = ord("x")
        B = bs or n
        pieces = [(0, b"1234 "), (10, b"colour color"), (30, b"GETS GET GETGETS"), (60, b"1234567 99 1"), (n - 5, b" 4567"), (200, b"colourcolor12")]
        if name != "3B":
            pieces += [(TILE - 2, b"12345"), (2 * TILE - 3, b"colour"), (B - 2, b"GETS"), (B + TILE - 1, b"987"), (3 * TILE - 4, b"color123"),
                       (CHUNK - 2, b"1234567"), (CHUNK + TILE - 3, b"GETSGET")]
        _made[name] = encode(torch, codec, plant(data, pieces), bs)
    return _made[name]


def head(enc):
    return (enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs)


def host(t):
    return t.cpu().numpy()


PATTERNS = {"digits": (GpuCodec.regex(rb"[0-9]{1,3}"), rb"[0-9]{1,3}"), "colour": (GpuCodec.regex(rb"colou?r"), rb"colou?r"),
            "gets": (GpuCodec.AnyOf(b"GET", b"GETS"), rb"GET|GETS")}


@pytest.mark.parametrize("name", LAYOUTS)
def test_find_matches_against_re(torch_mod, codec, name):
    enc = text_of(torch_mod, codec, name)
    dropped = 0
    for what, (pattern, expr) in PATTERNS.items():
        spans, want = truth(expr, enc.data)
        pos, lens, totals, ftotals, errs, ranks = codec.find_matches(*head(enc), pattern, max_positions=len(spans) + 5)
        assert codec.select_result(totals) == (len(want), len(want)) and host(ftotals).tolist() == [len(spans), len(spans), 0, 0], (name, what)
        assert not host(errs).any()
        got = list(zip(host(pos)[:len(want)].tolist(), host(lens)[:len(want)].tolist()))
        assert got == want, (name, what)
        starts = sorted(spans)
        assert [starts[r] for r in host(ranks)[:len(want)].tolist()] == [p for p, _ in want]
        dropped += len(spans) - len(want)
        ctot, cftot, _ = codec.count_matches(*head(enc), pattern, max_positions=len(spans) + 5)
        assert host(ctot).tolist() == [len(want), 0, 0, 0] and host(cftot).tolist() == host(ftotals).tolist()
    assert dropped >= 8, "no overlapping start was there to drop"
    assert (0, 3) in truth(rb"[0-9]{1,3}", enc.data)[1] and (3, 1) in truth(rb"[0-9]{1,3}", enc.data)[1]


@pytest.mark.parametrize("name", LAYOUTS)
def test_a_run_of_ten_thousand(torch_mod, codec, name):
    """'a{1,64}' over 10 000 'a': every byte is a start, and 157 matches are selected, 156 of 64 bytes and one of 16"""
    bs = LAYOUTS[name][0]
    enc = encode(torch_mod, codec, np.full(10_000, ord("a"), np.uint8), bs)
    pos, lens, totals, ftotals, _, _ = codec.find_matches(*head(enc), GpuCodec.regex(rb"a{1,64}"), max_positions=10_000)
    assert codec.select_result(totals) == (157, 157) and host(ftotals)[:3].tolist() == [10_000, 10_000, 0]
    assert host(pos)[:157].tolist() == list(range(0, 10_000, 64)) and host(lens)[:157].tolist() == [64] * 156 + [16]


def test_a_damaged_block_in_the_middle(torch_mod, codec):
    """the greedy selection over what the search reported: the spans model's answer for the served blocks"""
    enc = text_of(torch_mod, codec, "4K")
    alts = [rep(b"0123456789", 1, 3)]
    seen = 0
    for b in (2, 1, 3):
        bad = damaged(enc, payload_start(enc, b) + 3, 0x5A)
        pos, lens, totals, ftotals, errs, _ = codec.find_matches(*head(bad), GpuCodec.regex(rb"[0-9]{1,3}"), max_positions=enc.n)
        served = host(errs) == OK
        if served.all():
            continue                                                # (the flipped bits left the block decodable)
        seen += 1
        spans = find_spans_model(enc.data, alts, NLB, W, 0, enc.bs, enc.n, served)
        want = select_model(spans[0], spans[1])
        assert host(ftotals).tolist() == spans[4].tolist() and host(totals).tolist() == want[3].tolist(), b
        w = int(want[3][1])
        assert host(pos)[:w].tolist() == want[0].tolist() and host(lens)[:w].tolist() == want[1].tolist(), b
    assert seen >= 1, "no damage was noticed"


@pytest.mark.parametrize("name", LAYOUTS)
def test_extract_and_scatter_of_the_selected_rows(torch_mod, codec, name):
    torch = torch_mod
    enc = text_of(torch, codec, name)
    pattern, expr = PATTERNS["digits"]
    spans, want = truth(expr, enc.data)
    cap = len(spans) + 4
    raw = bytes(enc.data)
    slots, pos, lens, statuses, totals = codec.extract(*head(enc), pattern, cap, nonoverlapping=True)
    assert host(totals)[:2].tolist() == [len(spans), len(spans)] and not host(statuses).any()
    k = len(want)
    assert list(zip(host(pos)[:k].tolist(), host(lens)[:k].tolist())) == want
    assert (host(pos)[k:] == enc.n).all() and (host(lens)[k:] == 0).all()
    rows = host(slots)
    assert [bytes(rows[r, :want[r][1]]) for r in range(k)] == [m.group() for m in re.finditer(expr, raw)]
    # every row gets bytes of its own: were two rows to overlap, the outcome would depend on which of them wins
    new = torch.from_numpy(np.tile((np.arange(cap) % 23 + 65).astype(np.uint8)[:, None], (1, 64))).cuda()
    out, new_offsets, result, _ = codec.scatter(enc.stream, enc.length, enc.offsets, enc.nb, pos, lens, data=new, raw_size=enc.n,
                                                blocksize=enc.bs, sub_index=enc.sub, max_len=GpuCodec.SPAN_MAX)
    length, _ = codec.scatter_result(result)
    changed = enc.data.copy()
    for r, (p, n) in enumerate(want):
        changed[p:p + n] = r % 23 + 65
    ref = encode(torch, codec, changed, enc.bs)
    assert length == ref.length and torch.equal(out[:length], ref.stream[:length]) and torch.equal(new_offsets, ref.offsets)
    # redact: the same rows, blanked
    out, new_offsets, result, _, _ = codec.redact(*head(enc), pattern, b"#", max_matches=cap, spans=True, nonoverlapping=True)
    length, _ = codec.scatter_result(result)
    ref = encode(torch, codec, np.frombuffer(re.sub(expr, lambda m: b"#" * len(m.group()), raw), np.uint8), enc.bs)
    assert length == ref.length and torch.equal(out[:length], ref.stream[:length])


# ---- streams and graphs ----------------------------------------------------------------------------------------------------
def test_on_a_side_stream_behind_a_long_kernel(torch_mod, codec):
    torch = torch_mod
    T, _ = geometry(codec)
    pos, lens = spans_of("mixed", 3 * T + 11, seed=21)
    want = select_model(pos, lens)
    cap = int(want[3][0]) + 3
    for _ in range(3):                                              # call after call on one context
        check(select_enqueue(torch, codec, pos, lens, cap, pad=77), want, cap, 77, True, "again")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                                   # (the stream's first use of these kernels is not the call under test)
        d_in = select_enqueue(torch, codec, pos, lens, cap, stream=side)[5]
        side.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(10_000_000)
    t1.record()
    torch.cuda.synchronize()
    per_ms = 10_000_000 / t0.elapsed_time(t1)
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(50 * per_ms))
        opened = torch.cuda.Event()
        opened.record(side)
        res = select_enqueue(torch, codec, pos, lens, cap, pad=77, stream=side, d_in=d_in)
        closed = not opened.query()
    side.synchronize()
    assert closed, "the long kernel had ended before the call returned: this run has proved nothing"
    check(res, want, cap, 77, True, "a side stream")


def test_search_select_gather_captured_as_one_graph(torch_mod, codec):
    """hufgpu_find_any_spans -> hufgpu_select_spans(PAD) -> hufgpu_gather on buffers made outside the capture, after a first
    call has made the workspaces; replayed on other contents, with other work on the context between the replays"""
    from test_gpu_scatter import capture
    torch = torch_mod
    bs, n, cap = 4096, 3 * 4096 + 100, 64
    digits = [rep(b"0123456789", 1, 3)]
    cls, alens, n_alts, opt, _, _ = arrays([digits])
    variants = []
    for seed in (1, 2):
        d = datagen.zipf255(n, seed=40 + seed).copy()
        d[(d >= ord("0")) & (d <= ord("9"))] = ord("x")
        d = plant(d, [(50 * seed, b"1234567"), (TILE - 2, b"98765"), (4096 * seed - 1, b"12"), (n - 4 - seed, b"4321")])
        variants.append((encode(torch, codec, d, bs), truth(rb"[0-9]{1,3}", d)[1]))
    assert variants[0][1] != variants[1][1] and all(len(w) >= 8 for _, w in variants)
    room = max(v.length for v, _ in variants) + 64
    live = variants[0][0].with_stream(torch.zeros(room, dtype=torch.uint8, device="cuda"))
    live.offsets, live.sub = torch.zeros_like(live.offsets), torch.zeros_like(live.sub)
    zeros = lambda k, dt: torch.zeros(k, dtype=dt, device="cuda")    # noqa: E731
    d_pos, d_len, totals, errs = zeros(cap, torch.int64), zeros(cap, torch.int32), zeros(4, torch.int64), zeros(live.nb, torch.int32)
    s_pos, s_len, s_totals = zeros(cap, torch.int64), zeros(cap, torch.int32), zeros(4, torch.int64)
    rows, g_errs, g_lens = zeros((cap, 64), torch.uint8), zeros(cap, torch.int32), zeros(cap, torch.int32)
    s = torch.cuda.Stream()
    lib, st = codec.lib, C.c_void_p(s.cuda_stream)

    def load(v):
        live.stream[:v.length] = v.stream[:v.length]
        live.offsets.copy_(v.offsets)
        live.sub.copy_(v.sub)

    def enqueue():
        rc = lib.hufgpu_find_any_spans(codec._ctx, live.stream.data_ptr(), room, live.offsets.data_ptr(), live.nb, live.sub.data_ptr(), n, bs,
                                       cls, alens, n_alts, opt, byte_set(NLB), byte_set(W), 0, d_pos.data_ptr(), d_len.data_ptr(), None, cap,
                                       None, totals.data_ptr(), errs.data_ptr(), 0, st)
        assert rc == 0
        rc = lib.hufgpu_select_spans(codec._ctx, d_pos.data_ptr(), d_len.data_ptr(), totals[1:].data_ptr(), cap, s_pos.data_ptr(),
                                     s_len.data_ptr(), None, cap, n, s_totals.data_ptr(), PAD, st)
        assert rc == 0
        rc = lib.hufgpu_gather(codec._ctx, live.stream.data_ptr(), room, live.offsets.data_ptr(), live.nb, live.sub.data_ptr(), n, bs, cap,
                               s_pos.data_ptr(), s_len.data_ptr(), 64, rows.data_ptr(), 64, g_errs.data_ptr(), g_lens.data_ptr(), 0, st)
        assert rc == 0
        return True

    with torch.cuda.stream(s):                                      # warm-up on the stream itself: the workspaces stand
        load(variants[0][0])
        enqueue()
        s.synchronize()
    graph, _ = capture(torch, s, enqueue)
    for k, (v, want) in enumerate(variants[::-1] + variants):
        with torch.cuda.stream(s):
            load(v)
            for t in (s_totals, s_pos, s_len, rows):
                t.fill_(-1 if t.dtype != torch.uint8 else 0xEE)
            graph.replay()
            s.synchronize()
        w = len(want)
        assert host(s_totals).tolist() == [w, w, 0, 0] and not host(g_errs).any(), (k, host(s_totals))
        assert list(zip(host(s_pos)[:w].tolist(), host(s_len)[:w].tolist())) == want, k
        assert (host(s_pos)[w:] == n).all() and (host(s_len)[w:] == 0).all(), k
        got = host(rows)
        assert [bytes(got[r, :want[r][1]]) for r in range(w)] == [bytes(v.data[p:p + m]) for p, m in want], k
        assert (got[w:] == 0xEE).all(), "a pad row was written"
        encode(torch, codec, datagen.zipf255(n, seed=90 + k), bs)    # other work on the same context, of the same sizes
    del graph
    torch.cuda.synchronize()

"""Helpers of the GPU tests of the search family (tests/test_gpu_find*.py), once each: the fixtures, the guards and the
geometry, the shape tables, the input builders, ONE caller that makes the guarded output buffers, ONE checker that compares
every output and every guard word with a model's answer, and the drivers: `exact_answer` and `answer_or_not_served` for any
call, and on them the `exact` / `exact_or_not_served` pair for positions and the one for records.  Not a test module;
tests/test_find_support.py tests the checker without a device.

A result is always the 7-tuple of host arrays (starts, lengths, totals, errs, counts, numbers, flags); an output that the call
does not have, or was not given, is None.  The per-feature callers below return the part of it that their call has - the
positions calls (starts, totals, errs, counts), the records calls the first five, six or all seven - and the checker takes any
of these forms.  A model's answer is (starts, counts, totals) for positions and (starts, lengths, counts, totals[, numbers[,
flags]]) for records, as tests/find*_model.py give them.
"""
import numpy as np
import pytest

from find_calls import CALLS, invoke
from libhuffman_amd import datagen
from libhuffman_amd.codec import GpuCodec
from stream_support import GUARD, Enc, make

AnyOf = GpuCodec.AnyOf
ANY = GpuCodec.ANY
W = GpuCodec.WORD_BYTES

TILE, CHUNK = 2048, 65536
OK, RW = 0, 3
NL = 10
NOT_NL = bytes(v for v in range(256) if v != NL)
GUARD64 = int(np.array([GUARD] * 8, np.uint8).view(np.int64)[0])
GUARD32 = int(np.array([GUARD] * 4, np.uint8).view(np.int32)[0])
GUARD8 = GUARD
LEAD, TAIL = 3, 5

# ---- shapes ------------------------------------------------------------------------------------------------------------------
BIG = 3 * (1 << 20) + 77
# the byte search's: name -> (blocksize, bytes)
BYTE_SHAPES = {"bs4096": (4096, 5 * 4096 + 1500),       # two tiles a block
               "bs4099": (4099, 6 * 4099),              # every block ends in a 3-symbol group, no block start but the first is 32-aligned
               "bs65536": (65536, 3 * 65536 + 77),      # exactly one chunk a block, a short last block
               "oneblock": (0, BIG)}                    # several chunks, chunked encode
# shape -> (blocksize, bytes, starts that reach its seams: lane, tile, chunk, block, scan group; 64 bytes apart at least)
FOUR_SHAPES = {
    "5x4099": (4099, 5 * 4099, [0, 1000, 2047, 4099 + 31, 4099 + 2 * TILE - 10, 2 * 4099 + 2000, 2 * 4099 + 4096, 3 * 4099 + 2047,
                                3 * 4099 + 4098]),
    "300x64": (64, 299 * 64 + 21, [1, 5 * 64, 10 * 64 + 40, 253 * 64 + 60, 255 * 64 + 1, 270 * 64 + 63]),
    "200x3": (3, 200 * 3 - 1, [1, 70 * 3 + 2, 100 * 3]),
    "3chunks": (0, 3 * CHUNK + 77, [31, TILE - 1, CHUNK - 10, CHUNK + TILE - 4, 2 * CHUNK - 63, 2 * CHUNK + 3 * TILE - 1]),
}
# record starts at bit 0 of a lane's word, of a tile, of a chunk, of a block (behind a short last tile where the shape has
# one) and of a scan group of 256 tiles; 40 bytes apart at least
SEAMS = {
    "5x4099": [64, TILE, 4099, 4099 + 32, 4099 + TILE, 2 * 4099, 3 * 4099 + TILE, 4 * 4099, 4 * 4099 + 2 * TILE],
    "300x64": [32, 64, 5 * 64, 100 * 64 + 32, 255 * 64, 256 * 64, 257 * 64, 299 * 64],
    "200x3": [3, 48, 99, 300, 450, 597],
    "3chunks": [32, TILE, CHUNK - TILE, CHUNK, CHUNK + TILE, 2 * CHUNK, 3 * CHUNK, 3 * CHUNK + 64],
}
# a tile's end inside each shape, away from the shapes' planted starts: a short alternative is put right in front of it
TILE_END = {"5x4099": 4 * 4099 + TILE, "300x64": 21 * 64, "200x3": 51 * 3, "3chunks": 5 * TILE}


# ---- fixtures: a test module imports them by name, and so has a GpuCodec of its own ----------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    c = GpuCodec(0)
    yield c
    c.close()


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def encode(torch, codec, data, bs):
    enc = Enc(torch, codec, data, bs, sub=True)
    enc.codec, enc.raw_size, enc.row_bs = codec, enc.n, enc.bs
    return enc


_cache = {}


def encoded(torch, codec, kind, shape):
    """one encode per (input, byte-search shape) for the whole run; the tests never change it"""
    if (kind, shape) not in _cache:
        bs, n = BYTE_SHAPES[shape]
        if kind == "mix":                               # one-symbol and ordinary blocks alternate
            data = datagen.zipf255(n, seed=4).copy()
            for b in range(0, n, 2 * bs):
                data[b:b + bs] = 41
        else:
            data = make(kind, n, bs)
        enc = Enc(torch, codec, data, bs, sub=True)
        enc.raw_size, enc.row_bs = enc.n, enc.bs
        _cache[kind, shape] = enc
    return _cache[kind, shape]


_base = {}


def base_of(shape):
    """zipf-like bytes of one of the four shapes, made once; never changed (planted() copies)"""
    if shape not in _base:
        _base[shape] = datagen.zipf255(FOUR_SHAPES[shape][1], seed=60 + len(_base))
    return _base[shape]


def base_without(n, seed, value=NL):
    """zipf-like bytes in which `value` does not occur"""
    data = datagen.zipf255(n, seed=seed).copy()
    data[data == value] = value + 1
    return data


def with_delimiters(data, at, value=NL):
    data = np.array(data, dtype=np.uint8)
    data[np.asarray(at, dtype=np.int64)] = value
    return data


def pattern_upto_255(length, seed):
    """`length` bytes that zipf-like data does not hold by chance (for 5 bytes and more), without a period"""
    return bytes(np.random.default_rng(seed).integers(128, 256, length).astype(np.uint8))


def pattern_below_255(length, seed):
    """the same without the value 255, which zipf255 lacks: a block of all 256 values would need HUFGPU_RELAXED_TREE"""
    return bytes(np.random.default_rng(seed).integers(128, 255, length).astype(np.uint8))


def planted(data, pattern, starts):
    """a copy of data with the pattern at every start (cut at the end of the data: such a one cannot match)"""
    data = np.array(data, dtype=np.uint8)
    pat = np.frombuffer(pattern, np.uint8)
    for s in starts:
        k = min(pat.size, data.size - s)
        data[s:s + k] = pat[:k]
    return data


def planted_each(data, strings, starts):
    data = np.array(data, dtype=np.uint8)
    for s, at in zip(strings, starts):
        data = planted(data, s, [at])
    return data


def spellings(word, count, seed):
    """`count` mixed-case spellings of a word of letters, all different from each other while there are enough"""
    rng = np.random.default_rng(seed)
    out = [word.lower(), word.upper()]
    while len(out) < count:
        out.append(bytes(c ^ (0x20 * int(rng.integers(0, 2))) for c in word))
    return out[:count]


def mixed_blocks(bs, nblocks, seed):
    """one-symbol blocks (41) and ordinary ones alternate"""
    data = datagen.zipf255(nblocks * bs, seed=seed).copy()
    for b in range(0, nblocks, 2):
        data[b * bs:(b + 1) * bs] = 41
    return data


def two_values(n, seed):
    """two byte values have the codes 00 and 01: a 1 at an even payload bit leaves the tree"""
    return (np.random.default_rng(seed).integers(0, 2, n) * 200 + 7).astype(np.uint8)


def runs_input(torch, codec):
    """two byte values, codes 00 and 01: a 1 at an even payload bit leaves the tree.  7 is the delimiter, the records are the
    runs of 207; those of nine bytes and more hold the pattern.  Records run into and out of every block, and block 1's last
    byte is the delimiter in front of a record (tests/test_gpu_find_records.py)"""
    bs, n = 4099, 5 * 4099
    rng = np.random.default_rng(56)
    data = (rng.integers(0, 5, n) != 0).astype(np.uint8) * 200 + 7
    data[bs - 40:bs + 30] = 207
    data[3 * bs - 30:3 * bs + 40] = 207
    data[4 * bs - 40:4 * bs + 5] = 207
    data[[bs - 41, 2 * bs + 40, 3 * bs - 31, 3 * bs + 40, 4 * bs - 41, 4 * bs + 5]] = 7
    data[2 * bs - 1] = 7
    data[2 * bs:2 * bs + 40] = 207
    data[0:4] = 207
    data[4] = 7
    return encode(torch, codec, data, bs), bytes([7]), [[bytes([207])] * 9]


def literal(word):
    return [bytes([v]) for v in word]


def damaged(enc, at, xor):
    st = enc.stream.clone()
    st[at] ^= xor
    return enc.with_stream(st)


def payload_start(enc, b):
    bo = int(enc.h_offs[b])
    tl = int.from_bytes(bytes(enc.stream[bo + 8:bo + 10].cpu().numpy()), "little")
    return bo + 10 + 2 * tl


# ---- the caller --------------------------------------------------------------------------------------------------------------
METHODS = ("find_bytes", "find_pattern", "find_records")


def find_enqueue(torch, codec, enc, name, key, cap, delims=b"\n", words=W, anchors=0, max_len=0, invert=False, before=0, after=0,
                 numbers=None, flags=None, counts=True, sub=None, raw_size=None, blocksize=None, **kw):
    """One call with guarded output buffers - LEAD guard words in front, `cap` slots, TAIL behind, all filled with the guard -
    for exactly the outputs the call has; returns the 7-tuple of device tensors without a wait (find_fetch brings it to the
    host), so that the call can stand behind a gate or in a captured graph (tests/test_gpu_streams.py).

    `name` is a GpuCodec method - find_bytes, find_pattern, find_records - which picks the C call by the type of `key` (values,
    a literal, classes, an AnyOf) and by `kw` (ignore_case, relaxed, ...); `numbers` there is line_numbers=True with a third
    buffer.  Or it is one of the C calls of tests/find_calls.py that take the any-of table: `key` is the list of alternatives
    and the call is made as the table spells it; `numbers` and `flags` (default: given wherever the call has them) are live
    buffers at cap 0 as well, where d_rec_pos and d_rec_len are NULL.  With `direct=True` a name that both have means the C
    call, and `key` is what that call looks for: byte values, a literal, a list of classes or the list of alternatives."""
    direct = kw.pop("direct", False)
    sub = enc.sub if sub is None else sub
    raw_size = enc.raw_size if raw_size is None else raw_size
    blocksize = enc.row_bs if blocksize is None else blocksize
    by_method = name in METHODS and not direct
    slots = () if by_method else CALLS[name]
    has_lengths = name == "find_records" or "rlens" in slots
    if by_method:
        numbers, flags = bool(numbers) and bool(cap), False
    else:
        numbers, flags = "no" in slots and numbers is not False, "sel" in slots and flags is not False

    def guarded(guard, dtype, wanted):
        return torch.full((LEAD + cap + TAIL,), guard, dtype=dtype, device="cuda") if wanted else None

    pbuf = guarded(GUARD64, torch.int64, cap)
    lbuf = guarded(GUARD32, torch.int32, cap and has_lengths)
    nbuf = guarded(GUARD64, torch.int64, numbers)
    sbuf = guarded(GUARD8, torch.uint8, flags)
    if by_method:
        head = (enc.stream, enc.length, enc.offsets, enc.nb, sub, raw_size, blocksize)
        if has_lengths:
            out = tuple(b[LEAD:LEAD + cap] for b in (pbuf, lbuf, nbuf) if b is not None) if cap else None
            if numbers:
                kw["line_numbers"] = True
            res = codec.find_records(*head, key, delims, max_records=cap, max_len=max_len, block_counts=counts, out=out, **kw)
            totals, errs, cnt = res[2:5]
        else:
            _, totals, errs, cnt = getattr(codec, name)(*head, key, max_positions=cap, block_counts=counts,
                                                        out=pbuf[LEAD:LEAD + cap] if cap else None, **kw)
    else:
        assert not kw, kw
        if "lens" in slots:
            classes, lens = GpuCodec.alt_classes(AnyOf(*key))
            looked_for = dict(cls=classes.tobytes(), lens=lens.tobytes(), n=len(lens))
        elif "cls" in slots:
            looked_for = dict(cls=GpuCodec.byte_classes(key).tobytes(), plen=len(key))
        elif "pattern" in slots:
            looked_for = dict(pattern=bytes(key), plen=len(key))
        else:
            looked_for = dict(st=GpuCodec.byte_set(key))
        totals = torch.empty(4, dtype=torch.int64, device="cuda")
        errs = torch.empty(enc.nb, dtype=torch.int32, device="cuda")
        cnt = torch.empty(enc.nb, dtype=torch.int64, device="cuda") if counts else None

        def ptr(buf):
            return None if buf is None else buf[LEAD:].data_ptr()

        values = dict(ctx=codec._ctx, stream=enc.stream.data_ptr(), stream_len=enc.length, index=enc.offsets.data_ptr(), nblocks=enc.nb,
                      sub=sub.data_ptr(), raw_size=raw_size, blocksize=blocksize, **looked_for,
                      delims=None if delims is None else GpuCodec.byte_set(delims),
                      words=None if words is None else GpuCodec.byte_set(words), anchors=anchors, select=1 if invert else 0,
                      before=before, after=after, pos=ptr(pbuf), rlens=ptr(lbuf), no=ptr(nbuf), sel=ptr(sbuf), cap=cap, max_len=max_len,
                      counts=cnt.data_ptr() if counts else None, totals=totals.data_ptr(), errs=errs.data_ptr(), flags=0,
                      hip_stream=codec._stream())
        codec._check(invoke(codec.lib, name, values), "Failed to enqueue the search")

    return (pbuf, lbuf, totals, errs, cnt if counts else None, nbuf, sbuf)


def find_fetch(bufs):
    """find_enqueue's device tensors as the 7-tuple of host arrays (waits for the stream they are fetched on)"""
    return tuple(None if t is None else t.cpu().numpy() for t in bufs)


def find_call(torch, codec, enc, name, key, cap, **kw):
    """find_enqueue and find_fetch in one: the call and its 7-tuple of host arrays"""
    return find_fetch(find_enqueue(torch, codec, enc, name, key, cap, **kw))


def positions_of(res):
    """(starts, totals, errs, counts): what a positions call has"""
    return (res[0], res[2], res[3], res[4])


# the per-feature callers, by the names the tests use
def find(torch, codec, enc, values, cap, counts=True, sub=None, relaxed=False, raw_size=None, blocksize=None):
    """one GpuCodec.find_bytes call"""
    return positions_of(find_call(torch, codec, enc, "find_bytes", values, cap, counts=counts, sub=sub, relaxed=relaxed,
                                  raw_size=raw_size, blocksize=blocksize))


def psearch(torch, codec, enc, pattern, cap, counts=True, sub=None, **kw):
    """one GpuCodec.find_pattern call: a literal, classes or an AnyOf"""
    return positions_of(find_call(torch, codec, enc, "find_pattern", pattern, cap, counts=counts, sub=sub, **kw))


def rsearch(torch, codec, enc, pattern, delims, cap, max_len=0, counts=True, sub=None, **kw):
    """one GpuCodec.find_records call; (starts, lengths, totals, errs, counts)"""
    return find_call(torch, codec, enc, "find_records", pattern, cap, delims=delims, max_len=max_len, counts=counts, sub=sub, **kw)[:5]


def numbered(torch, codec, enc, pattern, delims, cap):
    """one GpuCodec.find_records(line_numbers=True) call - the select call; the first six"""
    return find_call(torch, codec, enc, "find_records", pattern, cap, delims=delims, numbers=True)[:6]


def select(torch, codec, enc, alts, delims, cap, max_len=0, invert=False, numbers=True, counts=True, sub=None):
    """one hufgpu_find_records_select call; the first six"""
    return find_call(torch, codec, enc, "find_records_select", alts, cap, delims=delims, max_len=max_len, invert=invert,
                     numbers=numbers, counts=counts, sub=sub)[:6]


def context(torch, codec, enc, alts, delims, cap, max_len=0, invert=False, before=0, after=0, numbers=True, flags=True, counts=True,
            sub=None):
    """one hufgpu_find_records_context call"""
    return find_call(torch, codec, enc, "find_records_context", alts, cap, delims=delims, max_len=max_len, invert=invert,
                     before=before, after=after, numbers=numbers, flags=flags, counts=counts, sub=sub)


def positions(torch, codec, enc, alts, anchors, cap, delims=b"\n", words=W, counts=True, sub=None):
    """one hufgpu_find_any_anchored call"""
    return positions_of(find_call(torch, codec, enc, "find_any_anchored", alts, cap, delims=delims, words=words, anchors=anchors,
                                  counts=counts, sub=sub))


def records(torch, codec, enc, alts, anchors, cap, delims=b"\n", words=W, max_len=0, invert=False, before=0, after=0, numbers=True,
            flags=True, counts=True, sub=None):
    """one hufgpu_find_records_anchored call"""
    return find_call(torch, codec, enc, "find_records_anchored", alts, cap, delims=delims, words=words, anchors=anchors,
                     max_len=max_len, invert=invert, before=before, after=after, numbers=numbers, flags=flags, counts=counts, sub=sub)


# ---- the checker -------------------------------------------------------------------------------------------------------------
def seven(res):
    """a result in any of its forms as the 7-tuple"""
    res = tuple(res)
    if len(res) == 4:
        return (res[0], None, res[1], res[2], res[3], None, None)
    assert 5 <= len(res) <= 7, len(res)
    return res + (None,) * (7 - len(res))


def model_parts(want):
    """a model's answer as (starts, lengths, counts, totals, numbers, flags)"""
    want = tuple(want)
    if len(want) == 3:
        return (want[0], None, want[1], want[2], None, None)
    assert 4 <= len(want) <= 6, len(want)
    return want + (None,) * (6 - len(want))


# output -> (its place in the result, its place in the model's answer, the guard, the buffer's type, the type compared in)
OUTPUTS = {"starts": (0, 0, GUARD64, np.int64, np.int64), "lengths": (1, 1, GUARD32, np.int32, np.uint32),
           "numbers": (5, 4, GUARD64, np.int64, np.int64), "flags": (6, 5, GUARD8, np.uint8, np.uint8)}


def check(res, want, cap, what=""):
    """the call's host arrays against the model's answer: totals, statuses, counts, and every output buffer the call has in
    full - the written entries and the guard words in front of them, behind them and from totals[1] on"""
    res, want = seven(res), model_parts(want)
    totals, errs, cnt = res[2:5]
    assert totals.tolist() == want[3].tolist(), (what, totals, want[3])
    assert int(np.count_nonzero(errs)) == int(totals[2]), what
    if cnt is not None:
        assert np.array_equal(cnt, want[2]), (what, np.flatnonzero(cnt != want[2])[:8])
    for name, (r, w, guard, dtype, view) in OUTPUTS.items():
        buf = res[r]
        if buf is None:
            continue
        assert want[w] is not None, (what, "the call gave", name, "and the model has none")
        full = np.full(LEAD + cap + TAIL, guard, dtype).view(view)
        full[LEAD:LEAD + want[w].size] = want[w]
        assert buf.size == full.size, (what, name, buf.size, full.size)
        bad = np.flatnonzero(buf.view(view) != full)
        assert bad.size == 0, (what, name, "differ at", bad[:8] - LEAD, buf[bad[:8]], full[bad[:8]])


def same_arrays(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


# ---- the drivers -------------------------------------------------------------------------------------------------------------
def exact_answer(call, model, n, must=(), must_not=(), room=7, what="", total_in=None, probe=None, all_served=True):
    """`call(cap)` is one call of any kind with the test's arguments, `model(cap, served)` its model's answer.  The model's
    answer at the cap `n`, which holds everything, has `must` among its starts and none of `must_not`, and its total lies in
    `total_in` = (lowest, highest) where that is given; the call at that total + `room` gives the model's answer.  Without
    `probe` every block must be served.  With it, `probe()` is the same call at cap 0 with no optional output: its statuses
    are OK or RW (all OK unless `all_served` is False), it gives the model's count for the served blocks, and the second call
    has the same statuses.  Returns (the model's full answer, the second call's result, the statuses)."""
    served = None
    if probe is not None:
        first = probe()
        errs = seven(first)[3]
        assert set(errs.tolist()) <= {OK, RW} and (not all_served or not errs.any()), (what, errs)
        served = errs == OK
    full = model(n, served)
    starts, totals = model_parts(full)[0], model_parts(full)[3]
    total = int(totals[0])
    if total_in is not None:
        assert total_in[0] <= total <= total_in[1], (what, "the planted input has", total)
    found = set(starts.tolist())
    assert found >= set(must) and not found & set(must_not), (what, sorted(set(must) - found), sorted(found & set(must_not)))
    if probe is not None:
        check(first, model(0, served), 0, (what, "count"))
    res = call(total + room)
    if probe is None:
        errs = seven(res)[3]
        assert not errs.any(), (what, np.flatnonzero(errs)[:8])
    else:
        assert np.array_equal(seven(res)[3], errs), what
    check(res, model(total + room, served), total + room, what)
    return full, res, errs


def answer_or_not_served(call, model, cap, what=""):
    """every block has status OK or RW, and the answer is the model's for the blocks with status OK; returns the statuses"""
    res = call(cap)
    errs = seven(res)[3]
    assert set(errs.tolist()) <= {OK, RW}, what
    check(res, model(cap, errs == OK), cap, what)
    return errs


def as_is(key):
    return key


def any_of(alts):
    return AnyOf(*alts)


# the pair for positions and the pair for records: GpuCodec.find_pattern / find_records against `model_fn`, one of tests/find*_model.py.
# A test module binds the first two arguments; `wrap` makes the call's pattern of the test's key (as_is, any_of)
def exact_positions(model_fn, wrap, torch, codec, enc, key, must=(), must_not=(), room=7, what="", model=None, literal=None, **kw):
    """all blocks served and everything equal to the model; `must` / `must_not`: starts the model is seen to hold / lack.
    `model`: the key the model gets when the call gets something else (a literal with ignore_case); `literal`: the string
    whose find_pattern answer on the GPU is the same, word for word.  Returns (the total, the call's host arrays)"""
    mkey = key if model is None else model
    full, res, _ = exact_answer(lambda cap: psearch(torch, codec, enc, wrap(key), cap, **kw),
                                lambda cap, served: model_fn(enc.data, mkey, enc.bs, cap, served=served), enc.n, must, must_not, room, what,
                                total_in=(1, enc.n - 1))
    total = int(full[2][0])
    if literal is not None:
        assert same_arrays(res, psearch(torch, codec, enc, literal, total + room)), (what, "differs from find_pattern")
    return total, res


def positions_exact_or_not_served(model_fn, wrap, torch, codec, enc, key, cap, sub=None, what=""):
    """every block has status 0 or RW, and the answer is the model's for the blocks with status 0; returns the statuses"""
    return answer_or_not_served(lambda cap: psearch(torch, codec, enc, wrap(key), cap, sub=sub),
                                lambda cap, served: model_fn(enc.data, key, enc.bs, cap, served=served), cap, what)


def exact_records(model_fn, wrap, torch, codec, enc, key, delims=b"\n", must=(), must_not=(), room=7, max_len=0, what="", model=None, **kw):
    """... for records: `must` / `must_not` are record starts; returns (the model's starts, its lengths, the call's host arrays)"""
    mkey = key if model is None else model
    full, res, _ = exact_answer(lambda cap: rsearch(torch, codec, enc, wrap(key), delims, cap, max_len, **kw),
                                lambda cap, served: model_fn(enc.data, mkey, delims, enc.bs, cap, max_len, served=served), enc.n, must, must_not,
                                room, what, total_in=(1, enc.n))
    return full[0], full[1], res


def records_exact_or_not_served(model_fn, wrap, torch, codec, enc, key, delims, cap, sub=None, max_len=0, what=""):
    return answer_or_not_served(lambda cap: rsearch(torch, codec, enc, wrap(key), delims, cap, max_len, sub=sub),
                                lambda cap, served: model_fn(enc.data, key, delims, enc.bs, cap, max_len, served=served), cap, what)

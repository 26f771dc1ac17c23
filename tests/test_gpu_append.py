"""GPU tests of hufgpu_append and hufgpu_truncate (GpuCodec.append / truncate): an indexed stream made longer or shorter
in place.

Bit-exact, no tolerance.  The expected stream and block index are the oracle's encode of the new data and, as a second
witness, hufgpu_encode of it.  The stream's buffer, the index and the new sub-index lie between guard bytes that must
still hold their fill, as must everything behind the new length and behind the new index' last entry; the records and
index entries in front of the first block that is encoded again are compared with a copy taken before the call, and
after an error the whole stream and index are.
"""
import ctypes as C

import numpy as np
import pytest

import sub_index_ref as sref
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 80
IDX_FILL = -0x5A5A5A5A5A5A5A5B
SUB_FILL = 0x7B7B7B7B7B7B7B7B
HUFE_OK, HUFE_MEMORY, HUFE_ARGUMENT = 0, 1, 2
KIB, MIB = 1 << 10, 1 << 20


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def make(kind, n, seed=0):
    if n == 0:
        return np.zeros(0, np.uint8)
    if kind == "zipf255":
        return datagen.zipf255(n, seed=3 + seed)
    if kind == "uniform256":
        return datagen.uniform256(n, seed=1 + seed)
    if kind == "logtext":
        return datagen.logtext(n, seed=5 + seed)
    raise ValueError(kind)


def nblocks(n, bs):
    return -(-n // bs)


def bound(n, bs):
    return nblocks(n, bs) * (10 + 2 * 1025 + 1) + (n * 9 + 7) // 8 + 16


class Buf:
    """a stream of `data` in blocks of bs in guarded device buffers: `cap` bytes for the stream, `entries` index entries"""

    def __init__(self, torch, codec, data, bs, cap=None, entries=None, sub=False, stream=None, index=None, room=64):
        self.torch, self.bs = torch, bs
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.raw = int(self.data.size)
        self.sub = codec.new_sub_index(self.raw, bs) if sub and self.raw else None
        if stream is None:
            if self.raw:
                st, offs, length = codec.encode(dev(torch, self.data), bs, sub_index=self.sub)
                stream, index = st[:length].cpu().numpy(), offs.cpu().numpy()
            else:
                stream, index = np.zeros(0, np.uint8), np.zeros(1, np.int64)
        self.length = int(stream.size)
        self.cap = self.length + room if cap is None else cap
        nb = nblocks(self.raw, bs)
        self.entries = nb + 1 if entries is None else entries
        assert self.cap >= self.length and self.entries >= nb + 1
        self.big = torch.full((self.cap + 2 * GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
        self.stream = self.big[GUARD_BYTES:GUARD_BYTES + self.cap]
        self.stream[:self.length] = dev(torch, stream) if self.length else self.stream[:0]
        self.idx_big = torch.full((self.entries + 4,), IDX_FILL, dtype=torch.int64, device="cuda")
        self.index = self.idx_big[2:2 + self.entries]
        self.index[:nb + 1] = torch.from_numpy(np.asarray(index[:nb + 1]).astype(np.int64)).cuda()

    def host(self):
        hb, hi = self.big.cpu().numpy(), self.idx_big.cpu().numpy()
        assert np.all(hb[:GUARD_BYTES] == GUARD) and np.all(hb[GUARD_BYTES + self.cap:] == GUARD), "guard bytes around the stream's buffer"
        assert np.all(hi[:2] == IDX_FILL) and np.all(hi[2 + self.entries:] == IDX_FILL), "guard words around the index"
        return hb[GUARD_BYTES:GUARD_BYTES + self.cap].copy(), hi[2:2 + self.entries].copy()


class Result:
    pass


def guarded_sub(torch, codec, n, bs):
    words = max(1, -(-codec.sub_index_bytes(n, bs) // 8))
    big = torch.full((words + 4,), SUB_FILL, dtype=torch.int64, device="cuda")
    return big, big[2:2 + words]


def finish(buf, r, before, nb_old, nb_keep, nb_new, sub_big):
    """the guards, and what has to be unchanged, after a call"""
    st, idx = buf.host()
    b_st, b_idx = before
    r.all, r.index_all = st, idx
    if sub_big is not None:
        hs = sub_big.cpu().numpy()
        assert np.all(hs[:2] == SUB_FILL) and np.all(hs[-2:] == SUB_FILL), "guard words around the new sub-index"
    if r.rc != HUFE_OK:
        assert r.length == 0, "on any error *out_len = 0"
        assert np.array_equal(st, b_st), "the stream's buffer was written by a call that failed"
        assert np.array_equal(idx, b_idx), "the index was written by a call that failed"
        return r
    keep_bytes = int(b_idx[nb_keep]) if nb_old else 0
    assert np.array_equal(st[:keep_bytes], b_st[:keep_bytes]), "a record in front of the first new one was written"
    if nb_old:
        assert np.array_equal(idx[:nb_keep + 1], b_idx[:nb_keep + 1]), "an index entry in front of the new ones was written"
    assert np.array_equal(st[r.length:], b_st[r.length:]), "bytes in [out_len, stream_cap) were written"
    assert np.array_equal(idx[nb_new + 1:], b_idx[nb_new + 1:]), "index entries behind the new last one were written"
    r.stream = st[:r.length]
    r.index = idx[:nb_new + 1].astype(np.uint64)
    return r


def append(torch, codec, buf, a, src_off=0, old_sub=None, want_sub=False, relaxed=False, raw_size=None, cap=None):
    """one hufgpu_append through the C ABI; the new bytes start src_off bytes behind an aligned address"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    raw = buf.raw if raw_size is None else raw_size
    bs = buf.bs
    d_src = torch.full((a.size + src_off + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    if a.size:
        d_src[src_off:src_off + a.size] = dev(torch, a)
    nb_old, nb_new = nblocks(raw, bs), nblocks(raw + a.size, bs)
    nb_keep = nb_old - (1 if raw % bs else 0)
    sub_big = sub_new = None
    if want_sub:
        sub_big, sub_new = guarded_sub(torch, codec, raw + a.size, bs)
    before = buf.host()
    out_len = C.c_uint64(77)
    r = Result()
    r.rc = int(codec.lib.hufgpu_append(codec._ctx, buf.stream.data_ptr(), buf.length, buf.cap if cap is None else cap,
                                       buf.index.data_ptr(), raw, bs, d_src.data_ptr() + src_off, a.size,
                                       old_sub.data_ptr() if old_sub is not None else None,
                                       sub_new.data_ptr() if sub_new is not None else None, 1 if relaxed else 0,
                                       C.byref(out_len), None))
    r.length, r.sub = int(out_len.value), sub_new
    r.msg = codec.lib.hufgpu_last_error(codec._ctx).decode()
    assert np.all(d_src.cpu().numpy()[:src_off] == 0xEE)
    if a.size == 0 and r.rc == HUFE_OK:
        nb_keep = nb_old
    return finish(buf, r, before, nb_old, nb_keep, nb_new, sub_big)


def truncate(torch, codec, buf, new_raw, old_sub=None, want_sub=False, relaxed=False):
    bs, raw = buf.bs, buf.raw
    nb_old, nb_new = nblocks(raw, bs), nblocks(new_raw, bs)
    sub_big = sub_new = None
    if want_sub:
        sub_big, sub_new = guarded_sub(torch, codec, new_raw, bs)
    before = buf.host()
    out_len = C.c_uint64(77)
    r = Result()
    r.rc = int(codec.lib.hufgpu_truncate(codec._ctx, buf.stream.data_ptr(), buf.length, buf.index.data_ptr(), raw, bs, new_raw,
                                         old_sub.data_ptr() if old_sub is not None else None,
                                         sub_new.data_ptr() if sub_new is not None else None, 1 if relaxed else 0,
                                         C.byref(out_len), None))
    r.length, r.sub = int(out_len.value), sub_new
    r.msg = codec.lib.hufgpu_last_error(codec._ctx).decode()
    nb_keep = nb_old if new_raw == raw else new_raw // bs
    return finish(buf, r, before, nb_old, nb_keep, nb_new if new_raw != raw else nb_old, sub_big)


def check_equals_encode(torch, codec, oracle, new, bs, r, what):
    """stream and index equal the oracle's and hufgpu_encode's encode of the new data"""
    assert r.rc == HUFE_OK, (what, r.rc, r.msg)
    want, woffs = oracle.encode(new, bs, with_offsets=True) if new.size else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert r.length == want.size, (what, r.length, want.size)
    bad = np.flatnonzero(r.stream != want)
    assert bad.size == 0, (what, "stream differs from the oracle's at", bad[:8], "index", woffs[:6])
    assert np.array_equal(r.index, np.asarray(woffs, dtype=np.uint64)), (what, "index", r.index, woffs)
    if new.size:
        st2, offs2, len2 = codec.encode(dev(torch, new), bs)
        assert len2 == r.length and np.array_equal(st2[:len2].cpu().numpy(), r.stream), (what, "hufgpu_encode of the new data")
        assert np.array_equal(offs2.cpu().numpy().astype(np.uint64), r.index), (what, "hufgpu_encode's index")
    return want, woffs


def tails(bs):
    return [0, 1, bs // 2 + 3, bs - 1]


def lengths(bs, t):
    return [0, 1, bs - t - 1, bs - t, bs - t + 1, 3 * bs + 17]


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
@pytest.mark.parametrize("kind", ["zipf255", "logtext", "uniform256"])
def test_append_equals_the_encode_of_the_new_data(torch_mod, codec, oracle, kind, bs):
    torch = torch_mod
    relaxed = kind == "uniform256"                       # (a block with all 256 values has the 1 025-entry tree)
    pool = make(kind, 8 * bs)
    for ti, t in enumerate(tails(bs)):
        raw = 2 * bs + t
        d = pool[:raw]
        for li, la in enumerate(lengths(bs, t)):
            if la < 0 or (la == 0 and li):
                continue
            a = pool[raw:raw + la]
            nb_new = nblocks(raw + la, bs)
            buf = Buf(torch, codec, d, bs, entries=nb_new + 1, room=bound(t + la, bs))
            r = append(torch, codec, buf, a, src_off=(ti + li) % 4, relaxed=relaxed)
            if la == 0:
                assert (r.rc, r.length) == (HUFE_OK, buf.length)
                assert np.array_equal(r.all, buf.host()[0])
                continue
            check_equals_encode(torch, codec, oracle, pool[:raw + la], bs, r, (kind, bs, t, la))


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_append_to_nothing_equals_encode(torch_mod, codec, oracle, bs):
    torch = torch_mod
    for la in (1, bs, 2 * bs + 77):
        a = make("logtext", la)
        buf = Buf(torch, codec, np.zeros(0, np.uint8), bs, entries=nblocks(la, bs) + 1, cap=bound(la, bs))
        buf.index[0] = 12345                             # (an empty stream's index is not read)
        r = append(torch, codec, buf, a, src_off=3)
        check_equals_encode(torch, codec, oracle, a, bs, r, ("to nothing", bs, la))


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_one_value_blocks(torch_mod, codec, oracle, bs):
    torch = torch_mod
    t = bs // 3
    d = np.concatenate([make("zipf255", bs), np.full(t, 0x41, np.uint8)])
    # a one-value tail becomes mixed
    a = make("zipf255", 100, seed=1)
    buf = Buf(torch, codec, d, bs, cap=4 * bs)
    r = append(torch, codec, buf, a, src_off=1)
    check_equals_encode(torch, codec, oracle, np.concatenate([d, a]), bs, r, "one value becomes mixed")
    # one-value data plus the same value: the one-symbol record, a five-entry tree and one bit a byte
    a = np.full(bs - t - 8, 0x41, np.uint8)
    buf = Buf(torch, codec, d, bs, cap=4 * bs)
    r = append(torch, codec, buf, a, src_off=2)
    _, woffs = check_equals_encode(torch, codec, oracle, np.concatenate([d, a]), bs, r, "one value stays")
    assert int(woffs[2] - woffs[1]) == 10 + 2 * 5 + (bs - 8) // 8


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_a_chain_of_twenty_appends(torch_mod, codec, oracle, bs):
    torch = torch_mod
    rng = np.random.default_rng(20 + bs)
    lens = [int(rng.integers(1, int(2.5 * bs) + 1)) for _ in range(20)]
    pool = make("zipf255", bs // 2 + 5 + sum(lens))
    raw = bs // 2 + 5
    buf = Buf(torch, codec, pool[:raw], bs, entries=nblocks(pool.size, bs) + 1, cap=bound(pool.size, bs) + 64)
    for i, la in enumerate(lens):
        r = append(torch, codec, buf, pool[raw:raw + la], src_off=i % 5)
        assert r.rc == HUFE_OK, (i, r.msg)
        raw += la
        want, woffs = oracle.encode(pool[:raw], bs, with_offsets=True)
        assert r.length == want.size and np.array_equal(r.stream, want), (i, la)
        assert np.array_equal(r.index, np.asarray(woffs, dtype=np.uint64)), (i, la)
        buf.raw, buf.length, buf.data = raw, r.length, pool[:raw]
    out = torch.empty(raw, dtype=torch.uint8, device="cuda")
    got = codec.decode(buf.stream, buf.length, buf.index, nblocks(raw, bs), out)
    assert got == raw and np.array_equal(out.cpu().numpy(), pool[:raw])


def test_the_chunked_route(torch_mod, codec, oracle):
    """blocks of 2 MiB: the slow route through the chunked encoder - append, a capacity one byte short, truncate"""
    torch = torch_mod
    bs = 2 * MIB
    raw, la = bs + bs // 2 + 3, bs + 17
    pool = make("zipf255", raw + la)
    buf = Buf(torch, codec, pool[:raw], bs, entries=4, room=bound(bs // 2 + 3 + la, bs))
    r = append(torch, codec, buf, pool[raw:], src_off=1)
    want, _ = check_equals_encode(torch, codec, oracle, pool, bs, r, "2 MiB blocks")
    short = Buf(torch, codec, pool[:raw], bs, entries=4, cap=int(want.size) - 1)
    r = append(torch, codec, short, pool[raw:], src_off=1)
    assert r.rc == HUFE_MEMORY
    buf.raw, buf.length = raw + la, int(want.size)
    r = truncate(torch, codec, buf, bs + 12345)
    check_equals_encode(torch, codec, oracle, pool[:bs + 12345], bs, r, "2 MiB blocks, truncate")
    sub_big, sub_new = guarded_sub(torch, codec, raw + la, bs)
    out_len = C.c_uint64(7)
    rc = codec.lib.hufgpu_append(codec._ctx, short.stream.data_ptr(), short.length, short.cap, short.index.data_ptr(), raw, bs,
                                 dev(torch, pool[raw:]).data_ptr(), la, None, sub_new.data_ptr(), 0, C.byref(out_len), None)
    assert (rc, out_len.value) == (HUFE_ARGUMENT, 0) and np.all(sub_big.cpu().numpy() == SUB_FILL)


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_capacity(torch_mod, codec, oracle, bs):
    torch = torch_mod
    raw, la = 2 * bs + bs // 2 + 3, bs + 99
    pool = make("logtext", raw + la)
    want, _ = oracle.encode(pool, bs, with_offsets=True)
    exact = Buf(torch, codec, pool[:raw], bs, entries=5, cap=int(want.size))
    r = append(torch, codec, exact, pool[raw:])
    check_equals_encode(torch, codec, oracle, pool, bs, r, "stream_cap exactly the new length")
    short = Buf(torch, codec, pool[:raw], bs, entries=5, cap=int(want.size) - 1)
    r = append(torch, codec, short, pool[raw:])
    assert r.rc == HUFE_MEMORY                           # (finish() compared the stream and the index with their copies)
    # a buffer longer than the capacity that is passed: nothing behind stream_cap is written
    roomy = Buf(torch, codec, pool[:raw], bs, entries=5, cap=int(want.size) + 500)
    r = append(torch, codec, roomy, pool[raw:], cap=int(want.size) - 1)
    assert r.rc == HUFE_MEMORY


def flip_payload_bit(buf, b, at=0.5):
    st, idx = buf.host()
    o0, o1 = int(idx[b]), int(idx[b + 1])
    tree_len = int(np.frombuffer(st[o0 + 8:o0 + 10].tobytes(), "<i2")[0])
    pay = o0 + 10 + 2 * tree_len
    pos = pay + int((o1 - pay) * at)
    buf.stream[pos] ^= 0x10
    return pos


def decode_block(codec, torch, buf, b, room, relaxed=False):
    out = torch.empty(max(1, room), dtype=torch.uint8, device="cuda")
    raw = C.c_uint64(0)
    offs = buf.index[b:b + 2].contiguous()
    return int(codec.lib.hufgpu_decode(codec._ctx, buf.stream.data_ptr(), buf.length, offs.data_ptr(), 1, out.data_ptr(), room,
                                       1 if relaxed else 0, C.byref(raw), None))


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_errors_leave_everything_unchanged(torch_mod, codec, oracle, bs):
    torch = torch_mod
    t = bs // 2 + 3
    raw, la = 3 * bs + t, bs + 5
    pool = make("uniform256", raw + la)                  # (every code is 8 or 9 bits: a flipped bit is another symbol or a short payload)
    pool[::7] = 0
    d, a = pool[:raw], pool[raw:]
    cap = Buf(torch, codec, d, bs).length + bound(t + la, bs)      # the bound the header gives: always enough

    # damage in the tail block that its decode reports: that error, and nothing is written
    hit = None
    for at in (0.999, 0.99, 0.9, 0.5, 0.2):
        buf = Buf(torch, codec, d, bs, entries=6, cap=cap)
        flip_payload_bit(buf, 3, at)
        expect = decode_block(codec, torch, buf, 3, t, relaxed=True)
        if expect != HUFE_OK:
            hit = (buf, expect)
            break
    assert hit is not None, "no flipped bit made hufgpu_decode of the tail block fail"
    buf, expect = hit
    r = append(torch, codec, buf, a, relaxed=True)
    assert r.rc == expect, (r.rc, expect, r.msg)
    r = truncate(torch, codec, buf, 3 * bs + 7, relaxed=True)
    assert r.rc == expect, (r.rc, expect, r.msg)

    # damage in an earlier block: not seen, the record is carried over
    clean = Buf(torch, codec, d, bs, entries=6, cap=cap)
    want = append(torch, codec, clean, a, relaxed=True)
    check_equals_encode(torch, codec, oracle, pool, bs, want, "clean")
    buf = Buf(torch, codec, d, bs, entries=6, cap=cap)
    pos = flip_payload_bit(buf, 1)
    r = append(torch, codec, buf, a, relaxed=True)
    assert r.rc == HUFE_OK and r.length == want.length and np.array_equal(r.index, want.index)
    assert np.flatnonzero(r.stream != want.stream).tolist() == [pos]

    # a last header whose block_len is not what (raw_size, blocksize) give: raw_size off by one, both ways
    for off in (-1, 1):
        buf = Buf(torch, codec, d, bs, entries=6, cap=cap)
        r = append(torch, codec, buf, a, raw_size=raw + off, relaxed=True)
        assert r.rc == HUFE_ARGUMENT, (off, r.rc, r.msg)

    # a last header that does not parse: what hufgpu_decode says of it
    buf = Buf(torch, codec, d, bs, entries=6, cap=cap)
    o = int(buf.host()[1][3])
    buf.stream[o + 8] = 0xFF                             # tree_len = 0x7fff: no tree is that long
    buf.stream[o + 9] = 0x7F
    expect = decode_block(codec, torch, buf, 3, t, relaxed=True)
    assert expect != HUFE_OK
    r = append(torch, codec, buf, a, relaxed=True)
    assert r.rc == expect, (r.rc, expect, r.msg)
    # the same with a tail of 0: nothing is decoded, the header is read all the same
    full = Buf(torch, codec, pool[:3 * bs], bs, entries=6, cap=cap)
    o = int(full.host()[1][2])
    full.stream[o + 8] = 0xFF
    full.stream[o + 9] = 0x7F
    expect = decode_block(codec, torch, full, 2, bs, relaxed=True)
    r = append(torch, codec, full, a, relaxed=True)
    assert expect != HUFE_OK and r.rc == expect


def test_a_batch_stream_is_not_canonical(torch_mod, codec):
    """the items' short last blocks lie in the middle of a batch's stream: its last header does not show raw_size % bs"""
    torch = torch_mod
    bs = 4 * KIB
    item_lens = [bs + 17, 2 * bs + 100]
    data = make("logtext", sum(item_lens))
    batch = codec.encode_batch(dev(torch, data), item_lens, bs)
    buf = Buf(torch, codec, data, bs, entries=8, cap=batch.stream_len + 3 * bs,
              stream=batch.stream[:batch.stream_len].cpu().numpy(), index=batch.offsets.cpu().numpy())
    r = append(torch, codec, buf, make("zipf255", 500))
    assert r.rc == HUFE_ARGUMENT, r.msg
    r = truncate(torch, codec, buf, bs + 5)
    assert r.rc == HUFE_ARGUMENT, r.msg


def check_sub_index(torch, codec, r, d_stream, d_index, new, want, woffs, bs, rows=None):
    exp = sref.expected(want, woffs, new, bs)
    if rows is not None:                                 # only these blocks' rows are written
        lay = exp.lay
        hit = np.zeros(lay.nb, bool)
        hit[rows] = True
        for w, per in ((exp.w_tiles, lay.tpb), (exp.w_groups, lay.gpb), (exp.w_lens, 256)):
            w &= np.repeat(hit, per)
    got = r.sub.cpu().numpy().view(np.uint8)
    assert sref.mismatches(got, exp) == [], "(block, array, index, found, expected)"
    if rows is not None:
        fill = np.full(got.size // 8, SUB_FILL, dtype=np.int64).view(np.uint8)
        assert sref.unwritten_changed(got, fill, exp) == [], "(block, array, index, found, held)"
        return
    n = new.size
    out = torch.full((n + 32,), GUARD, dtype=torch.uint8, device="cuda")
    raw = codec.decode(d_stream, r.length, d_index, exp.lay.nb, out[:n], relaxed=True, sub_index=r.sub, raw_size=n, blocksize=bs)
    assert raw == n and np.array_equal(out.cpu().numpy()[:n], new) and np.all(out.cpu().numpy()[n:] == GUARD)
    assert codec.decode_counters()[0] == 0               # every row verified: no block went to the exact decoder


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_the_new_sub_index(torch_mod, codec, oracle, bs):
    torch = torch_mod
    t = bs // 2 + 3
    raw, la = 2 * bs + t, 2 * bs + 17
    pool = make("logtext", raw + la)
    d, a = pool[:raw], pool[raw:]
    cap = Buf(torch, codec, d, bs).length + bound(t + la, bs)      # the bound the header gives: always enough
    buf = Buf(torch, codec, d, bs, entries=6, cap=cap, sub=True)
    r = append(torch, codec, buf, a, src_off=1, old_sub=buf.sub, want_sub=True)
    want, woffs = check_equals_encode(torch, codec, oracle, pool, bs, r, ("sub", bs))
    check_sub_index(torch, codec, r, buf.stream, buf.index, pool, want, woffs, bs)

    # only the new buffer: the new rows, the rest is still fill
    buf2 = Buf(torch, codec, d, bs, entries=6, cap=cap)
    r2 = append(torch, codec, buf2, a, want_sub=True)
    check_equals_encode(torch, codec, oracle, pool, bs, r2, ("sub, no old one", bs))
    check_sub_index(torch, codec, r2, buf2.stream, buf2.index, pool, want, woffs, bs, rows=slice(2, None))

    # an old sub-index that is zeroed or random: the same stream and index
    rnd = torch.from_numpy(np.random.default_rng(3).integers(-2**62, 2**62, buf.sub.numel(), dtype=np.int64)).cuda()
    for name, old in (("zeroed", torch.zeros_like(buf.sub)), ("random", rnd)):
        buf3 = Buf(torch, codec, d, bs, entries=6, cap=cap)
        r3 = append(torch, codec, buf3, a, old_sub=old, want_sub=True)
        assert r3.rc == HUFE_OK and np.array_equal(r3.stream, r.stream) and np.array_equal(r3.index, r.index), name

    # truncate inside block 3 of the appended stream: rows [0, 3) copied, row 3 written
    buf.raw, buf.length = raw + la, r.length
    cut = 3 * bs + bs // 3
    rt = truncate(torch, codec, buf, cut, old_sub=r.sub, want_sub=True)
    want, woffs = check_equals_encode(torch, codec, oracle, pool[:cut], bs, rt, ("sub, truncate", bs))
    check_sub_index(torch, codec, rt, buf.stream, buf.index, pool[:cut], want, woffs, bs)
    # and on a border, where only rows are copied
    buf.raw, buf.length = cut, rt.length
    rb = truncate(torch, codec, buf, 2 * bs, old_sub=rt.sub, want_sub=True)
    want, woffs = check_equals_encode(torch, codec, oracle, pool[:2 * bs], bs, rb, ("sub, truncate on a border", bs))
    check_sub_index(torch, codec, rb, buf.stream, buf.index, pool[:2 * bs], want, woffs, bs)


@pytest.mark.parametrize("bs", [4 * KIB, 64 * KIB], ids=["4K", "64K"])
def test_truncate(torch_mod, codec, oracle, bs):
    torch = torch_mod
    raw = 2 * bs + bs // 2 + 3
    d = make("zipf255", raw)
    for cut in (0, 2 * bs, bs, 1, bs + bs // 3, 2 * bs + 5, raw - 1, raw):
        buf = Buf(torch, codec, d, bs)
        r = truncate(torch, codec, buf, cut)
        if cut == raw:
            assert (r.rc, r.length) == (HUFE_OK, buf.length) and np.array_equal(r.all, buf.host()[0])
            continue
        check_equals_encode(torch, codec, oracle, d[:cut], bs, r, ("truncate", bs, cut))
        if cut % bs == 0:
            assert np.array_equal(r.all, buf.host()[0])  # a cut on a border writes nothing
    # truncate, then append: the oracle's encode
    extra = make("logtext", bs + 40)
    buf = Buf(torch, codec, d, bs, entries=6, room=bound(bs + extra.size, bs))
    r = truncate(torch, codec, buf, bs + 77)
    assert r.rc == HUFE_OK
    buf.raw, buf.length = bs + 77, r.length
    r = append(torch, codec, buf, extra, src_off=3)
    check_equals_encode(torch, codec, oracle, np.concatenate([d[:bs + 77], extra]), bs, r, ("truncate, then append", bs))


def test_a_reference_written_stream(torch_mod, codec, oracle, reference):
    torch = torch_mod
    bs = 64 * KIB
    raw = 2 * bs + 321
    pool = make("zipf255", raw + bs + 9)
    ref_stream = reference.encode(pool[:raw], bs)
    length = int(ref_stream.size)
    d_ref = dev(torch, ref_stream)
    d_index, nb, used = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    lib = codec.lib
    rc = lib.hufgpu_block_index(codec._ctx, C.c_void_p(d_ref.data_ptr()), C.c_uint64(length), C.c_uint64(length), C.c_uint32(0),
                                C.byref(d_index), C.byref(nb), C.byref(used), None)
    assert rc == 0 and nb.value == nblocks(raw, bs) and used.value == length
    index = torch.empty(nb.value + 1, dtype=torch.int64, device="cuda")
    assert lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(index.data_ptr()), d_index, C.c_uint64(8 * (nb.value + 1))) == 0
    buf = Buf(torch, codec, pool[:raw], bs, entries=5, cap=length + bound(321 + bs + 9, bs), stream=ref_stream,
              index=index.cpu().numpy())
    r = append(torch, codec, buf, pool[raw:], src_off=1)
    check_equals_encode(torch, codec, oracle, pool, bs, r, "reference stream")
    assert np.array_equal(reference.encode(pool, bs), r.stream)


def test_relaxed_trees_and_interleaved_calls(torch_mod, codec, oracle):
    """strict and relaxed flags give the same result on the encoder's streams; a decode of the same context in between"""
    torch = torch_mod
    bs = 64 * KIB
    raw, la = bs + 100, bs + 7
    pool = make("zipf255", raw + la)
    other = make("logtext", 3 * bs + 5)
    o_st, o_offs, o_len = codec.encode(dev(torch, other), bs)
    out = torch.empty(other.size, dtype=torch.uint8, device="cuda")
    got = []
    for relaxed in (False, True):
        buf = Buf(torch, codec, pool[:raw], bs, entries=4, room=bound(100 + la, bs))
        codec.decode(o_st, o_len, o_offs, 4, out, sync=False)             # enqueued, not waited for
        r = append(torch, codec, buf, pool[raw:], relaxed=relaxed)
        check_equals_encode(torch, codec, oracle, pool, bs, r, ("relaxed", relaxed))
        assert codec.decode(o_st, o_len, o_offs, 4, out.zero_()) == other.size and np.array_equal(out.cpu().numpy(), other)
        buf.raw, buf.length = raw + la, r.length
        r = truncate(torch, codec, buf, bs + 9, relaxed=relaxed)
        check_equals_encode(torch, codec, oracle, pool[:bs + 9], bs, r, ("relaxed, truncate", relaxed))
        got.append(r.stream)
    assert np.array_equal(got[0], got[1])


def test_the_codec_methods(torch_mod, codec, oracle):
    torch = torch_mod
    from libhuffman_amd.codec import HuffmanGpuError
    bs = 4 * KIB
    raw, la = 2 * bs + 100, 3 * bs + 5
    pool = make("logtext", raw + la)
    st, offs, length = codec.encode(dev(torch, pool[:raw]), bs)
    tight_st, tight_offs = st[:length].clone(), offs.clone()
    # the tensors are too small: new ones of the bound, the old content copied
    st2, offs2, len2, raw2, sub2 = codec.append(tight_st, length, tight_offs, raw, bs, dev(torch, pool[raw:]), new_sub_index=True)
    assert st2.data_ptr() != tight_st.data_ptr() and offs2.data_ptr() != tight_offs.data_ptr() and raw2 == raw + la
    want, woffs = oracle.encode(pool, bs, with_offsets=True)
    assert len2 == want.size and np.array_equal(st2[:len2].cpu().numpy(), want)
    assert np.array_equal(offs2[:nblocks(raw2, bs) + 1].cpu().numpy().astype(np.uint64), np.asarray(woffs, dtype=np.uint64))
    assert sub2 is not None and torch.equal(tight_st, st[:length])          # the caller's tensor is left alone
    # large enough: in place
    roomy = torch.empty(len2 + codec.encode_bound(bs, bs) + 64, dtype=torch.uint8, device="cuda")
    roomy[:len2] = st2[:len2]
    roomy_offs = torch.zeros(16, dtype=torch.int64, device="cuda")
    roomy_offs[:offs2.numel()] = offs2
    more = make("zipf255", 50)
    st3, offs3, len3, raw3 = codec.append(roomy, len2, roomy_offs, raw2, bs, dev(torch, more))
    assert st3.data_ptr() == roomy.data_ptr() and offs3.data_ptr() == roomy_offs.data_ptr() and raw3 == raw2 + 50
    want, woffs = oracle.encode(np.concatenate([pool, more]), bs, with_offsets=True)
    assert len3 == want.size and np.array_equal(st3[:len3].cpu().numpy(), want)
    st4, offs4, len4, raw4 = codec.truncate(st3, len3, offs3, raw3, bs, bs + 1)
    want, woffs = oracle.encode(pool[:bs + 1], bs, with_offsets=True)
    assert raw4 == bs + 1 and len4 == want.size and np.array_equal(st4[:len4].cpu().numpy(), want)
    assert np.array_equal(offs4[:3].cpu().numpy().astype(np.uint64), np.asarray(woffs, dtype=np.uint64))
    with pytest.raises(HuffmanGpuError) as e:
        codec.truncate(st4, len4, offs4, raw4 + 1, bs, bs + 1)              # a wrong raw_size
    assert e.value.err == HUFE_ARGUMENT

"""The sub-index rebuilt for a stream that came without one (hufgpu_sub_index_from_raw, hufgpu_decode_build_sub,
hufgpu_build_sub_index; kernels/sub_build.hpp): entry by entry against the CPU reference of tests/sub_index_ref.py on the
ORACLE's streams, byte for byte against what the encoder writes, and - on hand-made and damaged streams - that a built
sub-index never changes what a decode returns.
"""
import numpy as np
import pytest

import decode_edge_cases as dec
import handmade_streams as hm
import sub_index_ref as R

pytestmark = pytest.mark.gpu

GUARD_WORDS = 1024                      # 8 KiB behind the sub-index that no build may touch
FILL_A = 0x5A5A5A5A5A5A5A5A
FILL_B = -1                             # all ones: what is not written stays garbage for the decoder
OUT_GUARD = 64
OUT_FILL = 0xA5
WAYS = ("from_raw", "with_decode", "stream_only")

CASES = [(c, off) for c in R.cases() for off in c.dev_offsets]


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


def at_offset(torch, a: np.ndarray, off: int, fill: int = 0xC3):
    """`a` on the device, `off` bytes into a larger tensor"""
    big = torch.full((a.size + off + 64,), fill, dtype=torch.uint8, device="cuda")
    v = big[off:off + a.size]
    if a.size:
        v.copy_(torch.from_numpy(np.array(a, dtype=np.uint8)).cuda())
    return v


def guarded_out(torch, n: int, off: int = 0):
    big = torch.full((n + off + 2 * OUT_GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    return big, big[OUT_GUARD + off:OUT_GUARD + off + n]


def out_guards_intact(big, n: int, off: int = 0) -> bool:
    ob = big.cpu().numpy()
    return bool(np.all(ob[:OUT_GUARD + off] == OUT_FILL) and np.all(ob[OUT_GUARD + off + n:] == OUT_FILL))


def sub_buffer(torch, size: int, fill: int):
    words = max(1, -(-size // 8))
    buf = torch.full((words + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    return buf, buf[:words]


def build(torch, codec, way, st, st_len, offs, n, bs, sub, raw=None, relaxed=True, out_off=0):
    """-> (unbuilt, what the decode of `with_decode` returned or None)"""
    if way == "from_raw":
        return codec.build_sub_index(st, st_len, offs, n, bs, raw=raw, sub_index=sub, relaxed=relaxed)[1], None
    if way == "stream_only":
        return codec.build_sub_index(st, st_len, offs, n, bs, sub_index=sub, relaxed=relaxed)[1], None
    big, out = guarded_out(torch, n, out_off)
    raw_len, _, unbuilt = codec.decode_build_sub(st, st_len, offs, out, n, bs, sub_index=sub, relaxed=relaxed)
    assert out_guards_intact(big, n, out_off)
    return unbuilt, (raw_len, out)


# ---- contents, entry by entry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,off", CASES, ids=[f"{c.name}@{off}" for c, off in CASES])
def test_built_sub_index_equals_the_reference(torch_mod, codec, oracle, case, off):
    torch = torch_mod
    data = case.data()
    n, bs = data.size, case.blocksize
    want, woffs = oracle.encode(data, bs, with_offsets=True)
    exp = R.expected(want, woffs, data, bs)
    lay = exp.lay
    assert codec.sub_index_bytes(n, bs) == lay.size
    st = at_offset(torch, want, off)                                  # the oracle's stream, not this encoder's
    offs = torch.from_numpy(woffs.astype(np.int64)).cuda()
    d = at_offset(torch, data, off)

    for way in WAYS:
        for fill in (FILL_A, FILL_B):
            buf, sub = sub_buffer(torch, lay.size, fill)
            unbuilt, decoded = build(torch, codec, way, st, want.size, offs, n, bs, sub, raw=d, out_off=off)
            got = buf.cpu().numpy().view(np.uint8)
            held = np.full(got.size // 8, fill, dtype=np.int64).view(np.uint8)
            tag = (case.name, way, hex(fill & 0xff))
            assert R.mismatches(got, exp) == [], tag + ("(block, array, index, found, expected)",)
            assert R.unwritten_changed(got, held, exp) == [], tag + ("(block, array, index, found, held)",)
            assert np.array_equal(got[lay.size:], held[lay.size:]), tag + ("guard",)
            assert unbuilt == 0, tag
            if decoded is not None:
                assert decoded[0] == n and torch.equal(decoded[1], d), tag
            if fill == FILL_B:
                # decode with the built index, its unwritten entries all ones
                big, out = guarded_out(torch, n, off)
                raw = codec.decode(st, want.size, offs, lay.nb, out, relaxed=True, sub_index=sub, raw_size=n, blocksize=bs)
                assert raw == n and torch.equal(out, d), tag
                assert out_guards_intact(big, n, off), tag + ("output guard",)
                # no block goes to the exact decoder, but one with a code over 32 bits (decode_sub.hpp, dsub_fast_tables)
                assert codec.decode_counters()[0] == case.fix, tag


# ---- the same bytes as the encoder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [4096, 65536, 1 << 20])
@pytest.mark.parametrize("kind", ["const41", "uniform256", "uniform255", "zipf255"])
def test_built_buffer_equals_the_encoders(torch_mod, codec, kind, bs):
    torch = torch_mod
    n = 64 << 20
    d = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), kind)
    size = codec.sub_index_bytes(n, bs)
    ebuf, esub = sub_buffer(torch, size, FILL_A)
    st, offs, length = codec.encode(d, bs, sub_index=esub)
    for way in WAYS:
        buf, sub = sub_buffer(torch, size, FILL_A)
        unbuilt, decoded = build(torch, codec, way, st, length, offs, n, bs, sub, raw=d)
        assert unbuilt == 0, (kind, bs, way)
        assert torch.equal(buf, ebuf), (kind, bs, way, int((buf != ebuf).sum()))
        if decoded is not None:
            assert decoded[0] == n and torch.equal(decoded[1], d), (kind, bs, way)


# ---- never trusted, never harmful -----------------------------------------------------------------------------------------
def duplicate_leaf(blk: bytes) -> bytes:
    """the block with its second leaf carrying the byte value of its first"""
    b = bytearray(blk)
    tl = int.from_bytes(b[8:10], "little", signed=True)
    ent = np.frombuffer(bytes(b[10:10 + 2 * tl]), dtype="<i2").copy()
    leaves = [i for i in range(tl - 2) if ent[i] != -1 and ent[i + 1] == -1 and ent[i + 2] == -1]
    assert len(leaves) >= 2
    ent[leaves[1]] = ent[leaves[0]]
    b[10:10 + 2 * tl] = ent.tobytes()
    return bytes(b)


def handmade(oracle) -> list:
    """[(name, stream, offsets, raw_size, blocksize)]: streams no encoder wrote, and damaged ones"""
    out = []
    rng = np.random.default_rng(20261016)

    def one(name, blk):
        a = np.frombuffer(bytes(blk), dtype=np.uint8)
        n = int.from_bytes(bytes(blk[:8]), "little")
        n = n if 0 < n <= 1 << 20 else 4000                          # (a damaged length: any layout of one block)
        out.append((name, a, np.array([0, a.size], dtype=np.uint64), n, n))

    # random tree shapes, with and without the wrapped root; chains with codes over 100 bits
    for k, (leaves, skew, wrap, nsym, deep) in enumerate([(2, 0.0, True, 700, False), (3, 0.5, False, 5000, False),
                                                          (40, 0.3, True, 9000, False), (200, 0.2, False, 20000, False),
                                                          (256, 0.1, True, 30000, False), (120, 1.0, True, 6000, True),
                                                          (130, 1.0, False, 6000, True), (256, 0.6, True, 70000, False),
                                                          (17, 0.9, False, 33, True), (64, 0.0, True, 2049, True)]):
        blk, syms, deepest = hm.block(rng, leaves, skew, wrap, nsym, deep_often=deep, pad_ones=bool(k & 1))
        assert not (skew == 1.0) or deepest > 100
        one(f"tree{k}_K{leaves}_d{deepest}", blk)
        if leaves >= 2:
            one(f"tree{k}_duplicate_leaf", duplicate_leaf(blk))
        # cut payloads and bad headers
        one(f"tree{k}_cut", blk[:len(blk) - max(1, (len(blk) - 10) // 3)])
        one(f"tree{k}_cut1", blk[:-1])
        b = bytearray(blk)
        b[8:10] = (int.from_bytes(blk[8:10], "little") + 2).to_bytes(2, "little")
        one(f"tree{k}_tree_len_plus2", b)
        b = bytearray(blk)
        b[0:8] = (nsym + 5).to_bytes(8, "little")
        one(f"tree{k}_block_len_plus5", b)
        b = bytearray(blk)
        b[8:10] = (-3).to_bytes(2, "little", signed=True)
        one(f"tree{k}_tree_len_negative", b)
    # the decoders' edge cases: the encoder's own layout where there is one, else one of blocks as long as the longest
    for case in dec.cases(oracle):
        streams = [(case.name, case.stream)] + dec.damaged(case)
        nb = len(case.parts)
        if case.encoded is not None:
            n, bs = case.encoded[0].size, case.encoded[1]
        else:
            bs = max(dec.block_facts(p)["len"] for p in case.parts)
            n = nb * bs
        for name, s in streams:
            out.append((name, s, case.offsets, n, bs))
    return out


def decode_outcome(torch, codec, st, st_len, offs, nb, cap, relaxed, sub=None, n=0, bs=0, how="decode"):
    """(error, raw length, delivered bytes) of a decode into a guarded buffer of `cap` bytes"""
    from libhuffman_amd.codec import HuffmanGpuError
    big, out = guarded_out(torch, cap)
    err = 0
    unbuilt = None
    try:
        if how == "decode":
            raw = codec.decode(st, st_len, offs, nb, out, relaxed=relaxed, sub_index=sub, raw_size=n, blocksize=bs)
        else:
            raw, _, unbuilt = codec.decode_build_sub(st, st_len, offs, out, n, bs, sub_index=sub, relaxed=relaxed)
    except HuffmanGpuError as e:
        err, raw = e.err, e.raw
    assert out_guards_intact(big, cap), "output guard"
    return (err, raw, out[:raw].cpu().numpy().tobytes()), unbuilt


@pytest.fixture(scope="module")
def handmade_table(oracle):
    return handmade(oracle)


@pytest.mark.parametrize("relaxed", [False, True], ids=["strict", "relaxed"])
def test_a_built_sub_index_never_changes_a_decode(torch_mod, codec, handmade_table, relaxed):
    torch = torch_mod
    rng = np.random.default_rng(5)
    built_some = 0
    for name, s, offsets, n, bs in handmade_table:
        st = at_offset(torch, s, 1)
        offs = torch.from_numpy(offsets.astype(np.int64)).cuda()
        nb = offsets.size - 1
        assert codec.block_count(n, bs) == nb, name
        cap = n + 4096
        size = codec.sub_index_bytes(n, bs)
        want, _ = decode_outcome(torch, codec, st, s.size, offs, nb, cap, relaxed)

        def guard_ok(buf):
            g = buf.cpu().numpy().view(np.uint8)
            return bool(np.all(g[-(-size // 8) * 8:] == 0x5A))

        # stream only, then decode with what it built
        buf, sub = sub_buffer(torch, size, FILL_A)
        unbuilt, _ = build(torch, codec, "stream_only", st, s.size, offs, n, bs, sub, relaxed=relaxed)
        assert guard_ok(buf), name
        assert 0 <= unbuilt <= nb, name
        built_some += unbuilt < nb
        got, _ = decode_outcome(torch, codec, st, s.size, offs, nb, cap, relaxed, sub=sub, n=n, bs=bs)
        assert got == want, (name, "decode with the built sub-index", got[:2], want[:2])

        # the decode that builds: decode's results exactly, and an index that serves as well
        buf, sub = sub_buffer(torch, size, FILL_B)
        got, unbuilt2 = decode_outcome(torch, codec, st, s.size, offs, nb, cap, relaxed, sub=sub, n=n, bs=bs, how="build")
        assert got == want, (name, "decode_build_sub", got[:2], want[:2])
        assert np.all(buf.cpu().numpy().view(np.uint8)[-(-size // 8) * 8:] == 0xFF), name
        assert unbuilt2 is None or 0 <= unbuilt2 <= nb, name      # (None: the decode raised its error)
        got, _ = decode_outcome(torch, codec, st, s.size, offs, nb, cap, relaxed, sub=sub, n=n, bs=bs)
        assert got == want, (name, "decode with decode_build_sub's sub-index", got[:2], want[:2])

        # from data that is not the stream's: unbuilt or stale rows, the same results
        other = at_offset(torch, rng.integers(0, 256, n, dtype=np.uint8), 3)
        buf, sub = sub_buffer(torch, size, FILL_A)
        build(torch, codec, "from_raw", st, s.size, offs, n, bs, sub, raw=other, relaxed=relaxed)
        assert guard_ok(buf), name
        got, _ = decode_outcome(torch, codec, st, s.size, offs, nb, cap, relaxed, sub=sub, n=n, bs=bs)
        assert got == want, (name, "decode with a sub-index from other data", got[:2], want[:2])
    # the ten random trees as they were written build (but, under the strict limit, the two of 1 025 entries)
    assert built_some >= 8, built_some


# ---- ranges ---------------------------------------------------------------------------------------------------------------
def test_ranges_with_a_built_sub_index(torch_mod, codec, oracle):
    torch = torch_mod
    from libhuffman_amd import datagen
    n, bs = 64 << 20, 65536
    data = datagen.zipf255(n, seed=11)
    want, woffs = oracle.encode(data, bs, with_offsets=True)
    st = torch.from_numpy(want).cuda()
    offs = torch.from_numpy(woffs.astype(np.int64)).cuda()
    nb = woffs.size - 1
    sub, unbuilt = codec.build_sub_index(st, want.size, offs, n, bs, relaxed=True)
    assert unbuilt == 0
    rng = np.random.default_rng(12)
    ranges = []
    for _ in range(400):
        lo = int(rng.integers(0, n))
        ranges.append((lo, min(n, lo + int(rng.choice([1, 100, 5000, 65536, 300000, 2 << 20])))))
    a, ea, ra = codec.decode_ranges(st, want.size, offs, nb, ranges, relaxed=True)
    b, eb, rb = codec.decode_ranges(st, want.size, offs, nb, ranges, relaxed=True, sub_index=sub, raw_size=n, blocksize=bs)
    assert ea == eb == [0] * 400 and ra == rb == [hi - lo for lo, hi in ranges]
    assert torch.equal(a, b)
    o = 0
    host = a.cpu().numpy()
    for lo, hi in ranges[:40]:
        assert np.array_equal(host[o:o + hi - lo], data[lo:hi])
        o += hi - lo


# ---- unbuilt is counted honestly --------------------------------------------------------------------------------------------
def test_one_block_with_a_duplicate_leaf_is_one_unbuilt_block(torch_mod, codec):
    torch = torch_mod
    rng = np.random.default_rng(7)
    blk, syms, _ = hm.block(rng, 12, 0.3, True, 5000)
    s = np.frombuffer(duplicate_leaf(blk), dtype=np.uint8)
    st = at_offset(torch, s, 0)
    offs = torch.tensor([0, s.size], dtype=torch.int64, device="cuda")
    n = syms.size
    raw = at_offset(torch, syms, 0)
    for way in WAYS:
        buf, sub = sub_buffer(torch, codec.sub_index_bytes(n, n), FILL_A)
        unbuilt, _ = build(torch, codec, way, st, s.size, offs, n, n, sub, raw=raw)
        assert unbuilt == 1, way
        assert bool((buf == FILL_A).all()), (way, "a tree that does not parse leaves its row alone")
    # and the block as it was written builds
    good = at_offset(torch, np.frombuffer(blk, dtype=np.uint8), 0)
    for way in WAYS:
        buf, sub = sub_buffer(torch, codec.sub_index_bytes(n, n), FILL_A)
        unbuilt, _ = build(torch, codec, way, good, len(blk), offs, n, n, sub, raw=raw)
        assert unbuilt == 0, way

"""GPU tests of the batch calls (hufgpu_encode_batch / hufgpu_decode_batch, GpuCodec.encode_batch / decode_batch).

A batch must be exactly the items handled one by one: every item's stream is the single-item hufgpu_encode stream and
the oracle's, the block index is the single indexes shifted into place, the sub-index rows are hufgpu_encode_sub's
rows, and every item's decode result - error, bytes delivered and the bytes of its slot - is what hufgpu_decode of the
item alone into the same slot returns.  Bytes outside the decoded part of every slot are never written.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import sub_index_ref as sref
from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

GUARD = 0xA5
HUFE_OK, HUFE_MEMORY, HUFE_ARGUMENT = 0, 1, 2


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
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")


def packed(torch, items, lead=1):
    """the items back to back in a device buffer, the first at byte `lead` of it (odd addresses for lead = 1)"""
    total = sum(int(x.size) for x in items)
    buf = torch.zeros(total + lead + 16, dtype=torch.uint8, device="cuda")
    if total:
        buf[lead:lead + total] = dev(torch, np.concatenate(items))
    return buf[lead:lead + total]


def single_encode(torch, codec, item, bs, sub=False):
    d = dev(torch, item)
    s = codec.new_sub_index(d.numel(), bs) if sub and d.numel() else None
    if d.numel() == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64), None
    stream, offs, _ = codec.encode(d, bs, sub_index=s)
    return stream.cpu().numpy(), offs.cpu().numpy(), s


def check_encode(torch, codec, oracle, items, bs, sub=False):
    """encode_batch == item-by-item hufgpu_encode == oracle; block index, item offsets and sub-index rows match"""
    lens = [int(x.size) for x in items]
    batch = codec.encode_batch(packed(torch, items), lens, bs, sub_index=sub)
    nb, rbs, bound, subb = codec.batch_geometry(lens, bs)
    assert batch.nblocks == nb and batch.row_blocksize == rbs and batch.item_lens == lens
    stream = batch.stream.cpu().numpy()
    offs = batch.offsets.cpu().numpy()
    assert offs.size == nb + 1 and offs[-1] == stream.size == batch.item_offsets[-1]
    if sub:
        subbuf = batch.sub_index.cpu().numpy().view(np.uint8)[:subb]
        tpb = -(-rbs // sref.TILE)
        gpb = (-(-rbs // sref.GROUP) + 7) & ~7
        tiles = subbuf[: nb * tpb * 8].view(np.uint64)
        groups = subbuf[nb * tpb * 8: nb * tpb * 8 + nb * gpb * 2].view(np.uint16)
        lens_arr = subbuf[nb * tpb * 8 + nb * gpb * 2:]
    for i, item in enumerate(items):
        got = stream[batch.item_offsets[i]:batch.item_offsets[i + 1]]
        want, want_offs = oracle.encode(item, bs, with_offsets=True) if item.size else (np.zeros(0, np.uint8), np.zeros(1))
        assert np.array_equal(got, want), f"item {i} ({item.size} bytes): stream differs from the oracle"
        one, one_offs, one_sub = single_encode(torch, codec, item, bs, sub)
        assert np.array_equal(got, one), f"item {i}: stream differs from hufgpu_encode"
        b0, b1 = batch.item_blocks[i], batch.item_blocks[i + 1]
        assert b1 - b0 == codec.block_count(item.size, bs)
        assert np.array_equal(offs[b0:b1 + 1] - batch.item_offsets[i], one_offs), f"item {i}: block index"
        if sub and item.size:
            exp = sref.expected(want, want_offs, item, bs)
            for k in range(b1 - b0):
                b = b0 + k
                t = exp.lay.tpb
                g = exp.lay.gpb
                wt = exp.w_tiles[k * t:(k + 1) * t]
                wg = exp.w_groups[k * g:(k + 1) * g]
                wl = exp.w_lens[k * 256:(k + 1) * 256]
                nt, ng = int(wt.sum()), int(wg.sum())
                assert np.array_equal(tiles[b * tpb:b * tpb + nt], exp.tiles[k * t:k * t + nt]), f"item {i} block {k}: tiles"
                assert np.array_equal(groups[b * gpb:b * gpb + ng], exp.groups[k * g:k * g + ng]), f"item {i} block {k}: groups"
                assert np.array_equal(lens_arr[b * 256:(b + 1) * 256][wl], exp.lens[k * 256:(k + 1) * 256][wl])
                # and hufgpu_encode_sub's own rows say the same
                ones = one_sub.cpu().numpy().view(np.uint8)
                lay = sref.layout(item.size, bs)
                st_t, st_g, st_l = sref.views(ones, lay)
                assert np.array_equal(tiles[b * tpb:b * tpb + nt], st_t[k * t:k * t + nt])
                assert np.array_equal(groups[b * gpb:b * gpb + ng], st_g[k * g:k * g + ng])
    return batch


def guarded_slots(lens, gap=13, lead=5):
    """slots with `gap` spare bytes behind every item (they must stay untouched), the first at byte `lead`"""
    oo = [lead]
    for n in lens:
        oo.append(oo[-1] + n + gap)
    return oo


def decode_into_guard(torch, codec, batch, oo, relaxed=False):
    out = torch.full((oo[-1] + 7,), GUARD, dtype=torch.uint8, device="cuda")
    _, errs, raws = codec.decode_batch(batch, out=out, out_offsets=oo, relaxed=relaxed)
    return out.cpu().numpy(), errs, raws


def check_round_trip(torch, codec, batch, items, relaxed=False):
    lens = [int(x.size) for x in items]
    oo = guarded_slots(lens)
    got, errs, raws = decode_into_guard(torch, codec, batch, oo, relaxed)
    assert errs == [0] * len(items) and raws == lens
    want = np.full(got.size, GUARD, np.uint8)
    for i, item in enumerate(items):
        want[oo[i]:oo[i] + item.size] = item
    assert np.array_equal(got, want), "round trip: item bytes wrong or a byte outside the items written"


def zipf(n, seed):
    return datagen.zipf255(n, seed=seed) if n else np.zeros(0, np.uint8)


# one case per encode route: (blocksize, item lengths) -> the row blocksize picks the kernels
ROUTES = [
    (4096, [3 * 4096 + 5, 1, 0, 4096, 777, 4095]),           # hist_tree (16-bit counters), short pack
    (16384, [40000, 16383, 0, 16385, 2]),                      # hist_tree, short pack
    (65536, [65536 * 2 + 1, 300, 0, 65535]),                   # lane counters + tree_wave, short pack
    (131072, [131072 + 9, 5000, 131071]),                      # lane counters, 64-bit pack
    (262144, [262144 + 3, 100, 0, 200000]),                    # lane counters, 64-bit pack, longer rows
    (0, [50000, 3, 0, 12345, 1]),                               # blocksize 0: every item one block
]


@pytest.mark.parametrize("bs,lens", ROUTES, ids=[f"bs{r[0]}" for r in ROUTES])
def test_routes_match_single_items_and_oracle(torch_mod, codec, oracle, bs, lens):
    items = [zipf(n, 100 + i) for i, n in enumerate(lens)]
    batch = check_encode(torch_mod, codec, oracle, items, bs, sub=True)
    check_round_trip(torch_mod, codec, batch, items)
    batch.sub_index = None
    check_round_trip(torch_mod, codec, batch, items)


def test_blocks_of_2_mib_go_item_by_item(torch_mod, codec, oracle):
    bs = 1 << 21
    items = [zipf((1 << 21) + (1 << 19) + 3, 7), zipf(1000, 8), np.zeros(0, np.uint8), datagen.logtext(300000)]
    batch = check_encode(torch_mod, codec, oracle, items, bs)
    assert batch.row_blocksize == bs
    check_round_trip(torch_mod, codec, batch, items)
    with pytest.raises(Exception):
        codec.encode_batch(packed(torch_mod, items), [x.size for x in items], bs, sub_index=True)


def mixed_items(rng):
    return [
        np.zeros(0, np.uint8),
        np.array([0x33], np.uint8),
        np.full(5000, 0x41, np.uint8),                     # one symbol
        sref.all_values(rng, 9000),                         # all 256 byte values: a 1025-entry tree
        np.zeros(0, np.uint8),
        sref.chain(rng, 200000, 25),                        # codes over 24 bits: the 64-bit pack
        zipf(70001, 3),
        sref.two_values(rng, 333),
        np.array([7, 7], np.uint8),
    ]


@pytest.mark.parametrize("bs", [4096, 262144])
def test_mixed_batch(torch_mod, codec, oracle, bs):
    rng = np.random.default_rng(bs)
    items = mixed_items(rng)
    batch = check_encode(torch_mod, codec, oracle, items, bs, sub=True)
    check_round_trip(torch_mod, codec, batch, items, relaxed=True)
    # strict trees: the all-256 item fails alone, as hufgpu_decode of it does
    lens = [x.size for x in items]
    oo = guarded_slots(lens)
    got, errs, raws = decode_into_guard(torch_mod, codec, batch, oo)
    plain = copy.copy(batch)
    plain.sub_index = None                              # (the failing block fails in its header: no decoder touches it)
    for i, item in enumerate(items):
        single = single_decode(torch_mod, codec, plain, i, oo[i + 1] - oo[i])
        assert (errs[i], raws[i]) == single[:2], f"item {i}"
        assert np.array_equal(got[oo[i]:oo[i + 1]], single[2]), f"item {i}: slot contents"
    assert errs[3] != 0 and all(e == 0 for j, e in enumerate(errs) if j != 3)


def single_decode(torch, codec, batch, i, slot, relaxed=False):
    """hufgpu_decode of item i alone into a slot of `slot` bytes filled with GUARD -> (err, raw, slot bytes).  With the
    batch's sub-index: hufgpu_decode_sub with the item's rows of it (items of whole blocks only: then a single encode's
    layout is the batch's rows of the item)"""
    b0, b1 = batch.item_blocks[i], batch.item_blocks[i + 1]
    out = torch.full((max(slot, 1),), GUARD, dtype=torch.uint8, device="cuda")
    raw = C.c_uint64(0)
    offs = batch.offsets[b0:b1 + 1].contiguous()
    flags = 1 if relaxed else 0
    if batch.sub_index is None:
        err = codec.lib.hufgpu_decode(codec._ctx, batch.stream.data_ptr(), batch.stream_len, offs.data_ptr(), b1 - b0,
                                      out.data_ptr(), slot, flags, C.byref(raw), None)
    else:
        n, bs = batch.item_lens[i], batch.blocksize
        assert bs == batch.row_blocksize and n >= bs
        rbs, nb = batch.row_blocksize, batch.nblocks
        tpb, gpb = -(-rbs // sref.TILE), (-(-rbs // sref.GROUP) + 7) & ~7
        whole = batch.sub_index.view(torch.uint8)
        g0, l0 = nb * tpb * 8, nb * tpb * 8 + nb * gpb * 2
        rows = torch.cat([whole[b0 * tpb * 8:b1 * tpb * 8], whole[g0 + b0 * gpb * 2:g0 + b1 * gpb * 2],
                          whole[l0 + b0 * 256:l0 + b1 * 256]])
        assert rows.numel() == codec.sub_index_bytes(n, bs)
        err = codec.lib.hufgpu_decode_sub(codec._ctx, batch.stream.data_ptr(), batch.stream_len, offs.data_ptr(), n, bs,
                                          rows.data_ptr(), out.data_ptr(), slot, flags, C.byref(raw), None)
    return int(err), int(raw.value), out.cpu().numpy()[:slot]


def damaged(torch, batch, pos, xor):
    st = batch.stream.clone()
    st[pos] ^= xor
    from libhuffman_amd.codec import EncodedBatch
    return EncodedBatch(st, batch.offsets, batch.item_blocks, batch.item_offsets, batch.item_lens, batch.blocksize,
                        batch.row_blocksize, batch.sub_index)


@pytest.mark.parametrize("where", ["payload_bit", "header_len", "header_tree_len", "tree"])
def test_damaged_middle_item(torch_mod, codec, oracle, where):
    bs = 4096
    items = [zipf(10000 + 37 * i, 20 + i) for i in range(7)]
    batch = codec.encode_batch(packed(torch_mod, items), [x.size for x in items], bs, sub_index=True)
    mid = 3
    o0 = batch.item_offsets[mid]
    blk = batch.item_blocks[mid] + 1                       # the item's second block
    bo = int(batch.offsets[blk].item())
    tl = int.from_bytes(bytes(batch.stream[bo + 8:bo + 10].cpu().numpy()), "little")
    pos, xor = {"payload_bit": (bo + 10 + 2 * tl + 40, 0x10), "header_len": (bo, 0x01), "header_tree_len": (bo + 8, 0x04),
                "tree": (bo + 10 + 3, 0x80)}[where]
    bad = damaged(torch_mod, batch, pos, xor)
    lens = [x.size for x in items]
    oo = guarded_slots(lens)
    for use_sub in (True, False):
        if not use_sub:
            bad.sub_index = None
        got, errs, raws = decode_into_guard(torch_mod, codec, bad, oo)
        err1, raw1, slot1 = single_decode(torch_mod, codec, bad, mid, oo[mid + 1] - oo[mid])
        assert (errs[mid], raws[mid]) == (err1, raw1)
        diff = np.flatnonzero(got[oo[mid]:oo[mid + 1]] != slot1)
        assert diff.size == 0, f"damaged item: slot differs from the single call's at {diff[:8]} (raw {raw1})"
        item_stream = bad.stream[o0:batch.item_offsets[mid + 1]].cpu().numpy()
        oerr, oout, _ = oracle.decode(item_stream, oo[mid + 1] - oo[mid])
        # (a damaged block length moves the block's end in a raw stream; the index keeps it: the oracle, which reads the
        # raw stream, then parses the next block elsewhere - the single indexed call is the yardstick there)
        if not where.startswith("header"):
            assert (errs[mid], raws[mid]) == (oerr, oout.size) and np.array_equal(got[oo[mid]:oo[mid] + raws[mid]], oout)
        for i, item in enumerate(items):
            if i == mid:
                continue
            assert (errs[i], raws[i]) == (0, item.size)
            assert np.array_equal(got[oo[i]:oo[i] + item.size], item)
            assert np.all(got[oo[i] + item.size:oo[i + 1]] == GUARD)
        assert np.all(got[:oo[0]] == GUARD) and np.all(got[oo[-1]:] == GUARD)


def test_undersized_slot_fails_alone(torch_mod, codec):
    bs = 4096
    items = [zipf(9000 + i, 40 + i) for i in range(5)]
    batch = codec.encode_batch(packed(torch_mod, items), [x.size for x in items], bs)
    oo = [0]
    for i, x in enumerate(items):
        oo.append(oo[-1] + x.size - (1 if i == 2 else 0))
    out = torch_mod.full((oo[-1],), GUARD, dtype=torch_mod.uint8, device="cuda")
    _, errs, raws = codec.decode_batch(batch, out=out, out_offsets=oo)
    got = out.cpu().numpy()
    err1, raw1, slot1 = single_decode(torch_mod, codec, batch, 2, oo[3] - oo[2])
    assert errs[2] == HUFE_MEMORY and (errs[2], raws[2]) == (err1, raw1)
    assert np.array_equal(got[oo[2]:oo[3]], slot1)
    for i in (0, 1, 3, 4):
        assert errs[i] == 0 and raws[i] == items[i].size and np.array_equal(got[oo[i]:oo[i + 1]], items[i])


def test_stale_or_garbage_sub_index_changes_nothing(torch_mod, codec):
    bs = 16384
    rng = np.random.default_rng(5)
    items = [zipf(int(n), 60 + i) for i, n in enumerate(rng.integers(0, 50000, 12))]
    lens = [x.size for x in items]
    batch = codec.encode_batch(packed(torch_mod, items), lens, bs, sub_index=True)
    other = codec.encode_batch(packed(torch_mod, [datagen.logtext(x.size) for x in items]), lens, bs, sub_index=True)
    oo = guarded_slots(lens)
    ref = decode_into_guard(torch_mod, codec, batch, oo)
    for fill in ("garbage", "zeros", "stale"):
        if fill == "garbage":
            batch.sub_index.copy_(torch_mod.from_numpy(rng.integers(-2**62, 2**62, batch.sub_index.numel())).cuda())
        elif fill == "zeros":
            batch.sub_index.zero_()
        else:
            batch.sub_index.copy_(other.sub_index)
        got = decode_into_guard(torch_mod, codec, batch, oo)
        assert got[1:] == ref[1:] and np.array_equal(got[0], ref[0]), fill


def test_ten_thousand_items(torch_mod, codec, oracle):
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 5001, 10000)
    data = datagen.zipf255(int(lens.sum()), seed=12)
    cut = np.concatenate([[0], np.cumsum(lens)])
    items = [data[cut[i]:cut[i + 1]] for i in range(lens.size)]
    bs = 4096
    batch = codec.encode_batch(packed(torch_mod, items), lens.tolist(), bs, sub_index=True)
    want = np.concatenate([oracle.encode(x, bs) for x in items if x.size])
    assert np.array_equal(batch.stream.cpu().numpy(), want)
    out, errs, raws = codec.decode_batch(batch)
    assert errs == [0] * lens.size and raws == lens.tolist()
    assert np.array_equal(out[: data.size].cpu().numpy(), data)


def test_two_unsynchronised_encodes(torch_mod, codec):
    """two enqueue-only encodes back to back: the second reuses (and rewrites) the caller's host length array at once"""
    torch = torch_mod
    bs = 4096
    a = [zipf(n, 80 + i) for i, n in enumerate([7000, 0, 12000, 5])]
    b = [datagen.logtext(n) for n in [30000, 1, 4097, 4096, 9]]
    outs = []
    lens = (C.c_uint64 * 8)()
    for items in (a, b):
        for i, x in enumerate(items):
            lens[i] = x.size
        nb, rbs, bound, _ = codec.batch_geometry([x.size for x in items], bs)
        src = packed(torch, items)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        offs = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
        ioffs = torch.empty(len(items) + 1, dtype=torch.int64, device="cuda")
        err = codec.lib.hufgpu_encode_batch(codec._ctx, src.data_ptr(), len(items), lens, bs, out.data_ptr(), bound,
                                            offs.data_ptr(), ioffs.data_ptr(), None, None, None)
        assert err == 0
        outs.append((items, src, out, offs, ioffs))
        for i in range(8):
            lens[i] = 999999                                     # the call has returned: the array is the caller's again
    torch.cuda.synchronize()
    for items, _, out, offs, ioffs in outs:
        io = ioffs.cpu().numpy()
        st = out.cpu().numpy()
        for i, x in enumerate(items):
            one, one_offs, _ = single_encode(torch, codec, x, bs)
            assert np.array_equal(st[io[i]:io[i + 1]], one)


def test_batch_from_streams(torch_mod, codec):
    bs = 8192
    items = [zipf(n, 90 + i) for i, n in enumerate([20000, 0, 8192, 1, 33333])]
    parts = []
    for x in items:
        if x.size:
            stream, offs, length = codec.encode(dev(torch_mod, x), bs)
            parts.append((stream.clone(), offs.clone(), x.size))
        else:
            parts.append((torch_mod.empty(0, dtype=torch_mod.uint8, device="cuda"),
                          torch_mod.zeros(1, dtype=torch_mod.int64, device="cuda"), 0))
    batch = codec.batch_from_streams(parts)
    assert batch.nitems == len(items) and batch.item_lens == [x.size for x in items]
    check_round_trip(torch_mod, codec, batch, items)
    direct = codec.encode_batch(packed(torch_mod, items), [x.size for x in items], bs)
    assert torch_mod.equal(batch.stream, direct.stream) and torch_mod.equal(batch.offsets, direct.offsets)
    assert batch.item_blocks == direct.item_blocks and batch.item_offsets == direct.item_offsets


def test_whole_batch_is_one_stream(torch_mod, codec):
    items = [zipf(n, 120 + i) for i, n in enumerate([5000, 0, 70000, 3, 65536])]
    batch = codec.encode_batch(packed(torch_mod, items), [x.size for x in items], 65536)
    total = sum(x.size for x in items)
    out = torch_mod.empty(total, dtype=torch_mod.uint8, device="cuda")
    raw = codec.decode(batch.stream, batch.stream_len, batch.offsets, batch.nblocks, out)
    assert raw == total and np.array_equal(out.cpu().numpy(), np.concatenate(items))


def test_argument_errors(torch_mod, codec):
    torch = torch_mod
    items = [zipf(3000, 1), zipf(5000, 2)]
    batch = codec.encode_batch(packed(torch, items), [3000, 5000], 4096)
    from libhuffman_amd.codec import HuffmanGpuError
    with pytest.raises(HuffmanGpuError):
        codec.decode_batch(batch, out_offsets=[0, 3000, 2000])      # slots must not go backwards
    with pytest.raises(ValueError):
        codec.encode_batch(packed(torch, items), [3000, 4999], 4096)
    lens = (C.c_uint64 * 2)(3000, 5000)
    out = torch.empty(100, dtype=torch.uint8, device="cuda")
    src = packed(torch, items)
    assert codec.lib.hufgpu_encode_batch(codec._ctx, src.data_ptr(), 2, lens, 4096, out.data_ptr(), 100, None, None,
                                         None, None, None) == HUFE_ARGUMENT      # output below the bound

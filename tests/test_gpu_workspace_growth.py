"""GPU tests of the context's workspaces as they grow (csrc/host/ctx.hpp, the table; csrc/host/workspace.hpp).

One long-lived context runs sequences of calls whose sizes cross each group's growth boundary - with 1 KiB blocks a
first call of 1 block leaves a capacity of 17 (n + n/8 + 16), so 40 blocks grow it and 400 grow it again - and every
call's results are compared, bit for bit, with those of the same call on a FRESH context, whose first growth is the
path every other GPU test runs.  Where there is an original, decoded bytes are also compared with it.  Exact equality
throughout, no tolerance.  Inputs are made once per module by a third context and never changed.
"""
import ctypes as C

import numpy as np
import pytest

from libhuffman_amd import datagen

pytestmark = pytest.mark.gpu

BS = 1024
DISC_CHUNK = 16384                       # bytes of stream one discovery workgroup scans (kernels/discover.hpp)
BIG_BLOCK = 1 << 22                      # HUF_BIG_BLOCK (kernels/hist_chunk.hpp)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def helper(torch_mod):
    """makes the inputs: its own workspaces are not under test"""
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def longlived(torch_mod):
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    yield c
    c.close()


def host(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else x


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"{what}: result {i} differs from the fresh context's"
        else:
            assert g == w, f"{what}: result {i} is {g!r}, the fresh context's {w!r}"


def both(longlived, step, what):
    """step(codec) -> list of host results, on the long-lived context and on a fresh one"""
    from libhuffman_amd.codec import GpuCodec
    got = [host(x) for x in step(longlived)]
    fresh = GpuCodec(0)
    try:
        want = [host(x) for x in step(fresh)]
    finally:
        fresh.close()
    same(got, want, what)
    return got


_inputs = {}


def data_of(n, seed=3):
    if (n, seed) not in _inputs:
        _inputs[n, seed] = datagen.zipf255(n, seed=seed)
    return _inputs[n, seed]


_encoded = {}


class Enc:
    pass


def encoded(torch, helper, n, bs=BS):
    """one encode, with its sub-index, per size for the whole module"""
    if (n, bs) not in _encoded:
        e = Enc()
        e.data = data_of(n)
        e.n, e.bs, e.nb = n, bs, helper.block_count(n, bs)
        e.sub = torch.zeros_like(helper.new_sub_index(n, bs))
        stream, e.offsets, e.length = helper.encode(torch.from_numpy(e.data.copy()).cuda(), bs, sub_index=e.sub)
        e.stream = torch.zeros(e.length + 64, dtype=torch.uint8, device="cuda")     # (16-byte aligned, as raw streams must be)
        e.stream[:e.length] = stream
        _encoded[n, bs] = e
    return _encoded[n, bs]


def encode_decode(torch, n):
    data = data_of(n)

    def step(codec):
        d = torch.from_numpy(data.copy()).cuda()
        nb = codec.block_count(n, BS)
        stream, offs, length = codec.encode(d, BS)
        out = torch.zeros(n, dtype=torch.uint8, device="cuda")
        raw = codec.decode(stream, length, offs, nb, out)
        sub = torch.zeros_like(codec.new_sub_index(n, BS))
        stream2, offs2, length2 = codec.encode(d, BS, sub_index=sub)
        out2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        raw2 = codec.decode(stream2, length2, offs2, nb, out2, sub_index=sub, raw_size=n, blocksize=BS)
        assert raw == n and raw2 == n and np.array_equal(host(out), data) and np.array_equal(host(out2), data), f"round trip of {n} bytes"
        return [stream, offs, length, out, stream2, offs2, length2, sub, out2]
    return step


def test_encode_and_indexed_decode_as_the_block_count_grows_and_shrinks(torch_mod, longlived):
    for n in (BS, 40 * BS, 400 * BS, 3 * BS):
        both(longlived, encode_decode(torch_mod, n), f"encode + decode of {n} bytes")


def raw_stream(torch, e, index=True):
    def step(codec):
        out = torch.zeros(e.n, dtype=torch.uint8, device="cuda")
        err, raw, used = codec.decode_stream(e.stream, e.length, e.length, out)
        assert (err, raw, used) == (0, e.n, e.length) and np.array_equal(host(out), e.data), f"raw-stream decode of {e.n} bytes"
        res = [err, raw, used, out]
        if index:
            d_index, nb, consumed = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
            rc = codec.lib.hufgpu_block_index(codec._ctx, C.c_void_p(e.stream.data_ptr()), C.c_uint64(e.length), C.c_uint64(e.length),
                                              C.c_uint32(0), C.byref(d_index), C.byref(nb), C.byref(consumed), None)
            assert rc == 0, f"block index of {e.n} bytes"
            idx = torch.zeros(nb.value + 1, dtype=torch.int64, device="cuda")      # (the context's array lives until its next decode)
            if nb.value:
                assert codec.lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(idx.data_ptr()), d_index, C.c_uint64(8 * (nb.value + 1))) == 0
            res += [int(nb.value), int(consumed.value), idx]
        return res
    return step


def test_raw_streams_as_the_discovery_groups_grow(torch_mod, helper, longlived):
    short, long_ = encoded(torch_mod, helper, 4 * BS), encoded(torch_mod, helper, 400 * BS)
    assert 4096 <= short.length <= DISC_CHUNK and long_.length >= 18 * DISC_CHUNK, (short.length, long_.length)
    for e in (short, long_, short):
        both(longlived, raw_stream(torch_mod, e), f"raw stream of {e.length} bytes")


def test_single_blocks_of_many_mib_as_the_lane_and_sub_index_groups_grow(torch_mod, helper, longlived):
    torch = torch_mod
    for n in (BIG_BLOCK, BIG_BLOCK + BIG_BLOCK // 2):
        e = encoded(torch, helper, n, bs=0)
        both(longlived, raw_stream(torch, e, index=False), f"one block of {n} bytes as a raw stream")

        def rows(codec, e=e):                # the sub-index builders' chunk arrays (blocks of 2 MiB and more are chunked)
            sub = torch.zeros_like(codec.new_sub_index(e.n, 0))
            _, unbuilt = codec.build_sub_index(e.stream, e.length, e.offsets, e.n, 0, raw=torch.from_numpy(e.data.copy()).cuda(), sub_index=sub)
            return [sub, unbuilt]
        both(longlived, rows, f"sub-index of one block of {n} bytes")


def batch(torch, items, blocks, sub):
    lens = [blocks * BS] * items
    data = data_of(items * blocks * BS, seed=11)

    def step(codec):
        b = codec.encode_batch(torch.from_numpy(data.copy()).cuda(), lens, BS, sub_index=sub)
        out, errs, raws = codec.decode_batch(b, out=torch.zeros(data.size, dtype=torch.uint8, device="cuda"))
        assert errs == [0] * items and raws == lens and np.array_equal(host(out), data), f"batch of {items} x {blocks} blocks"
        return [b.stream, b.offsets, list(b.item_offsets), out, errs, raws]
    return step


@pytest.mark.parametrize("sub", [False, True])
def test_batches_whose_two_dimensions_grow_separately(torch_mod, longlived, sub):
    for items, blocks in ((2, 1), (2, 40), (100, 1), (1, 1)):
        both(longlived, batch(torch_mod, items, blocks, sub), f"batch of {items} items x {blocks} blocks")


def ranges_of(e, count):
    rng = np.random.default_rng(count)
    lo = rng.integers(0, e.n - 1, size=count)
    ln = rng.integers(1, 3 * BS, size=count)
    return [(0, e.n)] if count == 1 else [(int(a), int(min(e.n, a + b))) for a, b in zip(lo, ln)]


def read_ranges(torch, e, count, tiles):
    ranges = ranges_of(e, count)

    def step(codec):
        total = sum(hi - lo for lo, hi in ranges)
        out, errs, raws = codec.decode_ranges(e.stream, e.length, e.offsets, e.nb, ranges, out=torch.zeros(total, dtype=torch.uint8, device="cuda"),
                                              sub_index=e.sub, raw_size=e.n, blocksize=e.bs, tiles=tiles)
        want = np.concatenate([e.data[lo:hi] for lo, hi in ranges])
        assert errs == [0] * count and raws == [hi - lo for lo, hi in ranges] and np.array_equal(host(out), want), f"{count} ranges"
        return [out, errs, raws]
    return step


def write_ranges(torch, e, count):
    step_ = e.n // count                                                # (overwritten ranges must not overlap)
    keep = [(0, e.n)] if count == 1 else [(i * step_ + 3, i * step_ + 4 + i % (step_ - 4)) for i in range(count)]
    new = data_of(sum(hi - lo for lo, hi in keep), seed=21)

    def step(codec):
        stream, length, offs, sub, touched = codec.update_ranges(e.stream, e.length, e.offsets, e.nb, keep, torch.from_numpy(new.copy()).cuda(),
                                                                 sub_index=e.sub, raw_size=e.n, blocksize=e.bs)
        out = torch.zeros(e.n, dtype=torch.uint8, device="cuda")
        raw = codec.decode(stream, length, offs, e.nb, out)
        want, at = e.data.copy(), 0
        for lo, hi in keep:
            want[lo:hi] = new[at:at + hi - lo]
            at += hi - lo
        assert raw == e.n and np.array_equal(host(out), want), f"{len(keep)} ranges overwritten"
        return [stream, length, offs, touched, out]
    return step


def test_ranges_and_updates_with_a_batch_decode_in_between(torch_mod, helper, longlived):
    torch = torch_mod
    e40, e400 = encoded(torch, helper, 40 * BS), encoded(torch, helper, 400 * BS)
    for e, count in ((e40, 1), (e40, 200), (None, 0), (e400, 1)):
        if e is None:                                                   # the batch group is shared with the range calls
            both(longlived, batch(torch, 3, 2, False), "batch between the range calls")
            continue
        both(longlived, read_ranges(torch, e, count, tiles=False), f"{count} ranges of {e.nb} blocks")
        both(longlived, read_ranges(torch, e, count, tiles=True), f"{count} ranges of {e.nb} blocks by tiles")
        both(longlived, write_ranges(torch, e, count), f"{count} ranges of {e.nb} blocks overwritten")


def gather(torch, e, count, length):
    pos = np.random.default_rng(count).integers(0, e.n - length, size=count)

    def step(codec):
        positions = torch.from_numpy(pos).cuda() + 0
        out, errs, raws = codec.gather(e.stream, e.length, e.offsets, e.nb, positions, length, sub_index=e.sub, raw_size=e.n, blocksize=e.bs,
                                       out=torch.zeros((count, length), dtype=torch.uint8, device="cuda"))
        out, errs, raws = host(out), host(errs), host(raws)
        for i in np.flatnonzero(errs == 0):
            assert raws[i] == length and np.array_equal(out[i], e.data[pos[i]:pos[i] + length]), f"record {i}"
        return [out, errs, raws]
    return step


def find(torch, e):
    values = [0, 1, 7]

    def step(codec):
        pos, totals, errs, counts = codec.find_bytes(e.stream, e.length, e.offsets, e.nb, e.sub, e.n, e.bs, values, max_positions=e.n,
                                                     block_counts=True)
        totals, errs = host(totals), host(errs)
        pos = host(pos)[:int(totals[1])]
        if not errs.any():
            assert np.array_equal(pos, np.flatnonzero(np.isin(e.data, values))), "positions"
        return [pos, totals, errs, np.where(errs == 0, host(counts), -1)]     # (a block not served has no count)
    return step


def append(torch, helper, e, extra):
    more = data_of(extra, seed=31)

    def step(codec):
        cap = e.length + codec.encode_bound(e.n % BS + extra, BS)
        stream = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        stream[:e.length] = e.stream[:e.length]
        nb_new = codec.block_count(e.n + extra, BS)
        offsets = torch.zeros(nb_new + 1, dtype=torch.int64, device="cuda")
        offsets[:e.nb + 1] = e.offsets
        stream, offsets, length, raw_size, sub = codec.append(stream, e.length, offsets, e.n, BS, torch.from_numpy(more.copy()).cuda(),
                                                              sub_index=e.sub, new_sub_index=True)
        out = torch.zeros(raw_size, dtype=torch.uint8, device="cuda")
        raw = codec.decode(stream, length, offsets, nb_new, out)
        assert raw == e.n + extra and np.array_equal(host(out), np.concatenate([e.data, more])), f"append of {extra} bytes"
        return [stream[:length], offsets[:nb_new + 1], length, raw_size, out]
    return step


def build_sub(torch, e):
    def step(codec):
        sub = torch.zeros_like(codec.new_sub_index(e.n, e.bs))
        _, unbuilt = codec.build_sub_index(e.stream, e.length, e.offsets, e.n, e.bs, sub_index=sub)
        out = torch.zeros(e.n, dtype=torch.uint8, device="cuda")
        raw = codec.decode(e.stream, e.length, e.offsets, e.nb, out, sub_index=sub, raw_size=e.n, blocksize=e.bs)
        assert raw == e.n and np.array_equal(host(out), e.data), "decode with the built sub-index"
        return [sub, unbuilt, out]
    return step


def test_gather_find_append_and_build_sub_index_small_then_larger(torch_mod, helper, longlived):
    torch = torch_mod
    small, large = encoded(torch, helper, 3 * BS + 500), encoded(torch, helper, 400 * BS)
    both(longlived, gather(torch, small, 3, 33), "gather of 3 records")
    both(longlived, gather(torch, large, 2000, 33), "gather of 2000 records")
    both(longlived, gather(torch, small, 3, 33), "gather of 3 records again")
    for e in (small, large, small):
        both(longlived, find(torch, e), f"find in {e.nb} blocks")
    both(longlived, append(torch, helper, small, 2 * BS + 100), "append to 4 blocks")
    both(longlived, append(torch, helper, encoded(torch, helper, 40 * BS), 300 * BS), "append of 300 blocks")
    for e in (small, large, small):
        both(longlived, build_sub(torch, e), f"sub-index of {e.nb} blocks")


def test_the_first_encode_and_decode_again_then_destroy(torch_mod, longlived):
    both(longlived, encode_decode(torch_mod, BS), "the first encode + decode, after everything else")
    both(longlived, encode_decode(torch_mod, 400 * BS), "and the largest")
    longlived.close()                                                   # (the fixture's close after it is harmless)

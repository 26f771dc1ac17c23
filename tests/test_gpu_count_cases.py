"""Every case of tests/count_cases.py - blocks on the branches of the counting bodies, with histograms whose tree shows a
miscount of one - through every route that counts: hufgpu_histogram directly, and the encoder's fused, lane-private,
chunked, batch and row routes, where the stream and the block index are the oracle's byte for byte and the indexed decode
gives the data back.  A miscount still round-trips through our own decoder, so a difference is reported as the first
differing entry of the serialised tree.  HUF_GPU_FUSED_HIST=1 and the builds with other tunables run in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import count_cases
from count_cases_fused_child import case_blocks, encode_case, encode_items, explain, lanes_batch_items, on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def table():
    return [(c, c.data()) for c in count_cases.cases()]


@pytest.mark.parametrize("offset", [0, 5])
def test_direct_counts_are_bincount(torch_mod, codec, table, offset):
    """hist256_kernel shares hist_add_chunk with the fused kernel and is public ABI (hufgpu_histogram)"""
    for case, data in table:
        hist = codec.histogram(on_device(torch_mod, data, offset), case.bs).cpu().numpy().astype(np.int64)
        nb = -(-case.n // case.bs)
        want = np.stack([np.bincount(data[b * case.bs:(b + 1) * case.bs], minlength=256) for b in range(nb)])
        bad = np.argwhere(hist != want)
        assert bad.size == 0, (case.name, "block, value", bad[0].tolist(), "ours / bincount",
                               int(hist[tuple(bad[0])]), int(want[tuple(bad[0])]))


ROUTES = {
    "fused": "hist_tree_kernel, 16-bit counters",
    "lanes": "hist_lanes_kernel + tree_wave_kernel",
    "lanes_big": "hist_lanes_kernel at 2 MiB - 1, one lane's counter loaded",
    "chunked": "chunk_hist_kernel + block_hist32_kernel / block_hist_kernel",
}


@pytest.mark.parametrize("group", list(ROUTES))
def test_every_case_is_the_oracles_stream(torch_mod, codec, oracle, table, group):
    ran = 0
    for case, data in table:
        if case.group == group:
            what = encode_case(torch_mod, codec, oracle, case, data, ROUTES[group])
            if what:
                pytest.fail(what)
            ran += 1
    assert ran >= 2, ran


def test_the_fused_blocks_as_items_of_one_batch(torch_mod, codec, oracle, table):
    """blocksize 0, every item below 32 KiB: hist_tree_batch_kernel; item starts fall where concatenation puts them"""
    items = [x for c, d in table if c.group == "fused" for x in case_blocks(c, d)]
    assert len(items) >= 200 and max(d.size for _, d in items) < count_cases.HL_MIN_BLOCK
    what = encode_items(torch_mod, codec, oracle, items, "encode_batch, items below 32 768 bytes")
    if what:
        pytest.fail(what)


def test_items_of_a_batch_whose_longest_takes_them_to_the_lane_counters(torch_mod, codec, oracle, table):
    what = encode_items(torch_mod, codec, oracle, lanes_batch_items(table), "encode_batch, longest item from 32 768 bytes")
    if what:
        pytest.fail(what)


ROW_CASES = ("f32767_skewed_shuffled", "f13009_flat_runs16", "l60001_skewed_wave_steps")     # skewed, runs16, the full8 window


def test_a_case_written_over_a_block_of_a_stream(torch_mod, codec, oracle, table):
    """update_ranges (hist_tree_pairs_kernel, hist_lanes_pairs_kernel): the last block of a small stream replaced by a
    case's block, the new bytes at an unaligned source offset, is what encoding the new data from scratch gives"""
    from libhuffman_amd import datagen
    torch = torch_mod
    by = {c.name: (c, d) for c, d in table}
    for name in ROW_CASES:
        case, data = by[name]
        bs = case.bs
        for b in (0, 3):                                    # two of the case's blocks (laid out for other alignments: all the same here)
            blk = data[b * bs:(b + 1) * bs]
            old = np.concatenate([datagen.zipf255(2 * bs, seed=5), datagen.uniform256(bs, seed=6)])
            stream, offs, length = codec.encode(torch.from_numpy(old).cuda(), bs)
            src = on_device(torch, np.concatenate([np.zeros(3, np.uint8), blk]), 0)
            st, ln, new_offs, _, count = codec.update_ranges(stream, length, offs, 3, [(2 * bs, 3 * bs)], src, src_offsets=[3],
                                                             blocksize=bs, relaxed=True)
            assert count == 1, name
            new = np.concatenate([old[:2 * bs], blk])
            want, want_offs = oracle.encode(new, bs, with_offsets=True)
            got = st.cpu().numpy()
            if not (got.size == want.size and np.array_equal(got, want)):
                pytest.fail(explain(name, "update_ranges", got, want, want_offs))
            assert np.array_equal(new_offs.cpu().numpy().astype(np.uint64), want_offs), (name, "block index")
            out = torch.empty(new.size, dtype=torch.uint8, device="cuda")
            assert codec.decode(st, ln, new_offs, 3, out, relaxed=True) == new.size, name
            assert np.array_equal(out.cpu().numpy(), new), name


def test_a_case_appended_to_a_stream(torch_mod, codec, oracle, table):
    """hufgpu_append with the new bytes 3 bytes behind an aligned address: the tail block and the new blocks are counted
    by the row kernels"""
    import test_gpu_append as A
    by = {c.name: (c, d) for c, d in table}
    for name in ("f32767_skewed_shuffled", "l60001_skewed_wave_steps"):
        case, data = by[name]
        bs = case.bs
        data = data[:4 * bs + 21]
        raw = bs + 1000
        buf = A.Buf(torch_mod, codec, data[:raw], bs, entries=A.nblocks(data.size, bs) + 1, room=A.bound(data.size - bs, bs))
        r = A.append(torch_mod, codec, buf, data[raw:], src_off=3, relaxed=True)
        A.check_equals_encode(torch_mod, codec, oracle, data, bs, r, (name, "append"))


def run_child(mode, lib=None):
    env = dict(os.environ)
    env.pop("HUF_GPU_FUSED_HIST", None)
    env.pop("HUF_LIB_PATH", None)
    if mode == "fused":
        env["HUF_GPU_FUSED_HIST"] = "1"
    if lib:
        env["HUF_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "count_cases_fused_child.py"), mode], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("done"), r.stdout[-3000:] + r.stderr[-3000:]
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    wrong = [x["what"] for x in rows if not x["equal"]]
    assert not wrong, "\n".join(wrong)
    return [x["case"] for x in rows]


def test_the_fused_kernels_above_32_kib(torch_mod):
    """HUF_GPU_FUSED_HIST=1: hist_tree_kernel<.., true> at 65 537 and 131 072 bytes - once with wave 0's share one value,
    32 768 on one fold target - and hist_tree_kernel<.., false> at 131 073 and 200 001"""
    ran = run_child("fused")
    want = [c.name for c in count_cases.cases() if c.group in ("env", "fused")]
    assert ran == want and sum(n.startswith("e") for n in ran) >= 6


@pytest.mark.parametrize("variant,flags,mode", [("hl_ahead4", "-DHL_AHEAD=4", "lanes"), ("htp_arrays4", "-DHTP_ARRAYS=4", "fused")])
def test_other_values_of_the_tunables_count_exactly(torch_mod, variant, flags, mode):
    """HL_AHEAD = 4 moves the window of the vectors ahead to nvec 1 537 .. 2 047 (the 32 767-byte items of the batch);
    HTP_ARRAYS = 4 gives the packed body four arrays per wave"""
    from test_gpu_pack_builds import build_variant
    ran = run_child(mode, build_variant(variant, flags))
    assert len(ran) >= 8

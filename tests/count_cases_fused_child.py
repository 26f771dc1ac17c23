"""The cases of tests/count_cases.py through the encoder, shared by test_gpu_count_cases.py and - run as a program - its
child process.  HUF_GPU_FUSED_HIST is read once per process, and a build variant is a library of its own (HUF_LIB_PATH),
so both need a fresh process:

    count_cases_fused_child.py fused    the groups "env" and "fused" (the parent sets HUF_GPU_FUSED_HIST=1: hist_tree_kernel
                                        packed up to 128 KiB, with 32-bit counters beyond)
    count_cases_fused_child.py lanes    the group "lanes" and the batch whose longest item takes every item to
                                        hist_lanes_batch_kernel

It prints one JSON line per case, {"case", "equal", "what"}, and "done"."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import count_cases  # noqa: E402


def block_tree(block: np.ndarray):
    """(tree_len, entries) from a block's header"""
    tl = int(np.frombuffer(block[8:10].tobytes(), dtype="<i2")[0])
    return tl, np.frombuffer(block[10:10 + 2 * max(tl, 0)].tobytes(), dtype="<i2").tolist()


def explain(name, route, got: np.ndarray, want: np.ndarray, want_offs) -> str:
    """a mismatch as test_gpu_tree_cases.explain says it, for the first block that differs: both tree lengths and the
    first differing tree entry in front of the first differing byte"""
    m = min(got.size, want.size)
    d = np.flatnonzero(got[:m] != want[:m])
    at = int(d[0]) if d.size else m
    offs = np.asarray(want_offs, dtype=np.int64)
    b = max(0, min(int(np.searchsorted(offs, at, side="right")) - 1, offs.size - 2))
    g, w = got[int(offs[b]):], want[int(offs[b]):int(offs[b + 1])]
    msg = f"{name} on {route}: block {b} of {offs.size - 1}"
    if g.size < 10 or w.size < 10:
        return msg + f"; streams of {got.size} / {want.size} bytes"
    gl, gt = block_tree(g)
    wl, wt = block_tree(w)
    msg += f": tree_len {gl} (ours) / {wl} (oracle)"
    e = next((i for i in range(min(len(gt), len(wt))) if gt[i] != wt[i]), None)
    if e is not None:
        msg += f"; first differing tree entry {e}: {gt[e]} (ours) / {wt[e]} (oracle) - a miscount reads like this"
    return msg + f"; first differing byte {at} of {got.size} / {want.size}"


def on_device(torch, data: np.ndarray, offset: int):
    """the bytes on the device, `offset` bytes behind an aligned address"""
    buf = torch.empty(data.size + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + data.size]
    d.copy_(torch.from_numpy(data))
    return d


def encode_case(torch, codec, oracle, case, data, route):
    """None, or what differs: the stream and block index against the oracle's, then the indexed decode"""
    d = on_device(torch, data, case.offset)
    stream, offs, length = codec.encode(d, case.bs)
    want, want_offs = oracle.encode(data, case.bs, with_offsets=True)
    got = stream.cpu().numpy()
    if not (got.size == want.size and np.array_equal(got, want)):
        return explain(case.name, route, got, want, want_offs)
    if not np.array_equal(offs.cpu().numpy().astype(np.uint64), np.asarray(want_offs, dtype=np.uint64)):
        return f"{case.name} on {route}: block index"
    out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    nb = codec.block_count(data.size, case.bs)
    if codec.decode(stream, length, offs, nb, out, relaxed=True) != data.size or not torch.equal(out, d):
        return f"{case.name} on {route}: round trip"
    return None


def encode_items(torch, codec, oracle, items, route):
    """encode_batch with blocksize 0 of [(name, bytes)]: every item's record is the oracle's encode of the item alone, the
    item offsets add up, decode_batch gives the items back"""
    cat = np.concatenate([d for _, d in items])
    batch = codec.encode_batch(torch.from_numpy(cat).cuda(), [d.size for _, d in items], 0)
    st = batch.stream.cpu().numpy()
    offs = batch.offsets.cpu().numpy().astype(np.int64)
    pos = 0
    for i, (name, d) in enumerate(items):
        want = oracle.encode(d, 0)
        got = st[int(offs[i]):int(offs[i + 1])]
        if not (got.size == want.size and np.array_equal(got, want)):
            return explain(name, route, got, want, [0, want.size])
        if not int(offs[i]) == pos == batch.item_offsets[i]:
            return f"{name} on {route}: block index"
        pos += want.size
    if batch.stream_len != pos:
        return f"{route}: stream length"
    out, errs, raws = codec.decode_batch(batch, relaxed=True)
    if any(errs) or raws != [d.size for _, d in items] or not np.array_equal(out.cpu().numpy()[:cat.size], cat):
        return f"{route}: round trip"
    return None


def case_blocks(case, data):
    return [(f"{case.name}[{b}]", blk) for b, (blk, _, _, _) in enumerate(case.block_list(data))]


def lanes_batch_items(table):
    """items whose longest has 32 768 bytes or more - all of them then go through hist_lanes_batch_kernel: blocks of the
    lane-private cases, blocks of the fused ones (nvec = 2 047 lies in the window of a build with four vectors ahead) and
    items of 1, 15 and 21 bytes"""
    by = {c.name: (c, d) for c, d in table}
    items = []
    for name in ("l60001_skewed_runs16", "l32769_flat_shuffled", "f32767_skewed_wave_steps", "f13009_flat_runs16"):
        items += case_blocks(*by[name])
    one = by["f4097_flat_shuffled"][1]
    items[5:5] = [("one_byte", one[:1]), ("fifteen_bytes", one[100:115])]
    assert max(d.size for _, d in items) >= count_cases.HL_MIN_BLOCK and {1, 15, 21} <= {d.size for _, d in items}
    return items


def main(mode):
    import torch
    from libhuffman_amd.codec import GpuCodec
    from oracle.oracle import Oracle
    fused_env = bool(int(os.environ.get("HUF_GPU_FUSED_HIST", "0") or 0))
    assert (mode == "fused") == fused_env, "the parent sets HUF_GPU_FUSED_HIST=1 for `fused` and only for it"
    codec, oracle = GpuCodec(0), Oracle()
    groups = ("env", "fused") if mode == "fused" else ("lanes",)
    table = [(c, c.data()) for c in count_cases.cases()]
    for c, d in table:
        if c.group in groups:
            what = encode_case(torch, codec, oracle, c, d, "HUF_GPU_FUSED_HIST=1" if fused_env else "the default routes")
            print(json.dumps({"case": c.name, "equal": what is None, "what": what}), flush=True)
    if mode == "lanes":
        what = encode_items(torch, codec, oracle, lanes_batch_items(table), "encode_batch, longest item from 32 768 bytes")
        print(json.dumps({"case": "lanes_batch", "equal": what is None, "what": what}), flush=True)
    codec.close()
    print("done")


if __name__ == "__main__":
    main(sys.argv[1])

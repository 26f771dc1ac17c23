"""Batch calls against a loop of single calls (GPU): many small inputs, one context, device-resident data.

    python tools/time_batch.py [--runs 5] [--out profiles/batch/time_batch.txt]

Cases: (items x size) = 4096 x 4 KiB, 1024 x 64 KiB, 65536 x 256 B, on zipf255 bytes and log text, with and without the
sub-index, blocksize 128 KiB (every item one block).  A batch round = encode_batch (synchronised: the item offsets come
back) + decode_batch; a loop round = hufgpu_encode (synchronised for its length) + hufgpu_decode (synchronised) per
item.  The loop over 65 536 items is timed over its first 4 096 items and scaled.  Every figure is the median of
--runs warm runs, with min and max; every round trip is checked.  Last: equal items of exactly the blocksize against
ONE hufgpu_encode / hufgpu_decode_sub of the same bytes (16 MiB in 64 KiB blocks).
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd import datagen  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402

BS = 131072
LOOP_CAP = 4096


def stats(ts):
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def timed(fn, runs):
    fn()                                    # warm-up (workspace, staging)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def batch_round(codec, data, lens, sub, out):
    b = codec.encode_batch(data, lens, BS, sub_index=sub)
    _, errs, raws = codec.decode_batch(b, out=out)
    return b, errs, raws


def loop_round(codec, data, lens, k, outs):
    lib, ctx = codec.lib, codec._ctx
    stream, offs, back = outs
    pos = 0
    length, raw = C.c_uint64(0), C.c_uint64(0)
    for i in range(k):
        n = lens[i]
        err = lib.hufgpu_encode(ctx, data.data_ptr() + pos, n, BS, stream.data_ptr(), stream.numel(), offs.data_ptr(),
                                C.byref(length), None)
        assert err == 0
        err = lib.hufgpu_decode(ctx, stream.data_ptr(), length.value, offs.data_ptr(), codec.block_count(n, BS),
                                back.data_ptr() + pos, n, 0, C.byref(raw), None)
        assert err == 0 and raw.value == n
        pos += n


def case(codec, kind, nitems, size, runs, lines):
    gen = datagen.zipf255 if kind == "zipf" else datagen.logtext
    host = gen(nitems * size)
    data = torch.from_numpy(host).cuda()
    lens = [size] * nitems
    out = torch.empty(nitems * size, dtype=torch.uint8, device="cuda")
    res = {}
    for sub in (False, True):
        b, errs, raws = batch_round(codec, data, lens, sub, out)
        assert errs == [0] * nitems and raws == lens and torch.equal(out, data), "batch round trip"
        res[sub] = stats(timed(lambda: batch_round(codec, data, lens, sub, out), runs))
    k = min(nitems, LOOP_CAP)
    outs = (torch.empty(codec.encode_bound(size, BS), dtype=torch.uint8, device="cuda"),
            torch.empty(2, dtype=torch.int64, device="cuda"), torch.zeros(nitems * size, dtype=torch.uint8, device="cuda"))
    loop_round(codec, data, lens, k, outs)
    assert torch.equal(outs[2][: k * size], data[: k * size]), "loop round trip"
    lt = [t * nitems / k for t in timed(lambda: loop_round(codec, data, lens, k, outs), runs)]
    loop = stats(lt)
    for sub in (False, True):
        med, lo, hi = res[sub]
        lines.append(f"{nitems:6d} x {size:6d} B {kind:5s} sub={int(sub)}  batch {med:9.3f} ms [{lo:.3f}, {hi:.3f}]   "
                     f"loop {loop[0]:10.2f} ms [{loop[1]:.2f}, {loop[2]:.2f}]{' (scaled from %d items)' % k if k < nitems else ''}"
                     f"   speed-up {loop[0] / med:7.1f}x")
        print(lines[-1], flush=True)


def equal_items(codec, runs, lines):
    bs, nitems = 65536, 256
    host = datagen.zipf255(bs * nitems)
    data = torch.from_numpy(host).cuda()
    n = data.numel()
    lens = [bs] * nitems
    nb, rbs, bound, subb = codec.batch_geometry(lens, bs)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    offs = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    sub = torch.empty((subb + 7) // 8, dtype=torch.int64, device="cuda")
    ls = (C.c_uint64 * nitems)(*lens)
    lib, ctx = codec.lib, codec._ctx

    def enc_batch():
        assert lib.hufgpu_encode_batch(ctx, data.data_ptr(), nitems, ls, bs, out.data_ptr(), bound, offs.data_ptr(),
                                       None, sub.data_ptr(), None, None) == 0

    def enc_single():
        assert lib.hufgpu_encode_sub(ctx, data.data_ptr(), n, bs, out.data_ptr(), bound, offs.data_ptr(), sub.data_ptr(),
                                     None, None) == 0
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    te_b = stats(timed(enc_batch, runs))
    enc_batch()
    torch.cuda.synchronize()
    stream_len = int(offs[-1].item())
    ib = (C.c_uint64 * (nitems + 1))(*range(nitems + 1))
    oo = (C.c_uint64 * (nitems + 1))(*[i * bs for i in range(nitems + 1)])
    errs, raws = (C.c_int32 * nitems)(), (C.c_uint64 * nitems)()

    def dec_batch():
        assert lib.hufgpu_decode_batch(ctx, out.data_ptr(), stream_len, offs.data_ptr(), nitems, ib, oo, sub.data_ptr(), bs,
                                       back.data_ptr(), 0, errs, raws, None) == 0
    td_b = stats(timed(dec_batch, runs))
    assert torch.equal(back, data)
    te_s = stats(timed(enc_single, runs))
    raw = C.c_uint64(0)

    def dec_single():
        assert lib.hufgpu_decode_sub(ctx, out.data_ptr(), stream_len, offs.data_ptr(), n, bs, sub.data_ptr(), back.data_ptr(),
                                     n, 0, C.byref(raw), None) == 0
    td_s = stats(timed(dec_single, runs))
    for what, b, s in (("encode", te_b, te_s), ("decode", td_b, td_s)):
        lines.append(f"{nitems} x 64 KiB zipf, blocksize 64 KiB, sub-index: {what} batch {b[0]:.3f} ms [{b[1]:.3f}, {b[2]:.3f}]"
                     f"  single {s[0]:.3f} ms [{s[1]:.3f}, {s[2]:.3f}]  batch/single {b[0] / s[0]:.3f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    codec = GpuCodec(0)
    lines = [f"time_batch.py: {torch.cuda.get_device_name(0)}, blocksize {BS}, median of {a.runs} warm runs [min, max]; "
             "batch = encode_batch + decode_batch, loop = hufgpu_encode + hufgpu_decode per item"]
    print(lines[0], flush=True)
    for nitems, size in ((4096, 4096), (1024, 65536), (65536, 256)):
        for kind in ("zipf", "log"):
            case(codec, kind, nitems, size, a.runs, lines)
    equal_items(codec, a.runs, lines)
    codec.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

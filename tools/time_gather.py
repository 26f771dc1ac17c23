"""hufgpu_gather against what a caller with positions on the GPU had to do before it (GPU).

    python tools/time_gather.py [--runs 7] [--mib 1024] [--out profiles/ranges/time_gather.txt]

1 GiB of zipf255 bytes, device-resident, the record positions in a CUDA tensor.  The yardstick is
hufgpu_decode_ranges(..., HUFGPU_RANGES_TILES) on the same records with everything a caller needs to get there: the
synchronisation, the copy of the positions to the host, the host arrays, the call with its two waits.  The gather is
timed from its enqueue to one synchronize.  The two alternate in one process; every figure is the median of --runs warm
runs with [min, max], and both outputs are compared with slices of the input.

Every shape runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd.codec import GpuCodec  # noqa: E402

TILES = 4               # HUFGPU_RANGES_TILES
SHAPES = [("4 096 x 64 B, blocks of 64 KiB", 4096, 64, 65536, None),
          ("4 096 x 4 KiB, blocks of 64 KiB", 4096, 4096, 65536, None),
          ("4 096 x 64 B inside 16 MiB, blocks of 64 KiB", 4096, 64, 65536, 16 << 20),
          ("64 x 4 KiB, ONE block", 64, 4096, 0, None)]
STEP_SECONDS = 300


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:9.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


def one_shape(k, runs, mib):
    what, r, size, bs, span = SHAPES[k]
    codec = GpuCodec(0)
    n = mib << 20
    data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), "zipf255")
    sub = codec.new_sub_index(n, bs)
    stream, offs, length = codec.encode(data, bs, sub_index=sub)
    nb = codec.block_count(n, bs)
    rng = np.random.default_rng(r * 17 + size)
    lo0 = n // 3 if span else 0
    base = torch.from_numpy(rng.integers(0, (span or n) - size - 1, r) | 1).cuda()
    out_r = torch.zeros(r * size, dtype=torch.uint8, device="cuda")
    out_g = torch.zeros((r, size), dtype=torch.uint8, device="cuda")
    lib, ctx = codec.lib, codec._ctx
    errs, raws = (C.c_int32 * r)(), (C.c_uint64 * r)()
    oo = (C.c_uint64 * (r + 1))(*[i * size for i in range(r + 1)])

    def yardstick():
        positions = base + lo0                          # (produced one kernel earlier)
        t0 = time.perf_counter()
        los = positions.tolist()                        # the wait and the copy to the host
        lo, hi = (C.c_uint64 * r)(*los), (C.c_uint64 * r)(*[x + size for x in los])
        rc = lib.hufgpu_decode_ranges(ctx, stream.data_ptr(), length, offs.data_ptr(), nb, r, lo, hi, oo, sub.data_ptr(), n, bs,
                                      out_r.data_ptr(), TILES, errs, raws, None)
        t1 = time.perf_counter()
        assert rc == 0
        return t1 - t0

    def gather():
        positions = base + lo0
        t0 = time.perf_counter()
        _, e, _ = codec.gather(stream, length, offs, nb, positions, size, sub_index=sub, raw_size=n, blocksize=bs, out=out_g)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return t1 - t0, e

    yardstick()
    _, e = gather()
    assert int(e.abs().max()) == 0
    for i in list(range(8)) + [r - 1]:
        p = int(base[i]) + lo0
        assert torch.equal(out_r[i * size:(i + 1) * size], data[p:p + size]) and torch.equal(out_g[i], data[p:p + size]), i
    assert torch.equal(out_g.view(-1), out_r)
    ty, tg = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        ty.append(yardstick())
        torch.cuda.synchronize()
        tg.append(gather()[0])
    verdict = "below" if statistics.median(tg) < min(ty) else "NOT below"
    print(f"{what:46s} decode_ranges(tiles) from device positions {fmt(ty)}   gather {fmt(tg)} = "
          f"{statistics.median(ty) / statistics.median(tg):6.2f}x   (the gather's median is {verdict} the yardstick's minimum)", flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--shape", type=int, default=-1, help="run this shape only, in this process")
    a = ap.parse_args()
    if a.shape >= 0:
        one_shape(a.shape, a.runs, a.mib)
        return
    lines = [f"time_gather.py: {a.mib} MiB of zipf255, median of {a.runs} warm runs [min, max], the two calls alternating in one process per shape"]
    print(lines[0], flush=True)
    for k in range(len(SHAPES)):
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--shape", str(k),
                            "--runs", str(a.runs), "--mib", str(a.mib)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"shape {k} ended with status {p.returncode}: nothing further is run")
            print(lines[-1], flush=True)
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if len(lines) == 1 + len(SHAPES) else 1)


if __name__ == "__main__":
    main()

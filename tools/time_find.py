"""hufgpu_find_bytes against what a caller who wants the positions of byte values had to do before it (GPU).

    python tools/time_find.py [--runs 7] [--mib 1024] [--out profiles/find/time_find.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  Three sets each: {10} (the
newline; a frequent value of zipf255), one rare value, and 128 values; max_positions = 2^20.  find_bytes is timed from
its enqueue to one synchronize.  The yardstick is what a caller does today: decode with the sub-index into an N-byte
tensor, torch.nonzero over it (out == v; a 256-entry table look-up for the 128 values) and the wait for the result's size.
The two alternate in one process; every figure is the median of --runs warm runs with [min, max].  The indexed decode alone
(enqueue to synchronize, no nonzero) is timed in the same loop: find_sub_kernel reads the same bytes and writes an eighth.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd import datagen  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402

WORKLOADS = [("logtext, blocks of 1 MiB", "logtext", 1 << 20), ("zipf255, blocks of 64 KiB", "zipf255", 65536)]
CAP = 1 << 20
STEP_SECONDS = 420


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:9.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


def one_workload(k, runs, mib):
    what, kind, bs = WORKLOADS[k]
    codec = GpuCodec(0)
    n = mib << 20
    if kind == "logtext":
        tile = min(n, 16 << 20)
        data = torch.from_numpy(datagen.logtext(tile)).cuda().repeat(n // tile)
    else:
        data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), kind)
    sub = codec.new_sub_index(n, bs)
    stream, offs, length = codec.encode(data, bs, sub_index=sub)
    nb = codec.block_count(n, bs)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    hist = torch.bincount(data[:1 << 24].int(), minlength=256).cpu().numpy()
    present = np.flatnonzero(hist)
    rare = int(present[hist[present].argmin()])
    half = [int(v) for v in np.random.default_rng(7).permutation(256)[:128]]
    sets = [("{10}", [10]), (f"rare {{{rare}}}", [rare]), ("128 values", half)]
    pos = torch.empty(CAP, dtype=torch.int64, device="cuda")

    def decode_alone():
        t0 = time.perf_counter()
        codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codec.decode_result()
        return t1 - t0

    for name, values in sets:
        lut = torch.zeros(256, dtype=torch.bool, device="cuda")
        lut[torch.tensor(values, device="cuda")] = True

        def yardstick():
            t0 = time.perf_counter()
            codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
            p = torch.nonzero(out == values[0] if len(values) == 1 else lut[out.int()]).view(-1)   # (waits for the size)
            t1 = time.perf_counter()
            codec.decode_result()
            return t1 - t0, p

        def find():
            t0 = time.perf_counter()
            _, totals, errs, _ = codec.find_bytes(stream, length, offs, nb, sub, n, bs, values, max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            return t1 - t0, totals, errs

        _, p = yardstick()
        _, totals, errs = find()
        t = totals.cpu().tolist()
        assert t == [p.numel(), min(p.numel(), CAP), 0, 0] and int(errs.abs().max()) == 0, t
        assert torch.equal(pos[:t[1]], p[:t[1]])
        del p
        ty, tf, td = [], [], []
        for _ in range(runs):
            torch.cuda.synchronize()
            ty.append(yardstick()[0])
            torch.cuda.synchronize()
            tf.append(find()[0])
            torch.cuda.synchronize()
            td.append(decode_alone())
        print(f"{what:28s} {name:12s} {t[0]:11d} matches   decode + nonzero {fmt(ty)}   find_bytes {fmt(tf)} = "
              f"{statistics.median(ty) / statistics.median(tf):5.2f}x   decode alone {fmt(td)} = "
              f"{statistics.median(td) / statistics.median(tf):5.2f}x of find_bytes", flush=True)
    codec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", type=int, default=-1, help="run this workload only, in this process")
    a = ap.parse_args()
    if a.workload >= 0:
        one_workload(a.workload, a.runs, a.mib)
        return
    lines = [f"time_find.py: {a.mib} MiB, max_positions 2^20, median of {a.runs} warm runs [min, max], the calls alternating in one process per workload"]
    print(lines[0], flush=True)
    ok = True
    for k in range(len(WORKLOADS)):
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--workload", str(k),
                            "--runs", str(a.runs), "--mib", str(a.mib)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"workload {k} ended with status {p.returncode}: nothing further is run")
            print(lines[-1], flush=True)
            ok = False
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

"""hufgpu_find_pattern against what a caller who greps a compressed stream had to do before it (GPU).

    python tools/time_find_pattern.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_pattern.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  Three patterns each: a
frequent one of 5 bytes (the word ERROR; five times zipf255's most frequent value - a pattern whose every prefix is
frequent, the matcher's expensive kind), a string of 36 bytes that was planted at five places, four of them across block
seams, and one that does not occur but shares four bytes with the frequent one; max_positions = 2^20.  find_pattern is
timed from its enqueue to one synchronize.  Against it, alternating in one process, median of --runs warm runs with
[min, max]:
  (i)   what a caller does today: decode with the sub-index into an N-byte tensor, torch.nonzero of the first byte (a
        wait for the size), the candidates' bytes gathered and compared, torch.nonzero of the verdicts (a second wait);
  (ii)  that decode alone, enqueue to synchronize;
  (iii) find_bytes for the pattern's first byte: the same walk of the stream without the matcher and the seam launch.

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
SLICE = 1 << 24          # candidates compared at a time by the yardstick


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:9.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


def one_workload(k, runs, mib):
    what, kind, bs = WORKLOADS[k]
    codec = GpuCodec(0)
    n = mib << 20
    if kind == "logtext":
        tile = min(n, 16 << 20)
        data = torch.from_numpy(datagen.logtext(tile)).cuda().repeat(n // tile)
        frequent = b"ERROR"
    else:
        data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), kind)
        top = int(torch.bincount(data[:1 << 24].int(), minlength=256).argmax())
        frequent = bytes([top]) * 5
    planted = bytes(np.random.default_rng(36).integers(128, 255, 36).astype(np.uint8))
    places = [n // 2 + 12345] + [(j * (n // bs // 5) + 1) * bs - d for j, d in zip(range(1, 5), (1, 18, 35, 7))]
    for p in places:
        data[p:p + 36] = torch.frombuffer(bytearray(planted), dtype=torch.uint8).cuda()
    absent = frequent[:4] + (b"\xff" if kind == "zipf255" else b"\x00")
    sub = codec.new_sub_index(n, bs)
    stream, offs, length = codec.encode(data, bs, sub_index=sub)
    nb = codec.block_count(n, bs)
    del data
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    pos = torch.empty(CAP, dtype=torch.int64, device="cuda")

    def decode_alone():
        t0 = time.perf_counter()
        codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codec.decode_result()
        return t1 - t0

    for name, pat in (("frequent, 5 bytes", frequent), ("planted, 36 bytes", planted), ("absent, 5 bytes", absent)):
        m = len(pat)
        pat_t = torch.frombuffer(bytearray(pat), dtype=torch.uint8).cuda()
        span = torch.arange(m, device="cuda")

        def yardstick():
            t0 = time.perf_counter()
            codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
            cand = torch.nonzero(out[:n - m + 1] == pat[0]).view(-1)                    # (waits for the size)
            keep = [c[(out[c[:, None] + span] == pat_t).all(1)] for c in cand.split(SLICE)]   # (waits for each size)
            p = torch.cat(keep) if keep else cand
            t1 = time.perf_counter()
            codec.decode_result()
            return t1 - t0, p

        def find():
            t0 = time.perf_counter()
            _, totals, errs, _ = codec.find_pattern(stream, length, offs, nb, sub, n, bs, pat, max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            return t1 - t0, totals, errs

        def first_byte():
            t0 = time.perf_counter()
            codec.find_bytes(stream, length, offs, nb, sub, n, bs, pat[:1], max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        _, p = yardstick()
        _, totals, errs = find()
        t = totals.cpu().tolist()
        assert t == [p.numel(), min(p.numel(), CAP), 0, 0] and int(errs.abs().max()) == 0, (t, p.numel())
        assert torch.equal(pos[:t[1]], p[:t[1]])
        if pat is planted:
            assert p.cpu().tolist() == sorted(places)
        del p
        ty, tf, td, tb = [], [], [], []
        for _ in range(runs):
            torch.cuda.synchronize()
            ty.append(yardstick()[0])
            torch.cuda.synchronize()
            tf.append(find()[0])
            torch.cuda.synchronize()
            td.append(decode_alone())
            torch.cuda.synchronize()
            tb.append(first_byte())
        mf = statistics.median(tf)
        print(f"{what:28s} {name:18s} {t[0]:10d} matches   decode + torch search {fmt(ty)}   find_pattern {fmt(tf)} = "
              f"{statistics.median(ty) / mf:5.2f}x   decode alone {fmt(td)} = {statistics.median(td) / mf:5.2f}x   "
              f"find_bytes(first byte) {fmt(tb)} = {statistics.median(tb) / mf:5.2f}x of find_pattern", flush=True)
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
    lines = [f"time_find_pattern.py: {a.mib} MiB, max_positions 2^20, median of {a.runs} warm runs [min, max], the calls "
             "alternating in one process per workload"]
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

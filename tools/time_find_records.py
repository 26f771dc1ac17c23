"""hufgpu_find_records against the two-walk recipe it replaces (GPU).

    python tools/time_find_records.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_records.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the delimiter is the newline.
Three patterns each: a frequent one of 5 bytes (the word ERROR; five times zipf255's most frequent value), a string of 36
bytes that was planted at five places, four of them across block seams, and one that does not occur but shares four bytes
with the frequent one.  The caps are the exact counts, taken by count_bytes / count_pattern before anything is timed.
Alternating in one process, median of --runs warm runs with [min, max], each from its first enqueue to one synchronize:
  (i)   find_records: one walk, the records' starts and lengths;
  (ii)  the recipe: find_bytes(newline) + find_pattern + torch.where x 3 + torch.searchsorted, up to the `starts` tensor
        (one start per MATCH, duplicates included, and no lengths);
  (iii) find_pattern alone: what (i) costs beyond it is the second mask and the record kernels.
The tool asserts that the records of (i) are the deduplicated starts of (ii), with the lengths the recipe's newlines give,
and that (i) takes no longer than (ii) on any row.

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
STEP_SECONDS = 420


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


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
        hist = torch.bincount(data[:1 << 24].int(), minlength=256)
        hist[10] = 0                                    # (a pattern holds no delimiter)
        frequent = bytes([int(hist.argmax())]) * 5
    planted = bytes(np.random.default_rng(36).integers(128, 255, 36).astype(np.uint8))
    places = [n // 2 + 12345] + [(j * (n // bs // 5) + 1) * bs - d for j, d in zip(range(1, 5), (1, 18, 35, 7))]
    for p in places:
        data[p:p + 36] = torch.frombuffer(bytearray(planted), dtype=torch.uint8).cuda()
    absent = frequent[:4] + (b"\xff" if kind == "zipf255" else b"\x00")
    sub = codec.new_sub_index(n, bs)
    stream, offs, length = codec.encode(data, bs, sub_index=sub)
    nb = codec.block_count(n, bs)
    del data
    args = (stream, length, offs, nb, sub, n, bs)
    nl_cap = int(codec.count_bytes(*args, b"\n")[0][0]) + 1
    nl_pos = torch.empty(nl_cap, dtype=torch.int64, device="cuda")
    nl_slots = torch.arange(nl_cap, device="cuda")

    for name, pat in (("frequent, 5 bytes", frequent), ("planted, 36 bytes", planted), ("absent, 5 bytes", absent)):
        cap = int(codec.count_pattern(*args, pat)[0][0]) + 1
        hit_pos = torch.empty(cap, dtype=torch.int64, device="cuda")
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))
        slots = torch.arange(cap, device="cuda")

        def records():
            t0 = time.perf_counter()
            pos, lens, totals, errs, _ = codec.find_records(*args, pat, b"\n", max_records=cap, out=out)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, pos, lens, totals, errs

        def recipe():
            t0 = time.perf_counter()
            nl, nl_totals, _, _ = codec.find_bytes(*args, b"\n", max_positions=nl_cap, out=nl_pos)
            hit, hit_totals, _, _ = codec.find_pattern(*args, pat, max_positions=cap, out=hit_pos)
            nl = torch.where(nl_slots < nl_totals[1], nl, n)
            hit = torch.where(slots < hit_totals[1], hit, n)
            k = torch.searchsorted(nl, hit)
            starts = torch.where(k > 0, nl[(k - 1).clamp(min=0)] + 1, 0)
            starts = torch.where(hit < n, starts, n)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, starts, nl, k, hit_totals

        def pattern_alone():
            t0 = time.perf_counter()
            codec.find_pattern(*args, pat, max_positions=cap, out=hit_pos)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        _, starts, nl, k, hit_totals = recipe()
        _, pos, lens, totals, errs = records()
        t = totals.cpu().tolist()
        matches = int(hit_totals[0])
        assert matches == cap - 1 and int(errs.abs().max()) == 0 and t[2:] == [0, 0], (t, matches, cap)
        first = torch.ones(matches, dtype=torch.bool, device="cuda")
        first[1:] = starts[1:matches] != starts[:matches - 1]
        want = starts[:matches][first]                                      # the deduplicated starts of the recipe
        ends = torch.cat([nl, nl.new_tensor([n])])[k[:matches][first]]      # the next newline, or the end of the data
        assert t[0] == t[1] == want.numel(), (t, want.numel())
        assert torch.equal(pos[:t[1]], want) and torch.equal(lens[:t[1]].long(), ends - want)
        if pat is planted:
            assert matches == len(places) and t[0] == len(places)
        del starts, nl, k, want, ends, first
        tr, ty, tp = [], [], []
        for _ in range(runs):
            torch.cuda.synchronize()
            tr.append(records()[0])
            torch.cuda.synchronize()
            ty.append(recipe()[0])
            torch.cuda.synchronize()
            tp.append(pattern_alone())
        mr, my, mp = statistics.median(tr), statistics.median(ty), statistics.median(tp)
        print(f"{what:26s} {name:18s} {matches:9d} matches {t[0]:9d} records   (i) find_records {fmt(tr)}   (ii) recipe {fmt(ty)} = "
              f"{my / mr:5.2f}x   (iii) find_pattern {fmt(tp)}: (i) is {mr / mp:5.2f}x of it, + {(mr - mp) * 1e3:.3f} ms", flush=True)
        assert mr <= my, f"find_records ({mr * 1e3:.3f} ms) takes longer than the recipe ({my * 1e3:.3f} ms)"
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
    lines = [f"time_find_records.py: {a.mib} MiB, delimiter newline, caps = the exact counts, median of {a.runs} warm runs "
             "[min, max], the calls alternating in one process per workload"]
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

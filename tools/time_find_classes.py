"""hufgpu_find_classes against the literal hufgpu_find_pattern, and against the 32 literal calls that a case-insensitive
search for a five-letter word took before it (GPU).

    python tools/time_find_classes.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_classes.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  The caps are the exact
counts, taken by count_pattern before anything is timed.  Alternating in one process, median of --runs warm runs with
[min, max], each from its first enqueue to one synchronize.

  log text   literal        find_pattern(b"ERROR"): the yardstick, the literal kernels
             one value      the same string as five classes of one value each
             ignore case    find_pattern(b"error", ignore_case=True)
             hex key        a planted key of 36 bytes, "req-" + eight classes of the hex digits + 24 bytes
             first full     the full class in front of b"RROR": every start a candidate
             32 literals    find_pattern for each of the 32 spellings of "error" (without the caller's merge of their
                            positions, which the class call does not need)
  zipf255    literal        five times the most frequent value
             one value      the same as classes
             wide           five classes of the 128 values 64 .. 191

The tool asserts that a literal and its classes of one value give the same totals and positions, that the 32 literal
calls find together what the one class call finds, and that the one class call takes less time than the 32.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import argparse
import itertools
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
HEX = b"0123456789abcdef"


def fmt(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


def one_workload(k, runs, mib):
    what, kind, bs = WORKLOADS[k]
    codec = GpuCodec(0)
    n = mib << 20
    rows = []                                               # (name, the patterns of one timing, ignore_case)
    if kind == "logtext":
        tile = min(n, 16 << 20)
        data = torch.from_numpy(datagen.logtext(tile)).cuda().repeat(n // tile)
        key = b"req-1a2b3c4d-" + bytes(np.random.default_rng(36).integers(128, 255, 23).astype(np.uint8))
        assert len(key) == 36
        places = [n // 2 + 12345] + [(j * (n // bs // 5) + 1) * bs - d for j, d in zip(range(1, 5), (1, 18, 35, 7))]
        rng = np.random.default_rng(37)
        for p in places:                                    # another eight hex digits at every place
            one = key[:4] + bytes(HEX[int(v)] for v in rng.integers(0, 16, 8)) + key[12:]
            data[p:p + 36] = torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda()
        spellings = [bytes(c) for c in itertools.product(*[(x, x ^ 0x20) for x in b"error"])]
        assert len(set(spellings)) == 32
        rows = [("literal ERROR", [b"ERROR"], False), ("one value ERROR", [[bytes([c]) for c in b"ERROR"]], False),
                ("ignore case error", [b"error"], True),
                ("hex key, 36 bytes", [[bytes([c]) for c in key[:4]] + [HEX] * 8 + [bytes([c]) for c in key[12:]]], False),
                ("first full .RROR", [[GpuCodec.ANY] + [bytes([c]) for c in b"RROR"]], False),
                ("32 literals of error", spellings, False)]
    else:
        data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), kind)
        hist = torch.bincount(data[:1 << 24].int(), minlength=256)
        frequent = bytes([int(hist.argmax())]) * 5
        rows = [("literal, 5 bytes", [frequent], False), ("one value, 5 bytes", [[bytes([c]) for c in frequent]], False),
                ("wide, 5 x [64..191]", [[bytes(range(64, 192))] * 5], False)]
    sub = codec.new_sub_index(n, bs)
    stream, offs, length = codec.encode(data, bs, sub_index=sub)
    nb = codec.block_count(n, bs)
    del data
    args = (stream, length, offs, nb, sub, n, bs)

    jobs = []
    for name, pats, ic in rows:
        caps = [int(codec.count_pattern(*args, p, ignore_case=ic)[0][0]) + 1 for p in pats]
        outs = [torch.empty(c, dtype=torch.int64, device="cuda") for c in caps]
        jobs.append((name, pats, ic, caps, outs))

    def timed(job):
        _, pats, ic, caps, outs = job
        t0 = time.perf_counter()
        res = [codec.find_pattern(*args, p, max_positions=c, out=o, ignore_case=ic) for p, c, o in zip(pats, caps, outs)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    answers = {}
    for job in jobs:                                        # warm, and the answers
        _, res = timed(job)
        for (_, totals, errs, _), c in zip(res, job[3]):
            t = totals.cpu().tolist()
            assert t == [c - 1, c - 1, 0, 0] and int(errs.abs().max()) == 0, (job[0], t, c)
        answers[job[0]] = (sum(job[3]) - len(job[3]), [r[0][:c - 1].clone() for r, c in zip(res, job[3])])
    lit, one = answers[rows[0][0]], answers[rows[1][0]]
    assert lit[0] == one[0] and torch.equal(lit[1][0], one[1][0]), "classes of one value differ from the literal"
    if kind == "logtext":
        merged = torch.cat(answers["32 literals of error"][1]).sort().values
        assert torch.equal(merged, answers["ignore case error"][1][0]), "the 32 literal calls and the class call differ"
        assert answers["hex key, 36 bytes"][0] == 5
    del answers, lit, one

    times = {job[0]: [] for job in jobs}
    for _ in range(runs):
        for job in jobs:
            torch.cuda.synchronize()
            times[job[0]].append(timed(job)[0])
    base = statistics.median(times[rows[0][0]])
    for name, pats, ic, caps, outs in jobs:
        m = statistics.median(times[name])
        print(f"{what:26s} {name:22s} {len(pats):3d} call(s) {sum(caps) - len(caps):10d} matches   {fmt(times[name])}   "
              f"{m / base:5.2f}x of the literal", flush=True)
    if kind == "logtext":
        cls, many = statistics.median(times["ignore case error"]), statistics.median(times["32 literals of error"])
        print(f"{what:26s} one class call for `error` takes {cls * 1e3:.3f} ms, the 32 literal calls {many * 1e3:.3f} ms: {many / cls:.1f}x", flush=True)
        assert cls < many, f"the class call ({cls * 1e3:.3f} ms) takes no less than the 32 literal calls ({many * 1e3:.3f} ms)"
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
    lines = [f"time_find_classes.py: {a.mib} MiB, caps = the exact counts, median of {a.runs} warm runs [min, max], from the first "
             "enqueue to one synchronize, the rows alternating in one process per workload"]
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

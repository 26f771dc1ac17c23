"""hufgpu_find_any - ANY of several class patterns in one walk - against the K hufgpu_find_classes calls it replaces, and
against ONE class call of the longest alternative's length (GPU).

    python tools/time_find_any.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_any.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  The caps are the exact
counts, taken by count_pattern before anything is timed.  Alternating in one process, median of --runs warm runs with
[min, max], each from its first enqueue to one synchronize.  For K = 3 and K = 8 alternatives:

  any of K       find_pattern(AnyOf(...)): one call, one walk
  K class calls  find_pattern for each alternative as a class pattern (without the caller's merge and de-duplication of
                 their positions, which the one call does not need)
  longest alone  ONE class call for the longest alternative: the yardstick - the class kernels, unchanged in this build

  log text   K = 3: ERROR, WARN, retrying; K = 8: those and DEBUG, heartbeat, flushed, "cache miss", "status=5"
  zipf255    K strings of 3 to 8 of the four most frequent values

The tool asserts that the one call's total and positions are the sorted union, without duplicates, of the K class calls',
and that the one call takes less time than the K calls.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import numpy as np
import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

LOG_WORDS = [b"ERROR", b"WARN", b"retrying", b"DEBUG", b"heartbeat", b"flushed", b"cache miss", b"status=5"]
ZIPF_LENGTHS = [5, 3, 8, 4, 6, 7, 5, 4]
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, kind, codec = load.what, load.kind, load.codec
    if kind == "logtext":
        words = LOG_WORDS
    else:
        top = load.histogram().argsort(descending=True)[:4].tolist()
        rng = np.random.default_rng(38)
        words = [bytes([top[0]] * 5)]
        while len(words) < 8:
            w = bytes(top[int(v)] for v in rng.integers(0, 4, ZIPF_LENGTHS[len(words)]))
            if w not in words:
                words.append(w)
    assert sum(len(w) for w in words) <= 64
    args = load.encode()

    rows = []                                               # (name, K, the patterns of one timing)
    for K in (3, 8):
        alts = [[bytes([c]) for c in w] for w in words[:K]]
        rows += [(f"any of {K}", K, [GpuCodec.AnyOf(*alts)]), (f"{K} class calls", K, alts),
                 (f"longest of {K} alone", K, [max(alts, key=len)])]
    jobs = []
    for name, K, pats in rows:
        caps = [int(codec.count_pattern(*args, p)[0][0]) + 1 for p in pats]
        outs = [torch.empty(c, dtype=torch.int64, device="cuda") for c in caps]
        jobs.append((name, K, pats, caps, outs))

    def timed(job):
        _, _, pats, caps, outs = job
        t0 = time.perf_counter()
        res = [codec.find_pattern(*args, p, max_positions=c, out=o) for p, c, o in zip(pats, caps, outs)]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    answers = {}
    for job in jobs:                                        # warm, and the answers
        _, res = timed(job)
        for (_, totals, errs, _), c in zip(res, job[3]):
            t = totals.cpu().tolist()
            assert t == [c - 1, c - 1, 0, 0] and int(errs.abs().max()) == 0, (job[0], t, c)
        answers[job[0]] = [r[0][:c - 1].clone() for r, c in zip(res, job[3])]
    for K in (3, 8):
        union = torch.unique(torch.cat(answers[f"{K} class calls"]))     # (sorted, without duplicates)
        one = answers[f"any of {K}"][0]
        assert one.numel() == union.numel() and torch.equal(one, union), f"the one call and the union of the {K} class calls differ"
    del answers

    times = dict(zip([job[0] for job in jobs], alternate(runs, *[lambda job=job: timed(job)[0] for job in jobs])))
    for name, K, pats, caps, outs in jobs:
        m, base = statistics.median(times[name]), statistics.median(times[f"longest of {K} alone"])
        longest = max(len(w) for w in words[:K])
        print(f"{what:26s} {name:20s} {len(pats):2d} call(s) {sum(caps) - len(caps):10d} matches   {fmt(times[name])}   "
              f"{m / base:5.2f}x of one class call of {longest} positions", flush=True)
    for K in (3, 8):
        one, many = statistics.median(times[f"any of {K}"]), statistics.median(times[f"{K} class calls"])
        print(f"{what:26s} the one call for {K} alternatives takes {one * 1e3:.3f} ms, the {K} class calls {many * 1e3:.3f} ms: "
              f"{many / one:.2f}x", flush=True)
        assert one < many, f"the one call ({one * 1e3:.3f} ms) takes no less than the {K} class calls ({many * 1e3:.3f} ms)"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

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
import itertools
import statistics
import time

import numpy as np
import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

HEX = b"0123456789abcdef"
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, kind, codec, n, bs, data = w.what, w.kind, w.codec, w.n, w.bs, w.data
    rows = []                                               # (name, the patterns of one timing, ignore_case)
    if kind == "logtext":
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
        frequent = w.frequent()
        rows = [("literal, 5 bytes", [frequent], False), ("one value, 5 bytes", [[bytes([c]) for c in frequent]], False),
                ("wide, 5 x [64..191]", [[bytes(range(64, 192))] * 5], False)]
    del data
    args = w.encode()

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

    times = dict(zip([job[0] for job in jobs], alternate(runs, *[lambda job=job: timed(job)[0] for job in jobs])))
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


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_any_quant - patterns with optional and repeated positions, in one walk - against ONE any-of call of the same
longest length without optional positions, and against the any-of calls over the written-out forms that it replaces (GPU).

    python tools/time_find_quant.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_quant.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  The caps are the exact counts,
taken by count_pattern before anything is timed.  Alternating in one process, median of --runs warm runs with [min, max], each
from its first enqueue to one synchronize.  Three patterns a workload, three rows a pattern:

  (a) any-of   ONE find_pattern(AnyOf(longest form)): every position required - the older kernels, unchanged: what the closure
               over the optional positions costs a byte is (b) against this row
  (b) quant    find_pattern(the pattern with Opt / Rep): one call, one walk
  (c) forms    what a caller writes today: every form as an alternative of AnyOf - ONE call where the forms fit the 64
               positions, else K calls, the forms packed first-fit, and torch.unique over their position lists

  log text   'heartbeats? ok', 'lag=[0-9]{1,5} ms', '[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}' (81 forms of 7 to 15 bytes)
  zipf255    the same shapes over its most frequent values: a word of six with one optional letter, two values around one to
             five of four others, four groups of one to three of ten values with an eleventh between them

The tool asserts that (b) and (c) find the same starts, and that (b) takes less time than (c) wherever (c) is more than one call.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import itertools
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

AnyOf, Opt, Rep = GpuCodec.AnyOf, GpuCodec.Opt, GpuCodec.Rep
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def written_out(pattern):
    """every form of a list with Opt / Rep items, as lists of classes"""
    choices = []
    for c in pattern:
        if isinstance(c, Rep):
            choices.append([[c.cls] * k for k in range(c.lo, c.hi + 1)])
        elif isinstance(c, Opt):
            choices.append([[], [c.cls]])
        else:
            choices.append([[c]])
    return [sum(parts, []) for parts in itertools.product(*choices)]


def packed(forms, room=64):
    """the forms in as few AnyOf patterns as first-fit gives: at most `room` positions and `room` alternatives each"""
    calls = []
    for f in sorted(forms, key=len, reverse=True):
        for c in calls:
            if sum(map(len, c)) + len(f) <= room and len(c) < room:
                c.append(f)
                break
        else:
            calls.append([f])
    return [AnyOf(*c) for c in calls]


def patterns_of(load):
    if load.kind == "logtext":
        digits = b"0123456789"
        group = [Rep(digits, 1, 3), ord(".")]
        return [("heartbeats? ok", list(b"heartbeat") + [Opt(b"s")] + list(b" ok")),
                ("lag=[0-9]{1,5} ms", list(b"lag=") + [Rep(digits, 1, 5)] + list(b" ms")),
                ("a.b.c.d of [0-9]{1,3}", group * 3 + [Rep(digits, 1, 3)])]
    hist = load.histogram()
    hist[10] = 0
    top = hist.argsort(descending=True)[:16].tolist()
    group = [Rep(bytes(top[:10]), 1, 3), top[10]]
    return [("a word, one letter optional", [top[0], top[1], top[2], Opt(bytes([top[3]])), top[1], top[0]]),
            ("two values around {1,5}", [top[0], top[1], Rep(bytes(top[2:6]), 1, 5), top[0]]),
            ("four groups of {1,3}", group * 3 + [Rep(bytes(top[:10]), 1, 3)])]


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, codec = load.what, load.codec
    patterns = patterns_of(load)
    args = load.encode()

    def positions(pattern):
        cap = int(codec.count_pattern(*args, pattern)[0][0]) + 1
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        return lambda: codec.find_pattern(*args, pattern, max_positions=cap, out=out)[0][:cap - 1]

    def timed(calls):
        def run():
            t0 = time.perf_counter()
            found = [c() for c in calls]
            got = found[0] if len(found) == 1 else torch.unique(torch.cat(found))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, got
        return run

    rows, calls_of = [], {}
    for name, pattern in patterns:
        forms = written_out(pattern)
        pieces = packed(forms)
        calls_of[name] = len(pieces)
        rows += [((name, "(a) any-of"), timed([positions(AnyOf(max(forms, key=len)))])), ((name, "(b) quant"), timed([positions(pattern)])),
                 ((name, f"(c) forms, {len(pieces)} call" + "s" * (len(pieces) > 1)), timed([positions(p) for p in pieces]))]
    answers = {key: run()[1].clone() for key, run in rows}          # warm, and the answers
    for (name, row), found in answers.items():
        if row.startswith("(c)"):
            assert torch.equal(found, answers[name, "(b) quant"]), f"{name}: the quant call and the written-out forms differ"
    sizes = {key: int(a.numel()) for key, a in answers.items()}
    del answers

    times = dict(zip([key for key, _ in rows], alternate(runs, *[lambda run=run: run()[0] for _, run in rows])))
    for (name, row), _ in rows:
        print(f"{what:26s} {name:28s} {row:20s} {sizes[name, row]:10d} starts   {fmt(times[name, row])}", flush=True)
    med = {key: statistics.median(ts) for key, ts in times.items()}
    for name, _ in patterns:
        a, b = med[name, "(a) any-of"], med[name, "(b) quant"]
        c = next(v for (n, row), v in med.items() if n == name and row.startswith("(c)"))
        print(f"{what:26s} {name:28s} quant / any-of of the same length {b / a:.2f}x; the {calls_of[name]} call(s) over the forms / quant {c / b:.2f}x",
              flush=True)
        assert calls_of[name] == 1 or b < c, f"{name}: one quant call takes {b * 1e3:.3f} ms, the {calls_of[name]} calls it replaces {c * 1e3:.3f} ms"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

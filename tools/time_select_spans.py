"""hufgpu_select_spans - grep -o's non-overlapping matches, chosen on the device - behind the span call, against the span call
alone and against what a caller does without it: both arrays to the host, the greedy loop in numpy, the result back (GPU).

    python tools/time_select_spans.py [--runs 7] [--mib 1024] [--out profiles/find/time_select_spans.txt]

The inputs and patterns are tools/time_find_spans.py's - log text in blocks of 1 MiB, zipf255 bytes in blocks of 64 KiB -, and in
each input a run of 16 Mi bytes of one value that occurs nowhere else (block-aligned: one-symbol blocks), searched with
'v{1,64}': every byte of the run is a start, one in 64 is selected.  The caps are the exact counts, taken by count_pattern before
anything is timed.  Alternating in one process, median of --runs warm runs with [min, max], each from its first enqueue to one
synchronize.  Four rows a pattern:

  (a) spans      find_spans(the pattern): starts and lengths, overlapping ones included
  (b) matches    find_matches(the pattern): the same call and select_spans behind it, no host wait in between
  (c) recipe     find_spans, positions and lengths to the host, the loop of tests/select_spans_model.py, the result to the device
  (d) selection  select_spans alone, on the arrays and the count word that a span call has left on the device

In front of every timed run stands an untimed span call of the row's pattern and a synchronize: the recipe's host loop leaves the
device idle for a quarter of a second, and the row behind it would else be timed on a device that has clocked down.

The tool asserts that (b) and (c) give the same positions and lengths on every row.  (b) - (a), (d) and (c) / (b) are reported,
not asserted.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

from find_timing import ROOT, GpuCodec, Workload, alternate, fmt, main
from time_find_quant import patterns_of

sys.path.insert(0, os.path.join(ROOT, "tests"))
from select_spans_model import select_model  # noqa: E402

Opt, Rep = GpuCodec.Opt, GpuCodec.Rep
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")
RUN_VALUE = {"logtext": 1, "zipf255": 255}          # a byte value the input does not hold


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, codec = load.what, load.codec
    patterns = [(name, p, {}) for name, p in patterns_of(load)]
    if load.kind == "logtext":
        patterns.append(("-w heartbeats?", list(b"heartbeat") + [Opt(b"s")], {"word": True}))
    value = RUN_VALUE[load.kind]
    run_len = min(1 << 24, load.n // 4) // load.bs * load.bs
    at = load.n // 2 // load.bs * load.bs
    load.data[at:at + run_len] = value
    patterns.append(("v{1,64} over a run", [Rep(bytes([value]), 1, 64)], {}))
    args = load.encode()

    def as_call(pattern, kw):
        """an anchored pattern with Opt / Rep items is an Expr's"""
        return (GpuCodec.Expr(pattern, **kw), {}) if kw else (pattern, {})

    def calls(pattern, kw):
        pattern, kw = as_call(pattern, kw)
        cap = int(codec.count_pattern(*args, pattern, **kw)[0][0]) + 1

        def spans():
            return codec.find_spans(*args, pattern, max_positions=cap, want_open=False, **kw)[:3]

        def matches():
            pos, lens, totals = codec.find_matches(*args, pattern, max_positions=cap, want_open=False, **kw)[:3]
            return pos, lens, totals

        def recipe():
            pos, lens, totals = spans()
            n = int(totals[1])                                      # (the first wait)
            spos, slens, _, stotals = select_model(pos[:n].cpu().numpy().view(np.uint64), lens[:n].cpu().numpy())
            return torch.from_numpy(spos.view(np.int64)).cuda(), torch.from_numpy(slens).cuda(), torch.from_numpy(stotals).cuda()
        held = spans()

        def selection():
            return codec.select_spans(held[0], held[1], held[2][1:2])[3]
        return spans, matches, recipe, selection

    def timed(call, primer):
        def run():
            primer()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, got
        return run

    rows = []
    for name, pattern, kw in patterns:
        spans, matches, recipe, selection = calls(pattern, kw)
        rows += [((name, "(a) spans"), timed(spans, spans)), ((name, "(b) matches"), timed(matches, spans)),
                 ((name, "(c) recipe"), timed(recipe, spans)), ((name, "(d) selection"), timed(selection, spans))]
    answers = {key: run()[1] for key, run in rows}                  # warm, and the answers
    sizes = {}
    for name, _, _ in patterns:
        starts = int(answers[name, "(a) spans"][2][1])
        pos, lens, totals = answers[name, "(b) matches"]
        selected, written, status, _ = totals.tolist()
        assert status == 0 and selected == written, f"{name}: the selection's totals are {totals.tolist()}"
        rpos, rlens, rtotals = answers[name, "(c) recipe"]
        assert rtotals.tolist() == totals.tolist(), f"{name}: the device call and the recipe differ in the totals"
        assert torch.equal(pos[:written], rpos), f"{name}: the device call and the recipe differ in the positions"
        assert torch.equal(lens[:written], rlens), f"{name}: the device call and the recipe differ in the lengths"
        assert answers[name, "(d) selection"].tolist() == totals.tolist(), f"{name}: the selection alone differs in the totals"
        sizes[name] = (starts, selected)
    del answers

    times = dict(zip([key for key, _ in rows], alternate(runs, *[lambda run=run: run()[0] for _, run in rows])))
    for (name, row), _ in rows:
        print(f"{what:26s} {name:28s} {row:14s} {sizes[name][0]:10d} starts {sizes[name][1]:10d} selected   {fmt(times[name, row])}", flush=True)
    med = {key: statistics.median(ts) for key, ts in times.items()}
    for name, _, _ in patterns:
        a, b, c, d = (med[name, row] for row in ("(a) spans", "(b) matches", "(c) recipe", "(d) selection"))
        print(f"{what:26s} {name:28s} matches - spans {(b - a) * 1e3:.3f} ms ({(b - a) / a * 100:.1f} % of spans); the selection alone "
              f"{d * 1e3:.3f} ms; recipe / matches {c / b:.2f}x", flush=True)
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_any_spans - where each occurrence ends - against the positions call of the same pattern, and against what a caller
writes without it: one any-of call per distinct form length and the maximum per start in torch (GPU).

    python tools/time_find_spans.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_spans.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  The caps are the exact counts,
taken by count_pattern before anything is timed.  Alternating in one process, median of --runs warm runs with [min, max], each
from its first enqueue to one synchronize.  Three rows a pattern:

  (a) positions  find_pattern(the pattern): the quant call - the expr call for the -w row -, starts only
  (b) spans      find_spans(the pattern): the same chain and find_span_kernel behind it, starts and lengths
  (c) recipe     the older kernels: the written-out forms grouped by length, an AnyOf call a length (first-fit into the 64
                 positions: K calls in all), then torch.unique over the starts and the maximum length per start

  log text   'heartbeats? ok', 'lag=[0-9]{1,5} ms', '[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}', -w 'heartbeats?'
  zipf255    tools/time_find_quant.py's shapes over its most frequent values

The tool asserts that (b) and (c) give the same positions and lengths on every row, and that (b) takes less time than (c)
wherever (c) is more than one call.  (b) / (a) is reported, not asserted.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main
from time_find_quant import packed, patterns_of, written_out

AnyOf, Opt = GpuCodec.AnyOf, GpuCodec.Opt
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, codec = load.what, load.codec
    patterns = [(name, p, {}) for name, p in patterns_of(load)]
    if load.kind == "logtext":
        patterns.append(("-w heartbeats?", list(b"heartbeat") + [Opt(b"s")], {"word": True}))
    args = load.encode()

    def as_call(pattern, kw):
        """an anchored pattern with Opt / Rep items is an Expr's"""
        return (GpuCodec.Expr(pattern, **kw), {}) if kw else (pattern, {})

    def positions(pattern, kw):
        pattern, kw = as_call(pattern, kw) if not isinstance(pattern, AnyOf) else (pattern, kw)
        cap = int(codec.count_pattern(*args, pattern, **kw)[0][0]) + 1
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        return lambda: codec.find_pattern(*args, pattern, max_positions=cap, out=out, **kw)[0][:cap - 1]

    def spans(pattern, kw):
        pattern, kw = as_call(pattern, kw)
        cap = int(codec.count_pattern(*args, pattern, **kw)[0][0]) + 1
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))
        return lambda: tuple(t[:cap - 1] for t in codec.find_spans(*args, pattern, max_positions=cap, out=out, want_open=False, **kw)[:2])

    def recipe(pattern, kw):
        by_len = {}
        for f in written_out(pattern):
            by_len.setdefault(len(f), []).append(f)
        calls = [(length, positions(p, kw)) for length, fs in sorted(by_len.items()) for p in packed(fs)]

        def run():
            found = [(c(), length) for length, c in calls]
            starts, inverse = torch.unique(torch.cat([p for p, _ in found]), return_inverse=True)
            each = torch.cat([torch.full((p.numel(),), length, dtype=torch.int32, device="cuda") for p, length in found])
            longest = torch.zeros(starts.numel(), dtype=torch.int32, device="cuda").scatter_reduce_(0, inverse, each, "amax")
            return starts, longest
        return run, len(calls)

    def timed(call):
        def run():
            t0 = time.perf_counter()
            got = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, got
        return run

    rows, calls_of = [], {}
    for name, pattern, kw in patterns:
        older, calls_of[name] = recipe(pattern, kw)
        single, kws = as_call(pattern, kw)
        rows += [((name, "(a) positions"), timed(positions(single, kws))), ((name, "(b) spans"), timed(spans(pattern, kw))),
                 ((name, f"(c) recipe, {calls_of[name]} call" + "s" * (calls_of[name] > 1)), timed(older))]
    answers = {key: run()[1] for key, run in rows}                  # warm, and the answers
    sizes = {}
    for (name, row), found in answers.items():
        if row.startswith("(c)"):
            pos, lens = answers[name, "(b) spans"]
            assert torch.equal(found[0], pos), f"{name}: the span call and the recipe differ in the positions"
            assert torch.equal(found[1], lens), f"{name}: the span call and the recipe differ in the lengths"
            assert torch.equal(answers[name, "(a) positions"], pos), f"{name}: the span call and the positions call differ"
        sizes[name, row] = int((found if row.startswith("(a)") else found[0]).numel())
    del answers

    times = dict(zip([key for key, _ in rows], alternate(runs, *[lambda run=run: run()[0] for _, run in rows])))
    for (name, row), _ in rows:
        print(f"{what:26s} {name:28s} {row:22s} {sizes[name, row]:10d} starts   {fmt(times[name, row])}", flush=True)
    med = {key: statistics.median(ts) for key, ts in times.items()}
    for name, _, _ in patterns:
        a, b = med[name, "(a) positions"], med[name, "(b) spans"]
        c = next(v for (n, row), v in med.items() if n == name and row.startswith("(c)"))
        print(f"{what:26s} {name:28s} spans / positions {b / a:.2f}x; the recipe's {calls_of[name]} call(s) / spans {c / b:.2f}x", flush=True)
        assert calls_of[name] == 1 or b < c, f"{name}: the span call takes {b * 1e3:.3f} ms, the {calls_of[name]} calls it replaces {c * 1e3:.3f} ms"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_records_expr - anchors, terms and optional positions in ONE call - against the nearest single older call of the
same length, and against the recipe on the older calls that it replaces (GPU).

    python tools/time_find_expr.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_expr.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the records are the lines.  The
caps are the exact counts, taken by count_records before anything is timed.  Alternating in one process, median of --runs warm
runs with [min, max], each from its first enqueue to one synchronize.  Four patterns a workload, three rows a pattern:

  (a) older    ONE older call of the same length, every position required: the anchored call for the first two patterns, the
               terms call for the other two - the older kernels, unchanged
  (b) expr     find_records(Expr(...)): one call, one walk
  (c) recipe   what a caller writes today.  Anchors with optional positions: every form as an alternative of the anchored call
               (they fit the 64 positions here).  ALL of quantified terms: one quant call a term, and the intersection of the
               record starts in torch.  ORDERED with a quantified last term: the starts of both terms and of the delimiters
               (three calls), and in torch, a record, the first end of the first term against the last start of the second

  log text   '^2026-10-03T12:0[0-9]{1,3}', -w 'heartbeats?', 'ERROR.*lag=[0-9]{1,5} ms', 'heartbeats? ok' and 'lag=[0-9]{1,5} ms'
  zipf255    the same shapes over its most frequent values (the word bytes: the eight most frequent)

The tool asserts that (b) and (c) select the same records on every row, and that (b) takes less time than (c) wherever (c) is
more than one call; (b) / (a) is reported.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main
from time_find_quant import written_out

AnyOf, Opt, Rep, Expr, AllOf, Seq = GpuCodec.AnyOf, GpuCodec.Opt, GpuCodec.Rep, GpuCodec.Expr, GpuCodec.AllOf, GpuCodec.Seq
HEADER = ("{mib} MiB, records = lines, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def longest(pattern):
    return max(written_out(pattern), key=len)


def cases_of(load):
    """name -> (the Expr, the older call's pattern and keywords, the recipe: ("forms", keywords) | ("all", terms) | ("ordered", terms))"""
    if load.kind == "logtext":
        digits = b"0123456789"
        year = list(b"2026-10-03T12:0") + [Rep(digits, 1, 3)]
        beats = list(b"heartbeat") + [Opt(b"s")]
        beats_ok = beats + list(b" ok")
        lag = list(b"lag=") + [Rep(digits, 1, 5)] + list(b" ms")
        error, words = list(b"ERROR"), None
    else:
        hist = load.histogram()
        hist[10] = 0
        top = hist.argsort(descending=True)[:16].tolist()
        year = [Rep(bytes(top[:4]), 2, 4), top[0], top[1]]
        beats = [top[0], top[1], top[2], Opt(bytes([top[3]]))]
        beats_ok = [top[8], top[9], Opt(bytes([top[10]])), top[8]]
        lag = [top[0], top[1], Rep(bytes(top[2:6]), 1, 5), top[0]]
        error, words = [top[1], top[0], top[2]], bytes(top[:8])
    return {
        "^stamp x{1,3}": (Expr(year, bol=True), (AnyOf(longest(year)), dict(bol=True)), ("forms", year, dict(bol=True))),
        "-w, one letter optional": (Expr(beats, word=True, word_bytes=words), (AnyOf(longest(beats)), dict(word=True, word_bytes=words)),
                                    ("forms", beats, dict(word=True, word_bytes=words))),
        "A.*B{1,5}": (Expr(error, lag), (Seq(error, longest(lag)), {}), ("ordered", (error, lag))),
        "ALL of two quantified": (Expr(beats_ok, lag, ordered=False), (AllOf(longest(beats_ok), longest(lag)), {}), ("all", (beats_ok, lag))),
    }


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, codec = load.what, load.codec
    cases = cases_of(load)
    args = load.encode()
    n = args[5]

    def records(pattern, **kw):
        cap = int(codec.count_records(*args, pattern, **kw)[0][0]) + 1
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))
        return lambda: codec.find_records(*args, pattern, max_records=cap, out=out, **kw)[0][:cap - 1]

    def positions(pattern):
        cap = int((codec.count_pattern(*args, pattern) if not isinstance(pattern, bytes) else codec.find_bytes(*args, pattern, 0)[1:3])[0][0]) + 1
        out = torch.empty(cap, dtype=torch.int64, device="cuda")
        if isinstance(pattern, bytes):
            return lambda: codec.find_bytes(*args, pattern, cap, out=out)[0][:cap - 1]
        return lambda: codec.find_pattern(*args, pattern, max_positions=cap, out=out)[0][:cap - 1]

    def in_order(calls, first_len):
        """the records in which the first term's first occurrence ends at or in front of the second term's last start"""
        pa, pb, d = (c() for c in calls)
        ra, rb = torch.searchsorted(d, pa), torch.searchsorted(d, pb)          # the delimiters in front: the record's number
        nrec = int(d.numel()) + 1
        first = torch.full((nrec,), n, dtype=torch.int64, device="cuda").scatter_reduce(0, ra, pa, "amin")
        last = torch.full((nrec,), -1, dtype=torch.int64, device="cuda").scatter_reduce(0, rb, pb, "amax")
        rec = torch.nonzero(first + first_len <= last).flatten()
        return torch.where(rec > 0, d[(rec - 1).clamp(min=0)] + 1, torch.zeros_like(rec))

    def timed(calls, combine):
        def run():
            t0 = time.perf_counter()
            got = combine(calls)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, got
        return run

    one = lambda calls: calls[0]()                                  # noqa: E731

    def both(calls):
        a, b = (c() for c in calls)
        return a[torch.isin(a, b)]

    rows, calls_of = [], {}
    for name, (expr, (older, older_kw), recipe) in cases.items():
        if recipe[0] == "forms":
            calls, combine = [records(AnyOf(*written_out(recipe[1])), **recipe[2])], one
        elif recipe[0] == "all":
            calls, combine = [records(t) for t in recipe[1]], both
        else:
            first, second = recipe[1]
            calls = [positions(AnyOf(first)), positions(second), positions(b"\n")]
            combine = lambda calls, m=len(first): in_order(calls, m)             # noqa: E731
        calls_of[name] = len(calls)
        rows += [((name, "(a) older"), timed([records(older, **older_kw)], one)), ((name, "(b) expr"), timed([records(expr)], one)),
                 ((name, f"(c) recipe, {len(calls)} call" + "s" * (len(calls) > 1)), timed(calls, combine))]
    answers = {key: run()[1].clone() for key, run in rows}          # warm, and the answers
    for (name, row), found in answers.items():
        if row.startswith("(c)"):
            assert torch.equal(found, answers[name, "(b) expr"]), f"{name}: the expr call and the recipe differ"
    sizes = {key: int(a.numel()) for key, a in answers.items()}
    del answers

    times = dict(zip([key for key, _ in rows], alternate(runs, *[lambda run=run: run()[0] for _, run in rows])))
    for (name, row), _ in rows:
        print(f"{what:26s} {name:26s} {row:20s} {sizes[name, row]:10d} records  {fmt(times[name, row])}", flush=True)
    med = {key: statistics.median(ts) for key, ts in times.items()}
    for name in cases:
        a, b = med[name, "(a) older"], med[name, "(b) expr"]
        c = next(v for (m, row), v in med.items() if m == name and row.startswith("(c)"))
        print(f"{what:26s} {name:26s} expr / older call of the same length {b / a:.2f}x; the recipe's {calls_of[name]} call(s) / expr {c / b:.2f}x",
              flush=True)
        assert calls_of[name] == 1 or b < c, f"{name}: one expr call takes {b * 1e3:.3f} ms, the {calls_of[name]} calls it replaces {c * 1e3:.3f} ms"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_records_terms - the records that hold ALL of several terms, or all of them in order, in one walk - against the
recipes it replaces and against ONE any-of records call over the same alternatives (GPU).

    python tools/time_find_terms.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_terms.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the records are lines.  The
caps are the exact counts, taken by count_records / count_pattern before anything is timed.  Alternating in one process,
median of --runs warm runs with [min, max], each from its first enqueue to one synchronize:

  all of T        find_records(AllOf(w1 .. wT)): one call, one walk                                   T = 2 and T = 4
  T calls + join  find_records for each word, then the intersection of the T start lists in torch (cat, unique with counts)
  seq of 2        find_records(Seq(w1, w2)): one call, one walk
  2 + 2 + join    find_records for each of the two words - their intersection is the candidates -, find_pattern for each word,
                  then per candidate the first w1 in it and the first w2 behind that one's end, with searchsorted in torch
  any of T        ONE find_records(AnyOf(w1 .. wT)): the same alternatives without terms - the price of the terms

  log text   ERROR, "cache miss", "bytes)", "gc:" (the first two for T = 2 and for the sequence)
  zipf255    four strings of two of the four most frequent values that are no newline

The tool asserts that both sides of the first two comparisons give the same records.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
`rocprofv3 --kernel-trace --stats -- python tools/time_find_terms.py --trace` makes the log text's "all of 4" and "seq of 2"
calls six times each, nothing else.
"""
import statistics
import sys
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

LOG_WORDS = [b"ERROR", b"cache miss", b"bytes)", b"gc:"]
HEADER = ("{mib} MiB, caps = the exact counts, "
          "median of {runs} warm runs [min, max], from the first enqueue to one synchronize, the rows alternating in one process per workload")


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, kind, codec = load.what, load.kind, load.codec
    if kind == "logtext":
        words = LOG_WORDS
    else:
        hist = load.histogram()
        hist[10] = 0
        top = hist.argsort(descending=True)[:4].tolist()
        words = [bytes([top[0], top[1]]), bytes([top[2], top[0]]), bytes([top[1], top[3]]), bytes([top[3], top[2]])]
    args = load.encode()
    AllOf, Seq, AnyOf = GpuCodec.AllOf, GpuCodec.Seq, GpuCodec.AnyOf

    def count(pattern):
        return int(codec.count_records(*args, pattern)[0][0])

    rec_caps = {w: count(w) + 1 for w in words}
    pos_caps = {w: int(codec.count_pattern(*args, w)[0][0]) + 1 for w in words[:2]}

    def one_call(pattern):
        cap = count(pattern) + 1
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))

        def run():
            t0 = time.perf_counter()
            res = codec.find_records(*args, pattern, max_records=cap, out=out)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res[0][:cap - 1]
        return run

    def records_of(ws, bufs):
        return [codec.find_records(*args, w, max_records=rec_caps[w], out=b) for w, b in zip(ws, bufs)]

    def record_buffers(ws):
        return [(torch.empty(rec_caps[w], dtype=torch.int64, device="cuda"), torch.empty(rec_caps[w], dtype=torch.int32, device="cuda")) for w in ws]

    def all_recipe(ws):
        bufs = record_buffers(ws)

        def run():
            t0 = time.perf_counter()
            res = records_of(ws, bufs)
            starts, counts = torch.unique(torch.cat([r[0][:rec_caps[w] - 1] for r, w in zip(res, ws)]), return_counts=True)
            both = starts[counts == len(ws)]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, both
        return run

    def seq_recipe(a, b):
        bufs = record_buffers((a, b))
        pbufs = [torch.empty(pos_caps[w], dtype=torch.int64, device="cuda") for w in (a, b)]

        def run():
            t0 = time.perf_counter()
            ra, rb = records_of((a, b), bufs)
            pa = codec.find_pattern(*args, a, max_positions=pos_caps[a], out=pbufs[0])[0][:pos_caps[a] - 1]
            pb = codec.find_pattern(*args, b, max_positions=pos_caps[b], out=pbufs[1])[0][:pos_caps[b] - 1]
            sa, la = ra[0][:rec_caps[a] - 1], ra[1][:rec_caps[a] - 1]
            keep = torch.isin(sa, rb[0][:rec_caps[b] - 1], assume_unique=True)
            s, e = sa[keep], sa[keep] + la[keep]              # the candidates: the records that hold both words
            first = pa[torch.searchsorted(pa, s)]              # (a candidate holds the word: the index is in range)
            at = torch.searchsorted(pb, first + len(a))
            behind = pb[at.clamp(max=pb.numel() - 1)]
            got = s[(at < pb.numel()) & (behind < e)]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, got
        return run

    rows = []
    for T in (2, 4):
        rows += [(f"all of {T}", one_call(AllOf(*words[:T]))), (f"{T} calls + join", all_recipe(words[:T])),
                 (f"any of {T}", one_call(AnyOf(*words[:T])))]
    rows += [("seq of 2", one_call(Seq(*words[:2]))), ("2 + 2 + join", seq_recipe(*words[:2]))]
    answers = {name: run()[1].clone() for name, run in rows}     # warm, and the answers
    for T in (2, 4):
        assert torch.equal(answers[f"all of {T}"], answers[f"{T} calls + join"]), f"the one call and the {T} calls' intersection differ"
    assert torch.equal(answers["seq of 2"], answers["2 + 2 + join"]), "the one call and the join differ"
    assert 0 < answers["seq of 2"].numel() <= answers["all of 2"].numel()
    sizes = {name: int(a.numel()) for name, a in answers.items()}
    del answers

    times = dict(zip([name for name, _ in rows], alternate(runs, *[lambda run=run: run()[0] for _, run in rows])))
    for name, _ in rows:
        print(f"{what:26s} {name:16s} {sizes[name]:10d} records   {fmt(times[name])}", flush=True)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    print(f"{what:26s} seq of 2: {med['seq of 2'] * 1e3:.3f} ms, its recipe {med['2 + 2 + join'] * 1e3:.3f} ms: "
          f"{med['2 + 2 + join'] / med['seq of 2']:.2f}x", flush=True)
    for T in (2, 4):
        one, recipe, plain = med[f"all of {T}"], med[f"{T} calls + join"], med[f"any of {T}"]
        print(f"{what:26s} all of {T}: {one * 1e3:.3f} ms, its recipe {recipe * 1e3:.3f} ms: {recipe / one:.2f}x; "
              f"the same alternatives as one any-of call {plain * 1e3:.3f} ms: the terms cost {one / plain:.2f}x", flush=True)
    codec.close()


def trace(mib):
    """for `rocprofv3 --kernel-trace --stats -- python tools/time_find_terms.py --trace`: the log text, all of four words and
    the sequence of two, one counting call and five calls with outputs each, nothing else"""
    load = Workload(0, mib)
    codec = load.codec
    args = load.encode()
    for pattern in (GpuCodec.AllOf(*LOG_WORDS), GpuCodec.Seq(*LOG_WORDS[:2])):
        cap = int(codec.count_records(*args, pattern)[0][0]) + 1
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))
        for _ in range(5):
            codec.find_records(*args, pattern, max_records=cap, out=out)
        torch.cuda.synchronize()
    codec.close()


if __name__ == "__main__":
    if "--trace" in sys.argv:
        trace(1024)
    else:
        main(__file__, HEADER, one_workload)

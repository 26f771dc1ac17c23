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
import statistics
import time

import torch

from find_timing import Workload, alternate, fmt, main

HEADER = ("{mib} MiB, delimiter newline, caps = the exact counts, "
          "median of {runs} warm runs [min, max], the calls alternating in one process per workload")


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n = w.what, w.codec, w.n
    frequent = w.frequent(delimiter=10)
    planted, places = w.plant()
    absent = w.absent(frequent)
    args = w.encode()
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
        tr, ty, tp = alternate(runs, lambda: records()[0], lambda: recipe()[0], pattern_alone)
        mr, my, mp = statistics.median(tr), statistics.median(ty), statistics.median(tp)
        print(f"{what:26s} {name:18s} {matches:9d} matches {t[0]:9d} records   (i) find_records {fmt(tr)}   (ii) recipe {fmt(ty)} = "
              f"{my / mr:5.2f}x   (iii) find_pattern {fmt(tp)}: (i) is {mr / mp:5.2f}x of it, + {(mr - mp) * 1e3:.3f} ms", flush=True)
        assert mr <= my, f"find_records ({mr * 1e3:.3f} ms) takes longer than the recipe ({my * 1e3:.3f} ms)"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_records_context (grep -A / -B / -C) against the two-walk recipe it replaces (GPU).

    python tools/time_find_context.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_context.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the delimiter is the newline.
Two patterns each: a frequent one (the word ERROR; five times zipf255's most frequent value) and a rare one (the time stamp
of one of the log's lines; four bytes taken from the zipf255 data), and `context` 2 and 20 for each.  The caps are the exact
counts, taken by count_bytes / count_records before anything is timed.  Alternating in one process, median of --runs warm
runs with [min, max], each from its first enqueue to one synchronize:
  (i)   the context call with d_rec_no and d_rec_sel: one walk; starts, lengths, numbers and flags of the records to print;
  (ii)  the recipe from the older calls: find_records_select with numbers for the hits, find_bytes(newline) for where the
        neighbouring records lie, and on the device in torch the windows around the hits' numbers, their union, and the
        starts and lengths of those records from the list of newlines, the empty ones taken out;
  (iii) find_records_select with numbers alone: (i) - (iii) is the price of the context.
The tool asserts that (i) returns the same records as (ii) - starts, lengths, numbers, flags - and that (i) takes no longer
than (ii) on any row.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

CONTEXTS = (2, 20)
HEADER = ("{mib} MiB, delimiter newline, caps = the exact counts, "
          "median of {runs} warm runs [min, max], the calls alternating in one process per workload")


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n = w.what, w.codec, w.n
    frequent, rare = w.frequent(delimiter=10), w.rare()
    args = w.encode()
    nl_cap = int(codec.count_bytes(*args, b"\n")[0][0])
    nl_pos = torch.empty(nl_cap, dtype=torch.int64, device="cuda")
    zero, end = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), n, dtype=torch.int64, device="cuda")
    nrec = nl_cap + 1                                       # every record, the empty ones and the one behind the last newline

    for name, pat in ((f"frequent, {len(frequent)} bytes", frequent), (f"rare, {len(rare)} bytes", rare)):
        alts = GpuCodec.AnyOf(pat)
        mcap = int(codec.count_records(*args, alts)[0][0])
        assert mcap > 0, (name, pat)
        mout = (torch.empty(mcap, dtype=torch.int64, device="cuda"), torch.empty(mcap, dtype=torch.int32, device="cuda"),
                torch.empty(mcap, dtype=torch.int64, device="cuda"))

        def select():
            t0 = time.perf_counter()
            codec.find_records(*args, alts, b"\n", max_records=mcap, out=mout, line_numbers=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for c in CONTEXTS:
            cap = int(codec.count_records(*args, alts, context=c)[0][0])
            out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"),
                   torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.uint8, device="cuda"))

            def context():
                t0 = time.perf_counter()
                res = codec.find_records(*args, alts, b"\n", max_records=cap, out=out, context=c, line_numbers=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, res

            def recipe():
                t0 = time.perf_counter()
                no = codec.find_records(*args, alts, b"\n", max_records=mcap, out=mout, line_numbers=True)[5]
                nl = codec.find_bytes(*args, b"\n", max_positions=nl_cap, out=nl_pos)[0]
                edge = torch.zeros(nrec + 1, dtype=torch.int32, device="cuda")      # + 1 where a window opens, - 1 behind its end
                edge.index_add_(0, (no - c).clamp_(min=0), torch.ones_like(no, dtype=torch.int32))
                edge.index_add_(0, (no + c + 1).clamp_(max=nrec), torch.full_like(no, -1, dtype=torch.int32))
                numbers = torch.nonzero(torch.cumsum(edge[:nrec], 0) > 0).flatten()
                starts, ends = torch.cat([zero, nl + 1])[numbers], torch.cat([nl, end])[numbers]
                keep = ends > starts
                starts, numbers = starts[keep], numbers[keep]
                lens = ends[keep] - starts
                flags = torch.isin(numbers, no, assume_unique=True)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, starts, lens, numbers, flags

            _, want, want_lens, want_no, want_flags = recipe()
            _, (pos, lens, totals, errs, _, numbers, flags) = context()
            t = totals.cpu().tolist()
            assert int(errs.abs().max()) == 0 and t == [cap, cap, 0, 0] and want.numel() == cap, (t, cap, want.numel())
            assert torch.equal(pos, want) and torch.equal(lens.long(), want_lens)
            assert torch.equal(numbers, want_no) and torch.equal(flags.bool(), want_flags) and int(flags.sum()) == mcap
            del want, want_lens, want_no, want_flags, pos, lens, numbers, flags
            ti, ty, ts = alternate(runs, lambda: context()[0], lambda: recipe()[0], select)
            mi, my, ms = (statistics.median(x) for x in (ti, ty, ts))
            print(f"{what:26s} {name:18s} context {c:2d} {nl_cap:9d} newlines {mcap:9d} matching {cap:9d} reported records\n"
                  f"    (i)   context, numbers, flags   {fmt(ti)}\n"
                  f"    (ii)  the recipe                {fmt(ty)}   = {my / mi:5.2f}x of (i)\n"
                  f"    (iii) select, numbers           {fmt(ts)}   (i) is {mi / ms:5.2f}x of it, + {(mi - ms) * 1e3:.3f} ms", flush=True)
            assert mi <= my, f"the context call ({mi * 1e3:.3f} ms) takes longer than the recipe ({my * 1e3:.3f} ms)"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_records_select (grep -v, grep -n) against the two-walk recipe it replaces (GPU).

    python tools/time_find_select.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_select.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the delimiter is the newline.
Two patterns each: a frequent one of 5 bytes (the word ERROR; five times zipf255's most frequent value) and one that does not
occur but shares four bytes with it - the worst case of the inverted emit: every non-empty line is written.  The caps are the
exact counts, taken by count_bytes / count_records before anything is timed.  Alternating in one process, median of --runs
warm runs with [min, max], each from its first enqueue to one synchronize:
  (i)   the select call with HUFGPU_SELECT_INVERT: one walk, the starts and lengths of the non-empty records without a match;
        (i+n) the same call with d_rec_no;
  (ii)  the recipe: find_bytes(newline) + find_records_any + the set difference in torch on the device (every record's start
        and end from the newlines, the empty ones and those that find_records_any reported taken out);
  (iii) find_records_any alone: (i) - (iii) is the price of the invert kernel and of the longer emit;
        (iii+n) the select call without invert, with d_rec_no: (iii+n) - (iii) is the price of the numbers.
The tool asserts that (i) returns the same records as (ii) and that (i) takes no longer than (ii) on any row.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

HEADER = ("{mib} MiB, delimiter newline, caps = the exact counts, "
          "median of {runs} warm runs [min, max], the calls alternating in one process per workload")


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n = w.what, w.codec, w.n
    frequent = w.frequent(delimiter=10)
    absent = w.absent(frequent)
    args = w.encode()
    nl_cap = int(codec.count_bytes(*args, b"\n")[0][0])
    nl_pos = torch.empty(nl_cap, dtype=torch.int64, device="cuda")
    zero, end = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), n, dtype=torch.int64, device="cuda")

    for name, pat in (("frequent, 5 bytes", frequent), ("absent, 5 bytes", absent)):
        alts = GpuCodec.AnyOf(pat)
        mcap = int(codec.count_records(*args, alts)[0][0])
        cap = int(codec.count_records(*args, alts, invert=True)[0][0])
        mout = (torch.empty(mcap, dtype=torch.int64, device="cuda"), torch.empty(mcap, dtype=torch.int32, device="cuda"),
                torch.empty(mcap, dtype=torch.int64, device="cuda"))
        out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"),
               torch.empty(cap, dtype=torch.int64, device="cuda"))

        def select(invert, numbers):
            o, c = (out, cap) if invert else (mout, mcap)
            t0 = time.perf_counter()
            res = codec.find_records(*args, alts, b"\n", max_records=c, out=o if numbers else o[:2], invert=invert, line_numbers=numbers)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        def recipe():
            t0 = time.perf_counter()
            nl = codec.find_bytes(*args, b"\n", max_positions=nl_cap, out=nl_pos)[0]
            hit = codec.find_records(*args, alts, b"\n", max_records=mcap, out=mout[:2])[0]
            starts, ends = torch.cat([zero, nl + 1]), torch.cat([nl, end])
            keep = (ends > starts) & ~torch.isin(starts, hit, assume_unique=True)
            starts = starts[keep]
            lens = ends[keep] - starts
            torch.cuda.synchronize()
            return time.perf_counter() - t0, starts, lens

        def records_any():
            t0 = time.perf_counter()
            codec.find_records(*args, alts, b"\n", max_records=mcap, out=mout[:2])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        _, want, want_lens = recipe()
        _, (pos, lens, totals, errs, _, numbers) = select(True, True)
        t = totals.cpu().tolist()
        assert int(errs.abs().max()) == 0 and t == [cap, cap, 0, 0] and want.numel() == cap, (t, cap, want.numel())
        assert torch.equal(pos, want) and torch.equal(lens.long(), want_lens)
        assert torch.equal(numbers, torch.searchsorted(nl_pos, pos))        # the newlines in front of each start
        _, (pos2, lens2, totals2, _, _) = select(True, False)
        assert torch.equal(pos2, want) and torch.equal(lens2.long(), want_lens) and totals2.cpu().tolist() == t
        del want, want_lens, pos, lens, numbers, pos2, lens2
        ti, tn, ty, ta, tan = alternate(runs, lambda: select(True, False)[0], lambda: select(True, True)[0], lambda: recipe()[0],
                                        records_any, lambda: select(False, True)[0])
        mi, mn, my, ma, man = (statistics.median(x) for x in (ti, tn, ty, ta, tan))
        print(f"{what:26s} {name:18s} {nl_cap:9d} newlines {mcap:9d} matching {cap:9d} inverted records\n"
              f"    (i)     select, invert          {fmt(ti)}\n"
              f"    (i+n)   select, invert, numbers {fmt(tn)}   + {(mn - mi) * 1e3:.3f} ms\n"
              f"    (ii)    the recipe              {fmt(ty)}   = {my / mi:5.2f}x of (i)\n"
              f"    (iii)   find_records_any        {fmt(ta)}   (i) is {mi / ma:5.2f}x of it, + {(mi - ma) * 1e3:.3f} ms\n"
              f"    (iii+n) select, numbers         {fmt(tan)}   + {(man - ma) * 1e3:.3f} ms", flush=True)
        assert mi <= my, f"the select call ({mi * 1e3:.3f} ms) takes longer than the recipe ({my * 1e3:.3f} ms)"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

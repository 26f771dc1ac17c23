"""hufgpu_find_records_anchored (grep -w, grep -x) against the recipe of older calls and torch that it replaces (GPU).

    python tools/time_find_anchors.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_anchors.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB; the delimiter is the newline,
the word bytes are [A-Za-z0-9_].  Two patterns each: a frequent one (the word ERROR; five times zipf255's most frequent value)
and a rare one (the time stamp of one of the log's lines; four bytes taken from the zipf255 data), each with `word` and with
`whole_line`.  The caps are the exact counts, taken before anything is timed.  Alternating in one process, median of --runs
warm runs with [min, max], each from its first enqueue to one synchronize:
  (i)   the anchored records call: one walk; the starts and lengths of the records that hold a qualifying occurrence;
  (ii)  the recipe from the older calls: find_records for the records that hold the pattern at all, find_pattern for its
        starts, find_bytes for the boundary bytes (the bytes that are no word byte; the newlines), and on the device in torch
        the join: the starts whose neighbours are boundary bytes or absent, and the records that hold one of those;
  (iii) find_records alone, unanchored: (i) - (iii) is the price of the anchors.
The tool asserts that (i) returns the same records as (ii) and that (i) takes no longer than (ii) on any row.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import statistics
import time

import torch

from find_timing import GpuCodec, Workload, alternate, fmt, main

HEADER = ("{mib} MiB, delimiter newline, word bytes [A-Za-z0-9_], caps = the exact counts, "
          "median of {runs} warm runs [min, max], the calls alternating in one process per workload")


def among(sorted_pos, q):
    """is q[i] one of the ascending positions"""
    if sorted_pos.numel() == 0:
        return torch.zeros_like(q, dtype=torch.bool)
    at = torch.searchsorted(sorted_pos, q).clamp_(max=sorted_pos.numel() - 1)
    return sorted_pos[at] == q


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n = w.what, w.codec, w.n
    frequent, rare = w.frequent(delimiter=10), w.rare()
    args = w.encode()
    not_word = bytes(v for v in range(256) if v not in GpuCodec.WORD_BYTES)
    bounds = {}
    for name, values in (("word", not_word), ("whole_line", b"\n")):
        cap = int(codec.count_bytes(*args, values)[0][0])
        bounds[name] = (values, cap, torch.empty(cap, dtype=torch.int64, device="cuda"))

    for pname, pat in ((f"frequent, {len(frequent)} bytes", frequent), (f"rare, {len(rare)} bytes", rare)):
        mcap = int(codec.count_records(*args, pat)[0][0])
        pcap = int(codec.count_pattern(*args, pat)[0][0])
        assert mcap > 0 and pcap > 0, (pname, pat)
        mout = (torch.empty(mcap, dtype=torch.int64, device="cuda"), torch.empty(mcap, dtype=torch.int32, device="cuda"))
        pout = torch.empty(pcap, dtype=torch.int64, device="cuda")

        def plain():
            t0 = time.perf_counter()
            codec.find_records(*args, pat, b"\n", max_records=mcap, out=mout)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for anchor in ("word", "whole_line"):
            values, bcap, bout = bounds[anchor]
            kw = {anchor: True}
            cap = int(codec.count_records(*args, pat, **kw)[0][0])
            out = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda"))

            def anchored():
                t0 = time.perf_counter()
                res = codec.find_records(*args, pat, b"\n", max_records=cap, out=out, **kw)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, res

            def recipe():
                t0 = time.perf_counter()
                rpos, rlen = codec.find_records(*args, pat, b"\n", max_records=mcap, out=mout)[:2]
                p = codec.find_pattern(*args, pat, max_positions=pcap, out=pout)[0]
                b = codec.find_bytes(*args, values, max_positions=bcap, out=bout)[0]
                ok = ((p == 0) | among(b, p - 1)) & ((p + len(pat) == n) | among(b, p + len(pat)))
                q = p[ok]
                if q.numel():                               # the records that hold one of the starts that are left
                    at = torch.searchsorted(q, rpos).clamp_(max=q.numel() - 1)
                    keep = (q[at] >= rpos) & (q[at] < rpos + rlen)      # (behind the last start `at` is clamped: no start)
                else:
                    keep = torch.zeros_like(rpos, dtype=torch.bool)
                starts, lens = rpos[keep], rlen[keep]
                torch.cuda.synchronize()
                return time.perf_counter() - t0, starts, lens

            _, want, want_lens = recipe()
            _, (pos, lens, totals, errs, _) = anchored()
            t = totals.cpu().tolist()
            assert int(errs.abs().max()) == 0 and t == [cap, cap, 0, 0] and want.numel() == cap, (t, cap, want.numel())
            assert torch.equal(pos, want) and torch.equal(lens, want_lens)
            del want, want_lens, pos, lens
            ti, ty, ts = alternate(runs, lambda: anchored()[0], lambda: recipe()[0], plain)
            mi, my, ms = (statistics.median(x) for x in (ti, ty, ts))
            print(f"{what:26s} {pname:18s} {anchor:10s} {pcap:9d} starts {bcap:10d} boundary bytes {mcap:9d} records with the pattern "
                  f"{cap:9d} selected\n"
                  f"    (i)   the anchored records call  {fmt(ti)}\n"
                  f"    (ii)  the recipe                 {fmt(ty)}   = {my / mi:5.2f}x of (i)\n"
                  f"    (iii) find_records, unanchored   {fmt(ts)}   (i) is {mi / ms:5.2f}x of it, + {(mi - ms) * 1e3:.3f} ms", flush=True)
            assert mi <= my, f"the anchored call ({mi * 1e3:.3f} ms) takes longer than the recipe ({my * 1e3:.3f} ms)"
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_pattern against what a caller who greps a compressed stream had to do before it (GPU).

    python tools/time_find_pattern.py [--runs 7] [--mib 1024] [--out profiles/find/time_find_pattern.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  Three patterns each: a
frequent one of 5 bytes (the word ERROR; five times zipf255's most frequent value - a pattern whose every prefix is
frequent, the matcher's expensive kind), a string of 36 bytes that was planted at five places, four of them across block
seams, and one that does not occur but shares four bytes with the frequent one; max_positions = 2^20.  find_pattern is
timed from its enqueue to one synchronize.  Against it, alternating in one process, median of --runs warm runs with
[min, max]:
  (i)   what a caller does today: decode with the sub-index into an N-byte tensor, torch.nonzero of the first byte (a
        wait for the size), the candidates' bytes gathered and compared, torch.nonzero of the verdicts (a second wait);
  (ii)  that decode alone, enqueue to synchronize;
  (iii) find_bytes for the pattern's first byte: the same walk of the stream without the matcher and the seam launch.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import functools
import statistics
import time

import torch

import find_timing
from find_timing import Workload, alternate, main

CAP = 1 << 20
SLICE = 1 << 24          # candidates compared at a time by the yardstick
HEADER = "{mib} MiB, max_positions 2^20, median of {runs} warm runs [min, max], the calls alternating in one process per workload"
fmt = functools.partial(find_timing.fmt, width=9)


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n, bs = w.what, w.codec, w.n, w.bs
    frequent = w.frequent()
    planted, places = w.plant()
    absent = w.absent(frequent)
    stream, length, offs, nb, sub, _, _ = w.encode()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    pos = torch.empty(CAP, dtype=torch.int64, device="cuda")

    def decode_alone():
        t0 = time.perf_counter()
        codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codec.decode_result()
        return t1 - t0

    for name, pat in (("frequent, 5 bytes", frequent), ("planted, 36 bytes", planted), ("absent, 5 bytes", absent)):
        m = len(pat)
        pat_t = torch.frombuffer(bytearray(pat), dtype=torch.uint8).cuda()
        span = torch.arange(m, device="cuda")

        def yardstick():
            t0 = time.perf_counter()
            codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
            cand = torch.nonzero(out[:n - m + 1] == pat[0]).view(-1)                    # (waits for the size)
            keep = [c[(out[c[:, None] + span] == pat_t).all(1)] for c in cand.split(SLICE)]   # (waits for each size)
            p = torch.cat(keep) if keep else cand
            t1 = time.perf_counter()
            codec.decode_result()
            return t1 - t0, p

        def find():
            t0 = time.perf_counter()
            _, totals, errs, _ = codec.find_pattern(stream, length, offs, nb, sub, n, bs, pat, max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            return t1 - t0, totals, errs

        def first_byte():
            t0 = time.perf_counter()
            codec.find_bytes(stream, length, offs, nb, sub, n, bs, pat[:1], max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        _, p = yardstick()
        _, totals, errs = find()
        t = totals.cpu().tolist()
        assert t == [p.numel(), min(p.numel(), CAP), 0, 0] and int(errs.abs().max()) == 0, (t, p.numel())
        assert torch.equal(pos[:t[1]], p[:t[1]])
        if pat is planted:
            assert p.cpu().tolist() == sorted(places)
        del p
        ty, tf, td, tb = alternate(runs, lambda: yardstick()[0], lambda: find()[0], decode_alone, first_byte)
        mf = statistics.median(tf)
        print(f"{what:28s} {name:18s} {t[0]:10d} matches   decode + torch search {fmt(ty)}   find_pattern {fmt(tf)} = "
              f"{statistics.median(ty) / mf:5.2f}x   decode alone {fmt(td)} = {statistics.median(td) / mf:5.2f}x   "
              f"find_bytes(first byte) {fmt(tb)} = {statistics.median(tb) / mf:5.2f}x of find_pattern", flush=True)
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""hufgpu_find_bytes against what a caller who wants the positions of byte values had to do before it (GPU).

    python tools/time_find.py [--runs 7] [--mib 1024] [--out profiles/find/time_find.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  Three sets each: {10} (the
newline; a frequent value of zipf255), one rare value, and 128 values; max_positions = 2^20.  find_bytes is timed from
its enqueue to one synchronize.  The yardstick is what a caller does today: decode with the sub-index into an N-byte
tensor, torch.nonzero over it (out == v; a 256-entry table look-up for the 128 values) and the wait for the result's size.
The two alternate in one process; every figure is the median of --runs warm runs with [min, max].  The indexed decode alone
(enqueue to synchronize, no nonzero) is timed in the same loop: find_sub_kernel reads the same bytes and writes an eighth.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import functools
import statistics
import time

import numpy as np
import torch

import find_timing
from find_timing import Workload, alternate, main

CAP = 1 << 20
HEADER = "{mib} MiB, max_positions 2^20, median of {runs} warm runs [min, max], the calls alternating in one process per workload"
fmt = functools.partial(find_timing.fmt, width=9)


def one_workload(k, runs, mib):
    w = Workload(k, mib)
    what, codec, n, bs = w.what, w.codec, w.n, w.bs
    hist = w.histogram().cpu().numpy()
    stream, length, offs, nb, sub, _, _ = w.encode()
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    present = np.flatnonzero(hist)
    rare = int(present[hist[present].argmin()])
    half = [int(v) for v in np.random.default_rng(7).permutation(256)[:128]]
    sets = [("{10}", [10]), (f"rare {{{rare}}}", [rare]), ("128 values", half)]
    pos = torch.empty(CAP, dtype=torch.int64, device="cuda")

    def decode_alone():
        t0 = time.perf_counter()
        codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codec.decode_result()
        return t1 - t0

    for name, values in sets:
        lut = torch.zeros(256, dtype=torch.bool, device="cuda")
        lut[torch.tensor(values, device="cuda")] = True

        def yardstick():
            t0 = time.perf_counter()
            codec.decode(stream, length, offs, nb, out, sync=False, sub_index=sub, raw_size=n, blocksize=bs)
            p = torch.nonzero(out == values[0] if len(values) == 1 else lut[out.int()]).view(-1)   # (waits for the size)
            t1 = time.perf_counter()
            codec.decode_result()
            return t1 - t0, p

        def find():
            t0 = time.perf_counter()
            _, totals, errs, _ = codec.find_bytes(stream, length, offs, nb, sub, n, bs, values, max_positions=CAP, out=pos)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            return t1 - t0, totals, errs

        _, p = yardstick()
        _, totals, errs = find()
        t = totals.cpu().tolist()
        assert t == [p.numel(), min(p.numel(), CAP), 0, 0] and int(errs.abs().max()) == 0, t
        assert torch.equal(pos[:t[1]], p[:t[1]])
        del p
        ty, tf, td = alternate(runs, lambda: yardstick()[0], lambda: find()[0], decode_alone)
        print(f"{what:28s} {name:12s} {t[0]:11d} matches   decode + nonzero {fmt(ty)}   find_bytes {fmt(tf)} = "
              f"{statistics.median(ty) / statistics.median(tf):5.2f}x   decode alone {fmt(td)} = "
              f"{statistics.median(td) / statistics.median(tf):5.2f}x of find_bytes", flush=True)
    codec.close()


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

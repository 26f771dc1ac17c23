"""hufgpu_update_ranges against what the API offered before it (GPU): byte ranges overwritten in one compressed buffer.

    python tools/time_update.py [--runs 5] [--mib 1024] [--out profiles/update/time_update.txt]

1 GiB of zipf255 bytes in 64 KiB blocks, device-resident, encoded with its sub-index.  Workloads: 1, 64 and 4 096 ranges
of 4 KiB at random unaligned positions, 64 ranges of 64 KiB (unaligned), one range of 16 MiB, the whole data [0, N).
Each is the call up to its synchronised result (new stream, new index, new sub-index), against
  (a) what a caller did before: hufgpu_decode of the whole stream (the index-only decoder) + one device copy per patch +
      hufgpu_encode_sub of the whole, and
  (b) the floor: a device copy of stream_len bytes by the library's own mover (hufgpu_calib_bandwidth, copy, variant 0)
      in the same process.
Every figure is the median of --runs warm runs with [min, max].  The result of every workload is compared with (a)'s
stream, index and length.  Last, as an estimate from outside: a call whose one range lies in the last block (the copy
moves all other records) beside the same call on a stream of 16 blocks (the fixed cost).  The kernels' own times come
from a trace: `rocprofv3 --kernel-trace --stats -- python tools/time_update.py --trace` runs that one call five times
and the calibration copy five times, nothing else.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd.codec import GpuCodec  # noqa: E402

BS = 65536


def stats(ts):
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def timed(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def fmt(s):
    return f"{s[0]:10.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


class Setup:
    def __init__(self, codec, n):
        self.codec, self.n = codec, n
        self.data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), "zipf255")
        self.sub = codec.new_sub_index(n, BS)
        self.stream, self.offs, self.length = codec.encode(self.data, BS, sub_index=self.sub)
        self.stream = self.stream.clone()
        self.nb = codec.block_count(n, BS)
        self.bound = codec.encode_bound(n, BS)
        self.out = torch.empty(self.bound, dtype=torch.uint8, device="cuda")
        self.new_offs = torch.empty(self.nb + 1, dtype=torch.int64, device="cuda")
        self.new_sub = codec.new_sub_index(n, BS)
        self.whole = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.out_a = torch.empty(self.bound, dtype=torch.uint8, device="cuda")
        self.offs_a = torch.empty(self.nb + 1, dtype=torch.int64, device="cuda")
        self.sub_a = codec.new_sub_index(n, BS)


def update_call(s, ranges, src):
    lib, ctx = s.codec.lib, s.codec._ctx
    r = len(ranges)
    lo = (C.c_uint64 * r)(*[a for a, _ in ranges])
    hi = (C.c_uint64 * r)(*[b for _, b in ranges])
    res = {}

    def fn():
        out_len, count = C.c_uint64(0), C.c_uint64(0)
        rc = lib.hufgpu_update_ranges(ctx, s.stream.data_ptr(), s.length, s.offs.data_ptr(), s.nb, r, lo, hi, None,
                                      src.data_ptr(), s.sub.data_ptr(), s.n, BS, s.out.data_ptr(), s.out.numel(),
                                      s.new_offs.data_ptr(), s.new_sub.data_ptr(), 0, C.byref(out_len), C.byref(count), None)
        assert rc == 0, lib.hufgpu_last_error(ctx).decode()
        res["len"], res["count"] = int(out_len.value), int(count.value)
    return fn, res


def before_call(s, ranges, src):
    """(a): decode everything, patch, encode everything"""
    codec = s.codec
    starts = np.concatenate([[0], np.cumsum([b - a for a, b in ranges])])
    res = {}

    def fn():
        raw = codec.decode(s.stream, s.length, s.offs, s.nb, s.whole)
        assert raw == s.n
        for (a, b), at in zip(ranges, starts):
            s.whole[a:b].copy_(src[int(at):int(at) + b - a])
        _, _, res["len"] = codec.encode(s.whole, BS, out=s.out_a, offsets=s.offs_a, sub_index=s.sub_a)
    return fn, res


def random_ranges(n, count, size, seed):
    """non-overlapping ranges of `size` bytes at random unaligned positions"""
    rng = np.random.default_rng(seed)
    slots = rng.choice(n // (2 * size) - 1, size=count, replace=False)
    return [int(k) * 2 * size + 1 + int(rng.integers(0, size - 1)) for k in slots]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="only the launches a kernel trace wants: one small update and the calibration copy, five times each")
    args = ap.parse_args()
    if args.trace:
        codec = GpuCodec(0)
        n = args.mib << 20
        s = Setup(codec, n)
        src = torch.from_numpy(np.arange(50, dtype=np.uint8)).cuda()
        fn_u, _ = update_call(s, [(n - 100, n - 50)], src)
        moved = (s.length + 65535) & ~65535
        a, b = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
        for _ in range(5):
            fn_u()
            codec.calib_bandwidth("copy", 0, a, b, moved)
        torch.cuda.synchronize()
        print(f"stream {s.length} bytes, calibration copy {moved} bytes")
        codec.close()
        return
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    codec = GpuCodec(0)
    n = args.mib << 20
    s = Setup(codec, n)
    say(f"hufgpu_update_ranges: {args.mib} MiB of zipf255 in {BS >> 10} KiB blocks ({s.nb} blocks), stream {s.length} bytes "
        f"({s.length / n:.3f} of the data); median of {args.runs} warm runs [min, max]")

    # (b) the floor: the library's own copy of stream_len bytes (rounded up to the mover's 64 KiB granule)
    moved = (s.length + 65535) & ~65535
    src_b = torch.empty(moved, dtype=torch.uint8, device="cuda")
    dst_b = torch.empty(moved, dtype=torch.uint8, device="cuda")
    floor = stats(timed(lambda: codec.calib_bandwidth("copy", 0, src_b, dst_b, moved), args.runs))
    say(f"(b) floor: device copy of {moved} bytes (hufgpu_calib_bandwidth copy, variant 0) {fmt(floor)}"
        f" = {2 * moved / floor[0] / 1e6:.0f} GB/s read + write")
    del src_b, dst_b

    work = []
    for count, size in ((1, 4096), (64, 4096), (4096, 4096), (64, 65536)):
        starts = random_ranges(n, count, size, seed=count + size)
        work.append((f"{count:5d} x {size >> 10:3d} KiB, unaligned", sorted((a, a + size) for a in starts)))
    if n >= 64 << 20:
        work.append(("    1 x  16 MiB, unaligned", [(n // 3 + 12345, n // 3 + 12345 + (16 << 20))]))
    work.append(("    1 x the whole data", [(0, n)]))

    say()
    say(f"{'ranges':<30} {'blocks':>7}  {'update_ranges':<34} {'(a) decode + patch + encode':<34} {'(a)/call':>8} {'call/(b)':>8}")
    rng = np.random.default_rng(99)
    for name, ranges in work:
        total = sum(b - a for a, b in ranges)
        src = torch.from_numpy(rng.integers(0, 200, total, dtype=np.uint8)).cuda()
        fn_u, res_u = update_call(s, ranges, src)
        fn_a, res_a = before_call(s, ranges, src)
        t_u = stats(timed(fn_u, args.runs))
        t_a = stats(timed(fn_a, args.runs))
        same = (res_u["len"] == res_a["len"] and torch.equal(s.out[:res_u["len"]], s.out_a[:res_a["len"]])
                and torch.equal(s.new_offs, s.offs_a))
        say(f"{name:<30} {res_u['count']:7d}  {fmt(t_u):<34} {fmt(t_a):<34} {t_a[0] / t_u[0]:8.1f} {t_u[0] / floor[0]:8.2f}"
            f"{'' if same else '   RESULTS DIFFER'}")
        del src

    # the copy kernel alone: a call whose one range lies in the last block moves every other record; the same call on a
    # stream of 16 blocks costs the fixed part (plan, one block decoded, encoded and packed, two waits)
    say()
    last = [(n - 100, n - 50)]
    src = torch.from_numpy(rng.integers(0, 200, 50, dtype=np.uint8)).cuda()
    fn_u, _ = update_call(s, last, src)
    t_big = stats(timed(fn_u, args.runs))
    small = Setup(codec, 16 * BS)
    fn_s, _ = update_call(small, [(16 * BS - 100, 16 * BS - 50)], src)
    t_small = stats(timed(fn_s, args.runs))
    copy_ms = t_big[0] - t_small[0]
    say(f"one range in the last block: {fmt(t_big)}; the same on 16 blocks (fixed cost): {fmt(t_small)}")
    say(f"copy kernel and the launches that grow with the stream (difference): {copy_ms:.3f} ms for {s.length} bytes = {2 * s.length / copy_ms / 1e6:.0f} GB/s read + write; "
        f"copy ceiling (b) {2 * moved / floor[0] / 1e6:.0f} GB/s: {copy_ms / floor[0]:.2f} x the floor")
    codec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

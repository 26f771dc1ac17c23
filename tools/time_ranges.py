"""hufgpu_decode_ranges against what the API offered before it (GPU): byte ranges out of one compressed buffer.

    python tools/time_ranges.py [--runs 5] [--mib 1024] [--out profiles/ranges/time_ranges.txt]
    python tools/time_ranges.py --tiles-only [--out profiles/ranges/time_ranges_tiles.txt]

1 GiB of zipf255 bytes in 64 KiB blocks, device-resident.  R = 1, 64, 4096 random ranges of 4 KiB, of 64 KiB at
unaligned positions, and of 16 MiB, slots back to back; with and without the encoder's sub-index.  Against
  (a) hufgpu_decode (hufgpu_decode_sub) of the WHOLE stream into a buffer of its own + one device copy per range, and
  (b) per range: hufgpu_decode of the covering blocks into a temporary + one device copy of the slice (no sub-index: a
      block sub-range cannot be given to hufgpu_decode_sub).
Every figure is the median of --runs warm runs with [min, max]; the slots of every variant are compared with slices of
the input.  Cases whose output would pass 8 GiB are left out.  Last: the single range [0, N) - every block direct -
against hufgpu_decode / hufgpu_decode_sub of the same stream in the same process.

The sub=1 lines carry a column for HUFGPU_RANGES_TILES (cut blocks decoded by the sub-index tile, not whole), and the
tile lines - all that --tiles-only runs - set the call with the flag beside the same call without it, alternating, in
the same process: 4 096 x 64 B and 4 096 x 4 KiB out of 64 KiB blocks, 1 x 4 KiB and 64 x 4 KiB out of the same bytes
written as ONE block (blocksize = 0), each with the route hufgpu_ranges_counters() reports.
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
TILES = 4               # HUFGPU_RANGES_TILES
OUT_CAP = 8 << 30


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
    def __init__(self, codec, n, bs=BS, data=None):
        self.codec, self.n, self.bs = codec, n, bs
        self.data = codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), "zipf255") if data is None else data
        self.sub = codec.new_sub_index(n, bs)
        self.stream, self.offs, self.length = codec.encode(self.data, bs, sub_index=self.sub)
        self.nb = codec.block_count(n, bs)
        self.whole = torch.empty(n, dtype=torch.uint8, device="cuda") if data is None else None


def ranges_call(s, lo, hi, oo, out, sub, flags=0):
    lib, ctx = s.codec.lib, s.codec._ctx
    r = len(lo)
    errs, raws = (C.c_int32 * r)(), (C.c_uint64 * r)()

    def fn():
        rc = lib.hufgpu_decode_ranges(ctx, s.stream.data_ptr(), s.length, s.offs.data_ptr(), s.nb, r, lo, hi, oo,
                                      s.sub.data_ptr() if sub else None, s.n if sub else 0, s.bs if sub else 0,
                                      out.data_ptr(), flags, errs, raws, None)
        assert rc == 0
    return fn


def whole_call(s, sub, ranges=None, oo=None, out=None):
    lib, ctx = s.codec.lib, s.codec._ctx
    raw = C.c_uint64(0)

    def fn():
        if sub:
            rc = lib.hufgpu_decode_sub(ctx, s.stream.data_ptr(), s.length, s.offs.data_ptr(), s.n, BS, s.sub.data_ptr(),
                                       s.whole.data_ptr(), s.n, 0, C.byref(raw), None)
        else:
            rc = lib.hufgpu_decode(ctx, s.stream.data_ptr(), s.length, s.offs.data_ptr(), s.nb, s.whole.data_ptr(), s.n, 0,
                                   C.byref(raw), None)
        assert rc == 0 and raw.value == s.n
        if ranges:
            for i, (a, b) in enumerate(ranges):
                out[oo[i]:oo[i + 1]] = s.whole[a:b]
    return fn


def loop_call(s, ranges, oo, out, tmp):
    lib, ctx = s.codec.lib, s.codec._ctx
    raw = C.c_uint64(0)
    base = s.offs.data_ptr()

    def fn():
        for i, (a, b) in enumerate(ranges):
            fb, lb = a // BS, (b - 1) // BS
            rc = lib.hufgpu_decode(ctx, s.stream.data_ptr(), s.length, base + 8 * fb, lb - fb + 1, tmp.data_ptr(), tmp.numel(),
                                   0, C.byref(raw), None)
            assert rc == 0
            out[oo[i]:oo[i + 1]] = tmp[a - fb * BS:b - fb * BS]
    return fn


def check(s, ranges, oo, out, what):
    for i in list(range(min(len(ranges), 8))) + [len(ranges) - 1]:
        a, b = ranges[i]
        assert torch.equal(out[oo[i]:oo[i + 1]], s.data[a:b]), f"{what}: range {i} differs from the input"


def case(s, r, size, aligned, runs, lines):
    rng = np.random.default_rng(r * 31 + size)
    if r * size > OUT_CAP:
        lines.append(f"R={r:5d} x {size:9d} B: left out (the slots would take {r * size >> 30} GiB)")
        print(lines[-1], flush=True)
        return
    step = 4096 if aligned else 1
    los = (rng.integers(0, (s.n - size) // step + 1, r) * step).tolist()
    if not aligned:
        los = [x | 1 if x + 1 + size <= s.n else x for x in los]
    ranges = [(x, x + size) for x in los]
    oo_l = [i * size for i in range(r + 1)]
    lo, hi, oo = (C.c_uint64 * r)(*los), (C.c_uint64 * r)(*[x + size for x in los]), (C.c_uint64 * (r + 1))(*oo_l)
    out = torch.empty(r * size, dtype=torch.uint8, device="cuda")
    tmp = torch.empty((size // BS + 2) * BS, dtype=torch.uint8, device="cuda")
    res = {}
    for sub in (False, True):
        out.zero_()
        fn = ranges_call(s, lo, hi, oo, out, sub)
        fn()
        check(s, ranges, oo_l, out, "decode_ranges")
        res["new", sub] = stats(timed(fn, runs))
        if sub:
            out.zero_()
            fn = ranges_call(s, lo, hi, oo, out, sub, TILES)
            fn()
            check(s, ranges, oo_l, out, "decode_ranges, tiles")
            res["tiles"] = stats(timed(fn, runs))
        out.zero_()
        fn = whole_call(s, sub, ranges, oo_l, out)
        fn()
        check(s, ranges, oo_l, out, "whole + slices")
        res["whole", sub] = stats(timed(fn, runs))
    out.zero_()
    fn = loop_call(s, ranges, oo_l, out, tmp)
    fn()
    check(s, ranges, oo_l, out, "loop")
    loop = stats(timed(fn, runs))
    for sub in (False, True):
        new, whole = res["new", sub], res["whole", sub]
        flag = f"tiles {fmt(res['tiles'])} = {new[0] / res['tiles'][0]:6.2f}x   " if sub else ""
        lines.append(f"R={r:5d} x {size:9d} B {'aligned  ' if aligned else 'unaligned'} sub={int(sub)}  ranges {fmt(new)}   {flag}"
                     f"(a) whole + slices {fmt(whole)} = {whole[0] / new[0]:8.1f}x   (b) loop {fmt(loop)} = {loop[0] / new[0]:8.1f}x")
        print(lines[-1], flush=True)


def whole_range(s, runs, lines):
    lo, hi, oo = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(s.n), (C.c_uint64 * 2)(0, s.n)
    out = torch.empty(s.n, dtype=torch.uint8, device="cuda")
    for sub in (False, True):
        fn = ranges_call(s, lo, hi, oo, out, sub)
        fn()
        assert torch.equal(out, s.data)
        plain = stats(timed(whole_call(s, sub), runs))
        new = stats(timed(fn, runs))
        plain2 = stats(timed(whole_call(s, sub), runs))
        ref = min(plain[0], plain2[0])
        lines.append(f"[0, N) sub={int(sub)}: ranges {fmt(new)}   {'hufgpu_decode_sub' if sub else 'hufgpu_decode'} {fmt(plain)} and again {fmt(plain2)}"
                     f"   ratio {new[0] / ref:.3f}")
        print(lines[-1], flush=True)


def tile_line(s, r, size, runs, lines, what):
    """the same call without and with the flag, alternating: `runs` warm runs of each"""
    rng = np.random.default_rng(r * 17 + size)
    los = [int(x) | 1 for x in rng.integers(0, s.n - size - 1, r)]
    ranges = [(x, x + size) for x in los]
    oo_l = [i * size for i in range(r + 1)]
    lo, hi, oo = (C.c_uint64 * r)(*los), (C.c_uint64 * r)(*[x + size for x in los]), (C.c_uint64 * (r + 1))(*oo_l)
    out = torch.empty(r * size, dtype=torch.uint8, device="cuda")
    fns, ts, route = {}, {0: [], TILES: []}, {}
    for flags in (0, TILES):
        out.zero_()
        fns[flags] = ranges_call(s, lo, hi, oo, out, True, flags)
        fns[flags]()
        check(s, ranges, oo_l, out, f"{what}, flags {flags}")
        route[flags] = s.codec.ranges_counters()[:5]
    for _ in range(runs):
        for flags in (0, TILES):
            ts[flags] += timed(fns[flags], 1)
    plain, tiles = stats(ts[0]), stats(ts[TILES])
    lines.append(f"{what}: R={r:5d} x {size:5d} B  without the flag {fmt(plain)}   with {fmt(tiles)} = {plain[0] / tiles[0]:7.2f}x   "
                 f"(direct, staged, tiles, items, failed) {route[0]} -> {route[TILES]}")
    print(lines[-1], flush=True)


def tile_lines(s, runs, lines):
    tile_line(s, 4096, 64, runs, lines, "blocks of 64 KiB")
    tile_line(s, 4096, 4096, runs, lines, "blocks of 64 KiB")
    one = Setup(s.codec, s.n, 0, s.data)
    tile_line(one, 1, 4096, runs, lines, "ONE block        ")
    tile_line(one, 64, 4096, runs, lines, "ONE block        ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiles-only", action="store_true", help="only the lines that compare HUFGPU_RANGES_TILES with the same call without it")
    a = ap.parse_args()
    codec = GpuCodec(0)
    s = Setup(codec, a.mib << 20)
    lines = [f"time_ranges.py: {torch.cuda.get_device_name(0)}, {a.mib} MiB of zipf255 in blocks of {BS}, median of {a.runs} warm runs "
             "[min, max]; a call = everything up to the synchronised result, slots on the device"]
    print(lines[0], flush=True)
    if not a.tiles_only:
        for size, aligned in ((4096, True), (65536, False), (16 << 20, False)):
            for r in (1, 64, 4096):
                if size <= s.n:
                    case(s, r, size, aligned, a.runs, lines)
        whole_range(s, a.runs, lines)
    tile_lines(s, a.runs, lines)
    codec.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""hufgpu_append against what the API offered before it (GPU): bytes appended to one compressed buffer, in place.

    python tools/time_append.py [--runs 5] [--out profiles/append/time_append.txt]

zipf255 bytes in 64 KiB blocks, device-resident: streams of 16 MiB and of 1 GiB, each with a tail of t = 0 and of
t = 32 KiB, and A of 4 KiB, 64 KiB, 1 MiB and 16 MiB appended - without a sub-index and with both sub-indexes.  Each
figure is the call up to its synchronised result, the median of --runs warm runs with [min, max]; the stream's last
record and index entry are put back between runs, outside the timed part.  Yardsticks, in the same process:
  (a) hufgpu_encode_sub of the whole D ++ A, and
  (b) hufgpu_encode of A alone, plus hufgpu_decode of one block when t > 0.
The result of every call is compared with (a)'s stream, index and length.  The kernels' own times come from a trace:
`rocprofv3 --kernel-trace --stats -- python tools/time_append.py --trace` makes one append five times, nothing else.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd.codec import GpuCodec  # noqa: E402

BS = 65536
KIB, MIB = 1 << 10, 1 << 20
A_SIZES = (4 * KIB, 64 * KIB, MIB, 16 * MIB)


def stats(ts):
    return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def timed(fn, runs, reset=None):
    ts = []
    for i in range(runs + 1):                           # the first run warms up
        if reset:
            reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            ts.append(time.perf_counter() - t0)
    return ts


def fmt(s):
    return f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


class Stream:
    """D = whole[:raw] encoded with its sub-index into buffers with room for the longest append"""

    def __init__(self, codec, whole, raw):
        self.codec, self.whole, self.raw = codec, whole, raw
        grow = max(A_SIZES)
        self.nb = codec.block_count(raw, BS)
        self.stream = torch.empty(codec.encode_bound(raw + grow, BS), dtype=torch.uint8, device="cuda")
        self.offs = torch.empty(codec.block_count(raw + grow, BS) + 1, dtype=torch.int64, device="cuda")
        self.sub = codec.new_sub_index(raw, BS)
        _, _, self.length = codec.encode(whole[:raw], BS, out=self.stream, offsets=self.offs, sub_index=self.sub)
        t = raw % BS
        self.keep = self.nb - (1 if t else 0)
        base = int(self.offs[self.keep].item())
        self.base = base
        self.saved_tail = self.stream[base:self.length].clone()
        self.saved_offs = self.offs[: self.nb + 1].clone()
        self.last = torch.empty(BS, dtype=torch.uint8, device="cuda")
        self.new_sub = codec.new_sub_index(raw + grow, BS)

    def reset(self):
        self.stream[self.base:self.length].copy_(self.saved_tail)
        self.offs[: self.nb + 1].copy_(self.saved_offs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-mib", type=int, default=16)
    ap.add_argument("--large-mib", type=int, default=1024)
    ap.add_argument("--trace", action="store_true", help="only the launches a kernel trace wants: one append of 64 KiB to the large stream with t = 32 KiB, five times")
    args = ap.parse_args()
    codec = GpuCodec(0)
    sizes = (args.small_mib * MIB, args.large_mib * MIB)
    whole = codec.fill(torch.empty(sizes[1] + BS // 2 + max(A_SIZES), dtype=torch.uint8, device="cuda"), "zipf255")

    if args.trace:
        raw = sizes[1] + BS // 2
        s = Stream(codec, whole, raw)
        for _ in range(5):
            s.reset()
            codec.append(s.stream, s.length, s.offs, raw, BS, whole[raw:raw + 64 * KIB])
        torch.cuda.synchronize()
        print(f"stream {s.length} bytes, 64 KiB appended five times")
        codec.close()
        return

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"hufgpu_append: zipf255 in {BS >> 10} KiB blocks; median of {args.runs} warm runs [min, max]")
    say("(a) hufgpu_encode_sub of D ++ A; (b) hufgpu_encode of A alone, plus hufgpu_decode of one block when t > 0")
    out_a = torch.empty(codec.encode_bound(sizes[1] + BS + max(A_SIZES), BS), dtype=torch.uint8, device="cuda")
    offs_a = torch.empty(codec.block_count(sizes[1] + BS + max(A_SIZES), BS) + 1, dtype=torch.int64, device="cuda")
    sub_a = codec.new_sub_index(sizes[1] + BS + max(A_SIZES), BS)
    out_b = torch.empty(codec.encode_bound(max(A_SIZES), BS), dtype=torch.uint8, device="cuda")
    offs_b = torch.empty(codec.block_count(max(A_SIZES), BS) + 1, dtype=torch.int64, device="cuda")
    table = {}
    for t in (0, BS // 2):
        for size in sizes:
            raw = size + t
            s = Stream(codec, whole, raw)
            say()
            say(f"D = {size >> 20} MiB + {t >> 10} KiB ({s.nb} blocks, stream {s.length} bytes)")
            say(f"{'A':>8}  {'append':<30} {'append, both sub-indexes':<30} {'(a) encode_sub of all':<30} {'(b) encode A (+ decode 1)':<30} {'call - (b)':>10}")
            for la in A_SIZES:
                a = whole[raw:raw + la]
                res = {}

                def plain():
                    res["len"] = codec.append(s.stream, s.length, s.offs, raw, BS, a)[2]

                def with_subs():
                    n_out = C.c_uint64(0)
                    rc = codec.lib.hufgpu_append(codec._ctx, s.stream.data_ptr(), s.length, s.stream.numel(), s.offs.data_ptr(), raw,
                                                 BS, a.data_ptr(), la, s.sub.data_ptr(), s.new_sub.data_ptr(), 0, C.byref(n_out), None)
                    assert rc == 0, codec.lib.hufgpu_last_error(codec._ctx).decode()
                    res["len_sub"] = int(n_out.value)

                def whole_again():
                    res["len_a"] = codec.encode(whole[:raw + la], BS, out=out_a, offsets=offs_a, sub_index=sub_a)[2]

                def alone():
                    codec.encode(a, BS, out=out_b, offsets=offs_b)
                    if t:
                        codec.decode(s.stream, s.length, s.offs[s.keep:s.keep + 2], 1, s.last)

                t_a = stats(timed(whole_again, args.runs))
                s.reset()
                t_b = stats(timed(alone, args.runs))
                t_s = stats(timed(with_subs, args.runs, s.reset))
                t_p = stats(timed(plain, args.runs, s.reset))
                nb_new = codec.block_count(raw + la, BS)
                same = (res["len"] == res["len_a"] == res["len_sub"] and torch.equal(s.stream[:res["len"]], out_a[:res["len_a"]])
                        and torch.equal(s.offs[:nb_new + 1], offs_a[:nb_new + 1]))
                table[(t, size, la)] = (t_p, t_b)
                say(f"{la >> 10:6d} K  {fmt(t_p):<30} {fmt(t_s):<30} {fmt(t_a):<30} {fmt(t_b):<30} {t_p[0] - t_b[0]:7.3f} ms"
                    f"{'' if same else '   RESULTS DIFFER'}")
            del s
    say()
    say(f"without sub-indexes, {sizes[0] >> 20} MiB beside {sizes[1] >> 20} MiB (a difference inside the spread of the runs = no dependence on the stream's size):")
    for t in (0, BS // 2):
        for la in A_SIZES:
            p0, p1 = table[(t, sizes[0], la)][0], table[(t, sizes[1], la)][0]
            spread = max(p0[2] - p0[1], p1[2] - p1[1])
            say(f"  t = {t >> 10:2d} KiB, A = {la >> 10:6d} K: {fmt(p0)} | {fmt(p1)}  difference {p1[0] - p0[0]:+.3f} ms, spread {spread:.3f} ms"
                f"  {'inside' if abs(p1[0] - p0[0]) <= spread else 'OUTSIDE'}")
    codec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

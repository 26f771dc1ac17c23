"""What a sub-index costs to rebuild, against what it saves (GPU): hufgpu_sub_index_from_raw, hufgpu_decode_build_sub and
hufgpu_build_sub_index beside hufgpu_decode, hufgpu_decode_sub and hist_lanes_kernel (a kernel that only reads N).

    python tools/time_build_sub_index.py [--runs 7] [--mib 1024] [--kinds zipf255,uniform256,logtext]
                                         [--out profiles/sub_build/time_build_sub_index.txt]

1 GiB of zipf255, of uniform256 and of logtext (libhuffman_amd/datagen.py: the low-entropy one, under 100 distinct
bytes) in 64 KiB blocks, device-resident, all in one process.  The stream and its index are the encoder's; the encoder's
sub-index is kept only to check the built ones against (the whole buffers must be equal) and for hufgpu_decode_sub.
Every figure is the median of --runs warm runs with [min, max], taken with device events around the enqueued call
(hufgpu_build_sub_index is synchronous: the events see its kernels and the gaps between its slabs).  hist_lanes is stage 0
of a profiled hufgpu_encode.  The break-even lines are the issue's:
    from_raw         <  decode - decode_sub            (a stream decoded twice is ahead)
    decode_build_sub <= 1.05 * (decode + from_raw)
HUF_GPU_SUB_TABLE=1 in the environment times the 8-byte table reads instead of the byte reads (kernels/sub_build.hpp).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd import datagen  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402

BS = 65536
TILE = 16 << 20


def timed(fn, runs):
    fn()
    fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def fmt(s):
    return f"{s[0]:8.3f} ms [{s[1]:.3f}, {s[2]:.3f}]"


def workload(codec, kind, n):
    if kind in ("zipf255", "uniform256"):
        return codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), kind)
    host = datagen.GENERATORS[kind](min(n, TILE))
    return torch.from_numpy(host).cuda().repeat(-(-n // host.size))[:n].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kinds", default="zipf255,uniform256,logtext")
    args = ap.parse_args()
    n = args.mib << 20
    codec = GpuCodec(0)
    lib, ctx = codec.lib, codec._ctx
    nb = codec.block_count(n, BS)
    lines = [f"{args.mib} MiB in {BS >> 10} KiB blocks, median of {args.runs} warm runs [min, max]; table reads: "
             + ("8 bytes (HUF_GPU_SUB_TABLE=1)" if os.environ.get("HUF_GPU_SUB_TABLE") == "1" else "1 byte")]
    print(lines[0], flush=True)
    ok_all = True
    for kind in args.kinds.split(","):
        data = workload(codec, kind, n)
        esub = codec.new_sub_index(n, BS).zero_()
        stream, offs, length = codec.encode(data, BS, sub_index=esub)
        out = torch.empty(n, dtype=torch.uint8, device="cuda")
        sub = codec.new_sub_index(n, BS)
        sp, op, s = stream.data_ptr(), offs.data_ptr(), None

        def check(what):
            torch.cuda.synchronize()
            good = bool(torch.equal(sub, esub))
            sub.zero_()
            return "" if good else f"  {what}: the built sub-index DIFFERS from the encoder's"

        def f_decode():
            assert lib.hufgpu_decode(ctx, sp, length, op, nb, out.data_ptr(), n, 1, None, s) == 0

        def f_decode_sub():
            assert lib.hufgpu_decode_sub(ctx, sp, length, op, n, BS, esub.data_ptr(), out.data_ptr(), n, 1, None, s) == 0

        def f_from_raw():
            assert lib.hufgpu_sub_index_from_raw(ctx, sp, length, op, data.data_ptr(), n, BS, sub.data_ptr(), 1, None, s) == 0

        def f_decode_build():
            assert lib.hufgpu_decode_build_sub(ctx, sp, length, op, n, BS, out.data_ptr(), n, sub.data_ptr(), 1, None, None, s) == 0

        def f_stream_only():
            u = C.c_uint64(0)
            assert lib.hufgpu_build_sub_index(ctx, sp, length, op, n, BS, sub.data_ptr(), 1, C.byref(u), s) == 0 and u.value == 0

        sub.zero_()
        t_dec = timed(f_decode, args.runs)
        assert codec.decode_result() == n and torch.equal(out, data)
        t_sub = timed(f_decode_sub, args.runs)
        assert codec.decode_result() == n and torch.equal(out, data)
        t_raw = timed(f_from_raw, args.runs)
        bad = check("from_raw")
        t_both = timed(f_decode_build, args.runs)
        assert codec.decode_result() == n and torch.equal(out, data)
        bad += check("decode_build_sub")
        t_only = timed(f_stream_only, args.runs)
        bad += check("build_sub_index")
        codec.set_profiling(True)
        for _ in range(3):
            codec.encode(data, BS)
        prof, calls = codec.profile("encode")
        codec.set_profiling(False)
        t_hist = prof["hist256"] / calls

        margin = t_dec[0] - t_sub[0]
        limit = 1.05 * (t_dec[0] + t_raw[0])
        ok1, ok2 = t_raw[0] < margin, t_both[0] <= limit
        ok_all = ok_all and ok1 and ok2 and not bad
        block = [
            f"{kind}: stream {length / n:.3f} of the data",
            f"  hufgpu_decode              {fmt(t_dec)}",
            f"  hufgpu_decode_sub          {fmt(t_sub)}",
            f"  hist_lanes (reads N)       {t_hist:8.3f} ms (mean of {calls} profiled encodes)",
            f"  hufgpu_sub_index_from_raw  {fmt(t_raw)}",
            f"  hufgpu_decode_build_sub    {fmt(t_both)}",
            f"  hufgpu_build_sub_index     {fmt(t_only)}",
            f"  break-even: from_raw {t_raw[0]:.3f} < decode - decode_sub {margin:.3f}: {'yes' if ok1 else 'NO'}",
            f"  decode_build_sub {t_both[0]:.3f} <= 1.05 * (decode + from_raw) {limit:.3f}: {'yes' if ok2 else 'NO'}",
        ]
        if bad:
            block.append(bad)
        print("\n".join(block), flush=True)
        lines += block
        del data, esub, stream, offs, out, sub
        torch.cuda.empty_cache()
    lines.append("all break-even conditions hold" if ok_all else "NOT all break-even conditions hold")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    codec.close()


if __name__ == "__main__":
    main()

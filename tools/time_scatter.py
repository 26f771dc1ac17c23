"""hufgpu_scatter - records overwritten at positions that are on the device, enqueue-only - against what a caller with
positions on the device does without it: the positions copied to the host, overlapping matches merged there, and
hufgpu_update_ranges with its two waits (GPU).

    python tools/time_scatter.py [--runs 7] [--mib 1024] [--out profiles/update/time_scatter.txt]

Two device-resident inputs: log text in blocks of 1 MiB and zipf255 bytes in blocks of 64 KiB.  Alternating in one process,
median of --runs warm runs with [min, max].  Five rows an input, two or four columns a row:

  one record of 4 KiB; 4 096 records of 4 KiB at distinct places   new bytes from slots (source mode)
  about 7 000 and about 2 million matches of a pattern             HUFGPU_SCATTER_FILL
  the lines that hold the first pattern, up to 256 bytes each      HUFGPU_SCATTER_FILL

  (a) scatter        from positions (and lengths) already on the device to d_result read on the host
  (b) update_ranges  positions (and lengths) to the host, the ranges merged with numpy where matches overlap, the C call
                     with host arrays - its upload, its plan, its two waits
  (c) for the two pattern rows: find_pattern + (a) and find_pattern + (b), end to end

Both columns get the stream's own sub-index and write no new one.  Scatter runs with its default touched_cap, the bound.
The tool asserts that (a) and (b) write the same stream on every row, and - after every row is printed - that (a) is not
slower than (b) on any row.  The last line of an input is the device copy of its stream, the ceiling the untouched records
move at.

Every workload runs in a process of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import ctypes as C
import statistics
import time

import numpy as np
import torch

from find_timing import Workload, alternate, fmt, main

HEADER = ("{mib} MiB, median of {runs} warm runs [min, max], the columns of all rows alternating in one process per workload; "
          "(a) to d_result on the host, (b) to the call's return")
P64 = C.POINTER(C.c_uint64)
FILL = 0x2A
SCATTER_FILL = 0x100                                     # HUFGPU_SCATTER_FILL
LINE_BYTES = 256


def nearest(codec, args, candidates, goal):
    """the candidate whose count is nearest the goal: (pattern, count)"""
    counted = [(p, int(codec.count_pattern(*args, p)[0][0])) for p in candidates]
    return min((c for c in counted if c[1] > 0), key=lambda c: abs(np.log(c[1] / goal)))


def merged(lo, ln, n):
    """host ranges of records (start, length) in ascending order of start: cut at n, empty ones dropped, overlapping ones
    joined (ranges that touch stay apart) - what hufgpu_update_ranges asks of its caller"""
    lo = lo.astype(np.uint64)
    hi = np.minimum(lo + ln.astype(np.uint64), np.uint64(n))
    keep = hi > lo
    lo, hi = lo[keep], hi[keep]
    if lo.size == 0:
        return lo, hi
    run = np.maximum.accumulate(hi)
    first = np.concatenate([[True], lo[1:] >= run[:-1]])
    at = np.flatnonzero(first)
    return np.ascontiguousarray(lo[at]), np.ascontiguousarray(np.maximum.reduceat(hi, at))


def one_workload(k, runs, mib):
    load = Workload(k, mib)
    what, codec, n, bs = load.what, load.codec, load.n, load.bs
    lib = codec.lib
    if load.kind == "logtext":
        few_c, many_c = [load.rare()], [b"ERROR"]
    else:
        top = int(load.histogram().argmax())
        cut = lambda a, b: bytes(11 if v == 10 else v for v in load.data[a:b].cpu().tolist())     # noqa: E731 - no delimiter in it
        few_c = [cut(at, at + ln) for at in (1000, 5000, 9000) for ln in (3, 4, 5, 6)]
        many_c = [bytes([top]) * ln for ln in (2, 3, 4, 5)]
    args = load.encode()
    stream, length, offs, nb, sub = args[:5]
    few, few_n = nearest(codec, args, few_c, 7000)
    many, many_n = nearest(codec, args, many_c, 2_000_000)
    lines_n = int(codec.count_records(*args, few, delimiters=b"\n")[0][0])

    rng = np.random.default_rng(17)
    places = np.sort(rng.choice(n // 8192 - 1, 4096, replace=False).astype(np.int64) * 8192 + 123)
    slots = torch.from_numpy(rng.integers(0x20, 0x7F, (4096, 4096), dtype=np.uint8)).cuda()
    pos_few = codec.find_pattern(*args, few, max_positions=few_n)[0]
    pos_many = codec.find_pattern(*args, many, max_positions=many_n)[0]
    found = codec.find_records(*args, few, delimiters=b"\n", max_records=lines_n, max_len=LINE_BYTES)
    pos_lines, len_lines = found[0], found[1]
    # name, positions, lengths (int or tensor), max_len, slots or None, the pattern of column (c) or None
    rows = [("one record of 4 KiB", torch.from_numpy(places[2048:2049].copy()).cuda(), 4096, 4096, slots[:1], None),
            ("4 096 records of 4 KiB", torch.from_numpy(places).cuda(), 4096, 4096, slots, None),
            (f"{few_n} matches of {len(few)} bytes, fill", pos_few, len(few), len(few), None, (few, few_n)),
            (f"{many_n} matches of {len(many)} bytes, fill", pos_many, len(many), len(many), None, (many, many_n)),
            (f"{lines_n} lines, up to {LINE_BYTES} bytes, fill", pos_lines, len_lines, LINE_BYTES, None, None)]

    room = length + nb * codec.encode_bound(bs, 0) + 64             # the old length + every block at its bound: always enough
    out_a = torch.empty(room, dtype=torch.uint8, device="cuda")
    out_b = torch.empty(room, dtype=torch.uint8, device="cuda")
    idx_b = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    fill_src = torch.full((max(many_n * len(many), few_n * len(few), lines_n * LINE_BYTES, 1),), FILL, dtype=torch.uint8, device="cuda")

    idx_a = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    res_a = torch.empty(4, dtype=torch.int64, device="cuda")

    def scatter(pos, lens, max_len, data):
        """(a), through the C ABI as (b) is: returns (seconds, the four result words)"""
        t0 = time.perf_counter()
        nrec = pos.numel()
        cap = max(1, lib.hufgpu_scatter_touched_bound(nb, bs, nrec, max_len))
        rc = lib.hufgpu_scatter(codec._ctx, stream.data_ptr(), length, offs.data_ptr(), nb, sub.data_ptr(), n, bs, nrec, pos.data_ptr(),
                                lens.data_ptr() if isinstance(lens, torch.Tensor) else None, max_len,
                                data.data_ptr() if data is not None else None, data.stride(0) if data is not None else 0, FILL, cap,
                                out_a.data_ptr(), room, idx_a.data_ptr(), None, res_a.data_ptr(), 0 if data is not None else SCATTER_FILL,
                                codec._stream())
        assert rc == 0, f"hufgpu_scatter returned {rc}"
        words = res_a.cpu().tolist()
        return time.perf_counter() - t0, words

    def update(pos, lens, max_len, data):
        """(b): returns (seconds, (status, the new length, blocks encoded again))"""
        t0 = time.perf_counter()
        h_pos = pos.cpu().numpy()
        if data is not None:                                        # distinct places: range i's bytes are slot i
            lo = h_pos.astype(np.uint64)
            hi = lo + np.uint64(max_len)
            so = np.arange(lo.size, dtype=np.uint64) * np.uint64(data.stride(0))
            so_p, src = so.ctypes.data_as(P64), data
        else:
            h_len = lens.cpu().numpy() if isinstance(lens, torch.Tensor) else np.full(h_pos.size, lens, np.int64)
            lo, hi = merged(h_pos, h_len, n)
            so_p, src = None, fill_src
        out_len, count = C.c_uint64(0), C.c_uint64(0)
        rc = lib.hufgpu_update_ranges(codec._ctx, stream.data_ptr(), length, offs.data_ptr(), nb, lo.size, lo.ctypes.data_as(P64),
                                      hi.ctypes.data_as(P64), so_p, src.data_ptr(), sub.data_ptr(), n, bs, out_b.data_ptr(), room,
                                      idx_b.data_ptr(), None, 0, C.byref(out_len), C.byref(count), codec._stream())
        return time.perf_counter() - t0, (int(rc), int(out_len.value), int(count.value))

    def found_then(call, pattern, count, buf, lens, max_len):
        def run():
            t0 = time.perf_counter()
            pos = codec.find_pattern(*args, pattern, max_positions=count, out=buf)[0]
            _, answer = call(pos, lens, max_len, None)
            return time.perf_counter() - t0, answer
        return run

    calls = []
    for name, pos, lens, max_len, data, pat in rows:
        calls += [((name, "(a) scatter"), lambda p=pos, ln=lens, m=max_len, d=data: scatter(p, ln, m, d)),
                  ((name, "(b) update_ranges"), lambda p=pos, ln=lens, m=max_len, d=data: update(p, ln, m, d))]
        if pat is not None:
            buf = torch.empty(pat[1], dtype=torch.int64, device="cuda")
            calls += [((name, "(c) find + (a)"), found_then(scatter, pat[0], pat[1], buf, lens, max_len)),
                      ((name, "(c) find + (b)"), found_then(update, pat[0], pat[1], buf, lens, max_len))]

    # warm, and the answers: the same stream from both columns on every row
    for name, *_ in rows:
        for tail in (("(a) scatter", "(b) update_ranges"), ("(c) find + (a)", "(c) find + (b)")):
            pair = [run for key, run in calls if key[0] == name and key[1] in tail]
            if not pair:
                continue
            (_, words), (_, (rc, b_len, b_count)) = pair[0](), pair[1]()
            assert words[0] == 0 and rc == 0, f"{name}: scatter's status {words[0]}, update_ranges' {rc}"
            assert words[1] == b_len, f"{name}: scatter writes {words[1]} bytes, update_ranges {b_len}"
            assert torch.equal(out_a[:b_len], out_b[:b_len]), f"{name}: the two streams differ"
            if tail[0].startswith("(a)"):
                print(f"{what:26s} {name:44s} {words[2]:6d} blocks touched of {nb}, new stream {b_len} bytes (old {length})", flush=True)

    times = dict(zip([key for key, _ in calls], alternate(runs, *[lambda run=run: run()[0] for _, run in calls])))
    med = {key: statistics.median(ts) for key, ts in times.items()}
    for key, _ in calls:
        print(f"{what:26s} {key[0]:44s} {key[1]:20s} {fmt(times[key])}", flush=True)
    slower = []
    for name, *_ in rows:
        for a, b in (("(a) scatter", "(b) update_ranges"), ("(c) find + (a)", "(c) find + (b)")):
            if (name, a) in med:
                ratio = med[name, b] / med[name, a]
                print(f"{what:26s} {name:44s} {b} / {a}: {ratio:.2f}x", flush=True)
                if ratio < 1.0:
                    slower.append(f"{name}: {a} {med[name, a] * 1e3:.3f} ms, {b} {med[name, b] * 1e3:.3f} ms")

    def copy():
        t0 = time.perf_counter()
        out_a[:length].copy_(stream[:length])
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    ts = alternate(runs, copy)[0]
    print(f"{what:26s} {'device copy of the stream':44s} {'':20s} {fmt(ts)}  {2 * length / statistics.median(ts) / 1e12:.2f} TB/s read + write",
          flush=True)
    codec.close()
    assert not slower, "scatter is slower than positions to the host + update_ranges: " + "; ".join(slower)


if __name__ == "__main__":
    main(__file__, HEADER, one_workload)

"""What the timing tools of the search family (tools/time_find*.py) share: the two workloads and their set-up, the patterns
they draw from the data, the loop that alternates the calls, the figures' format, and the command line with one child
process per workload.  Each tool keeps its cases, its recipe, its assertions and its print format."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libhuffman_amd import datagen  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402

WORKLOADS = [("logtext, blocks of 1 MiB", "logtext", 1 << 20), ("zipf255, blocks of 64 KiB", "zipf255", 65536)]
STEP_SECONDS = 420


def fmt(ts, width=8):
    return f"{statistics.median(ts) * 1e3:{width}.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]"


class Workload:
    """workload k at `mib` MiB: `data` on the device, not yet encoded - the tool may plant its strings first; `page` is the
    host copy of the log text's 16 MiB tile"""

    def __init__(self, k, mib):
        self.what, self.kind, self.bs = WORKLOADS[k]
        self.codec = GpuCodec(0)
        self.n = n = mib << 20
        self.page = None
        if self.kind == "logtext":
            tile = min(n, 16 << 20)
            self.page = datagen.logtext(tile)
            self.data = torch.from_numpy(self.page).cuda().repeat(n // tile)
        else:
            self.data = self.codec.fill(torch.empty(n, dtype=torch.uint8, device="cuda"), self.kind)

    def histogram(self):
        return torch.bincount(self.data[:1 << 24].int(), minlength=256)

    def frequent(self, delimiter=None):
        """the word ERROR; five times zipf255's most frequent value (`delimiter`: but not this one - a pattern holds none)"""
        if self.kind == "logtext":
            return b"ERROR"
        hist = self.histogram()
        if delimiter is not None:
            hist[delimiter] = 0
        return bytes([int(hist.argmax())]) * 5

    def absent(self, frequent):
        """a string that does not occur but shares four bytes with the frequent one"""
        return frequent[:4] + (b"\xff" if self.kind == "zipf255" else b"\x00")

    def rare(self):
        """the time stamp of the log's first line (12:MM:SS.mmm); four bytes taken from the zipf255 data"""
        if self.kind == "logtext":
            return bytes(self.page[11:23])
        return bytes(11 if v == 10 else v for v in self.data[1000:1004].cpu().tolist())

    def plant(self):
        """a string of 36 bytes at five places, four of them across block seams; returns (the string, the places)"""
        n, bs = self.n, self.bs
        planted = bytes(np.random.default_rng(36).integers(128, 255, 36).astype(np.uint8))
        places = [n // 2 + 12345] + [(j * (n // bs // 5) + 1) * bs - d for j, d in zip(range(1, 5), (1, 18, 35, 7))]
        for p in places:
            self.data[p:p + 36] = torch.frombuffer(bytearray(planted), dtype=torch.uint8).cuda()
        return planted, places

    def encode(self):
        """encodes with a sub-index and lets go of the data; returns the arguments every search call starts with"""
        codec, n, bs = self.codec, self.n, self.bs
        sub = codec.new_sub_index(n, bs)
        stream, offs, length = codec.encode(self.data, bs, sub_index=sub)
        self.data = None
        return (stream, length, offs, codec.block_count(n, bs), sub, n, bs)


def alternate(runs, *calls):
    """`runs` rounds of the calls one after the other, a synchronize in front of each; a call returns its seconds.  Returns one
    list of times per call"""
    times = [[] for _ in calls]
    for _ in range(runs):
        for ts, f in zip(times, calls):
            torch.cuda.synchronize()
            ts.append(f())
    return times


def main(tool, header, one_workload):
    """the command line of the tool in the file `tool`: every workload in a child process under `timeout -k 10`, the first
    that fails ends the run; `header` is the first line behind the tool's name, with {mib} and {runs}"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default="")
    ap.add_argument("--workload", type=int, default=-1, help="run this workload only, in this process")
    a = ap.parse_args()
    if a.workload >= 0:
        one_workload(a.workload, a.runs, a.mib)
        return
    lines = [f"{os.path.basename(tool)}: " + header.format(mib=a.mib, runs=a.runs)]
    print(lines[0], flush=True)
    ok = True
    for k in range(len(WORKLOADS)):
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(tool), "--workload", str(k),
                            "--runs", str(a.runs), "--mib", str(a.mib)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += p.stdout.splitlines()
        if p.returncode != 0:
            lines.append(f"workload {k} ended with status {p.returncode}: nothing further is run")
            print(lines[-1], flush=True)
            ok = False
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)

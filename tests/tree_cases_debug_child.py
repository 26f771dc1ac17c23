"""Child of test_gpu_tree_cases.py: runs with HUF_LIB_PATH = the -DTREE_DEBUG build and prints, for every case of
tree_cases.py, one JSON line: tree.hpp's counters (g_tree_dbg, in the slot order of tree_rounds_ref.EVENTS) after encoding
the case's block alone on the tree_wave_kernel route and, where a block of that route holds it, on the fused route, and
whether both streams were the oracle's."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import tree_cases  # noqa: E402
from tree_cases import FUSED_BELOW, fused_bs, lanes_bs  # noqa: E402
import tree_rounds_ref as M  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

assert os.environ.get("HUF_LIB_PATH"), "needs the debug build"
codec = GpuCodec(0)
L = codec.lib
L.hufgpu_debug_tree.argtypes = [C.c_void_p, C.c_int]
oracle = Oracle()
counters = (C.c_ulonglong * len(M.EVENTS))()


def run(data, bs):
    d = torch.from_numpy(data).cuda()
    assert L.hufgpu_debug_tree(counters, 1) == 0
    stream, offs, length = codec.encode(d, bs)
    torch.cuda.synchronize()
    assert L.hufgpu_debug_tree(counters, 0) == 0
    want, want_offs = oracle.encode(data, bs, with_offsets=True)
    equal = np.array_equal(stream.cpu().numpy(), want) and np.array_equal(offs.cpu().numpy().astype(np.uint64), want_offs)
    return list(counters), bool(equal)


for c in tree_cases.cases():
    data = c.data()
    # (a large case with blocksize 0: lane-private or chunk counts by its size, tree_wave_kernel behind both)
    cnt, equal = run(data, 0 if c.large else lanes_bs(c.n))
    row = {"case": c.name, "counters": {"tree_wave": cnt}, "equal": equal}
    if fused_bs(c.n) < FUSED_BELOW:
        cnt, equal = run(data, fused_bs(c.n))
        row["counters"]["fused"] = cnt
        row["equal"] = row["equal"] and equal
    print(json.dumps(row), flush=True)
codec.close()
print("done")

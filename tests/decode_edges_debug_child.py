"""Child of test_gpu_decode_edges.py: runs with HUF_LIB_PATH = the -DDFAST_DEBUG build and prints, for every case of
decode_edge_cases.py that names its branch, one JSON line: the entry point, the branch it should take and decode_regs.hpp's
counters (g_dfast_dbg[16:32], and [0:4]) after decoding the case's probe blocks alone through that entry point."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import decode_edge_cases as dec  # noqa: E402
from libhuffman_amd import datagen  # noqa: E402
from libhuffman_amd.codec import GpuCodec  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

assert os.environ.get("HUF_LIB_PATH"), "needs the debug build"
codec = GpuCodec(0)
L = codec.lib
L.hufgpu_debug_dfast.argtypes = [C.c_void_p, C.c_int]
vp, u64 = C.c_void_p, C.c_uint64
L.hufgpu_decode_small.argtypes = [vp, vp, u64, u64, C.c_uint32, vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
oracle = Oracle()
counters = (C.c_ulonglong * 32)()


def run(entry, parts, syms):
    st = np.concatenate([np.frombuffer(bytes(p), dtype=np.uint8) for p in parts])
    n = syms.size
    s = torch.from_numpy(st).cuda()
    out = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    assert L.hufgpu_debug_dfast(counters, 1) == 0
    if entry == "indexed":
        offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        ok = codec.decode(s, st.size, torch.from_numpy(offs).cuda(), len(parts), out[1:1 + n], relaxed=True) == n
    elif entry == "probe":
        assert st.size >= dec.RAW_PARALLEL_MIN
        ok = codec.decode_stream(s, st.size, st.size, out[1:1 + n], relaxed=True) == (0, n, st.size)
    else:
        h_in = torch.from_numpy(st.copy()).pin_memory()
        h_out = torch.zeros(((n + 7) & ~7) + 64, dtype=torch.uint8).pin_memory()
        raw, used = C.c_uint64(), C.c_uint64()
        err = L.hufgpu_decode_small(codec._ctx, h_in.data_ptr(), st.size, st.size, 1, s.data_ptr(), out[1:].data_ptr(), n,
                                    h_out.data_ptr(), h_out.numel(), C.byref(raw), C.byref(used))
        ok = (err, raw.value, used.value) == (0, n, st.size)
    torch.cuda.synchronize()
    assert L.hufgpu_debug_dfast(counters, 0) == 0
    equal = bool(ok) and np.array_equal(out[1:1 + n].cpu().numpy(), syms)
    return list(counters), equal


def syms_of(parts):
    st = np.concatenate([np.frombuffer(bytes(p), dtype=np.uint8) for p in parts])
    err, out, _ = oracle.decode(st, 8 * st.size + 64, 1025)
    assert err == 0
    return out


probes = []
for c in dec.cases(oracle):
    if c.probe:
        probes.append((c.name, c.probe))
    probes += [(label, (parts, wants)) for label, parts, wants in c.more_probes]
for extra in (0, 1):                    # F: DREG_MAX_BLOCK
    n = dec.DREG_MAX_BLOCK + extra
    st = oracle.encode(datagen.zipf255(n, seed=26), 0)
    probes.append(("F_2^26" + ("+1" if extra else ""), ([st], {"indexed": "declined" if extra else "taken"})))
for name, (parts, wants) in probes:
    syms = syms_of(parts)
    for entry, want in wants.items():
        cnt, equal = run(entry, parts, syms)
        # (counters 0-3: why a lean pass gave up - input exhausted, rounds, a lane's codewords, no progress)
        print(json.dumps({"case": name, "entry": entry, "want": want, "counters": cnt[16:32], "gave_up": cnt[0:4], "equal": equal}), flush=True)
codec.close()
print("done")

"""NumPy model of hufgpu_find_bytes (include/huffman_gpu.h): what the call reports for an input, a set of byte values, a
layout, the blocks that are served and a cap on the positions.  Shared by tests/test_find_args.py (which checks the model
itself) and tests/test_gpu_find.py (which checks the GPU against it)."""
import numpy as np


def byte_set(values):
    """the 32 bytes of the `set` argument: bit v & 7 of byte v >> 3"""
    s = bytearray(32)
    for v in values:
        s[int(v) >> 3] |= 1 << (int(v) & 7)
    return bytes(s)


def block_lens(n, blocksize):
    bs = blocksize or n
    return [min(bs, n - o) for o in range(0, n, bs)] if n else []


def find_model(data, values, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block).  served: per block,
    False = the block is reported not served and contributes nothing (default: all served)."""
    data = np.asarray(data, dtype=np.uint8)
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    hit = np.isin(data, np.asarray(sorted(set(int(v) for v in values)), dtype=np.uint8)) if n else np.zeros(0, bool)
    if nb:
        hit &= np.repeat(served, bs)[:n]
    pos = np.flatnonzero(hit).astype(np.int64)
    counts = np.add.reduceat(hit.astype(np.int64), np.arange(0, n, bs)) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts.astype(np.int64), totals

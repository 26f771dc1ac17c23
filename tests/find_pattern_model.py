"""NumPy model of hufgpu_find_pattern (include/huffman_gpu.h): what the call reports for an input, a pattern of bytes, a
layout, the blocks that are served and a cap on the positions.  Shared by tests/test_find_pattern_args.py (which checks
the model itself against a plain bytes.find loop) and tests/test_gpu_find_pattern.py (which checks the GPU against it)."""
import numpy as np

from find_model import block_lens


def find_pattern_model(data, pattern, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block).  A match is a
    start p with data[p:p + len(pattern)] == pattern, overlapping ones included; it counts for the block of p and only
    when every block it touches is served (served: per block, default all)."""
    data = np.asarray(data, dtype=np.uint8)
    pat = np.frombuffer(bytes(pattern), dtype=np.uint8)
    n, m = int(data.size), int(pat.size)
    assert m >= 1
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    nstarts = max(n - m + 1, 0)
    hit = np.ones(nstarts, bool)
    for k in range(m):                                  # (m <= 64 passes over the data)
        hit &= data[k:k + nstarts] == pat[k]
    if nstarts:
        # blocks [first, last] of a start are all served: no block that is not served among them
        bad = np.concatenate([[0], np.cumsum(~served)])
        p = np.arange(nstarts)
        hit &= bad[(p + m - 1) // bs + 1] == bad[p // bs]
    pos = np.flatnonzero(hit).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals

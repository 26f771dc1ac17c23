"""NumPy models of hufgpu_find_classes and hufgpu_find_records_classes (include/huffman_gpu.h): what the calls report for
an input, a pattern whose every position is a set of byte values, a layout, the blocks that are served and the caps.  The
served rules are those of the literal models (tests/find_pattern_model.py, tests/find_records_model.py).  Shared by
tests/test_find_classes_args.py (which checks the models against Python's `re`) and tests/test_gpu_find_classes.py (which
checks the GPU against them)."""
import numpy as np

from find_model import block_lens
from find_records_model import delimiter_values


def class_table(classes):
    """bool [len][256]: value v may stand at position k.  `classes` is uint8 [len][32] in hufgpu_find_bytes()' encoding (what
    GpuCodec.byte_classes returns) or a sequence with an int, a `bytes` or an iterable of ints a position."""
    if isinstance(classes, np.ndarray) and classes.ndim == 2 and classes.shape[1] == 32:
        return np.unpackbits(classes.astype(np.uint8), axis=1, bitorder="little").astype(bool)
    if isinstance(classes, (bytes, bytearray)):
        classes = list(bytes(classes))
    table = np.zeros((len(classes), 256), bool)
    for k, c in enumerate(classes):
        values = [c] if isinstance(c, (int, np.integer)) else list(bytes(c)) if isinstance(c, (bytes, bytearray)) else [int(v) for v in c]
        table[k, values] = True
    return table


def class_hits(data, table):
    """bool [max(n - len + 1, 0)]: the starts p with data[p + k] in class k for every k"""
    n, m = int(data.size), int(table.shape[0])
    nstarts = max(n - m + 1, 0)
    hit = np.ones(nstarts, bool)
    for k in range(m):                                  # (m <= 64 passes over the data)
        hit &= table[k][data[k:k + nstarts]]
    return hit


def find_classes_model(data, classes, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block).  A match is a
    start p with data[p + k] in classes[k] for every k, overlapping ones included; it counts for the block of p and only
    when every block it touches is served (served: per block, default all)."""
    data = np.asarray(data, dtype=np.uint8)
    table = class_table(classes)
    n, m = int(data.size), int(table.shape[0])
    assert 1 <= m <= 64 and table.any(axis=1).all(), "1 to 64 classes, none empty"
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    hit = class_hits(data, table)
    if hit.size:
        bad = np.concatenate([[0], np.cumsum(~served)])
        p = np.arange(hit.size)
        hit &= bad[(p + m - 1) // bs + 1] == bad[p // bs]
    pos = np.flatnonzero(hit).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals


def find_class_records_model(data, classes, delims, blocksize, cap=0, max_len=0, served=None):
    """(starts written, lengths written, block counts, totals[4]) as find_records_model gives them, for the records that
    hold a match of the class pattern.  No class holds a delimiter."""
    data = np.asarray(data, dtype=np.uint8)
    table = class_table(classes)
    values = delimiter_values(delims)
    n, m = int(data.size), int(table.shape[0])
    assert 1 <= m <= 64 and table.any(axis=1).all(), "1 to 64 classes, none empty"
    assert not table[:, values].any(), "a class holds no delimiter"
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    clip = int(max_len) or 2**32 - 1
    hit = class_hits(data, table)
    dpos = np.flatnonzero(np.isin(data, np.asarray(values, dtype=np.uint8))).astype(np.int64)
    starts = np.concatenate([[0], dpos + 1]).astype(np.int64)
    ends = np.concatenate([dpos, [n]]).astype(np.int64)
    rec = np.unique(np.searchsorted(dpos, np.flatnonzero(hit)))
    s, e = starts[rec], ends[rec]
    if nb:
        bad = np.concatenate([[0], np.cumsum(~served)])
        keep = bad[np.minimum(e, n - 1) // bs + 1] == bad[np.maximum(s - 1, 0) // bs]
        s, e = s[keep], e[keep]
    counts = np.bincount(s // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(s.size)
    written = min(total, int(cap))
    lens = np.minimum(e - s, clip)
    totals = np.array([total, written, int(nb - served.sum()), int(np.count_nonzero((e - s)[:written] > clip))], dtype=np.int64)
    return s[:written], lens[:written], counts, totals

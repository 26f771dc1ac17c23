"""NumPy models of hufgpu_find_any and hufgpu_find_records_any (include/huffman_gpu.h): what the calls report for an input,
a list of ALTERNATIVES - each a pattern whose every position is a set of byte values -, a layout, the blocks that are served
and the caps.  A start is a match when at least one alternative lies there, each alternative with its own served rule (every
block that ITS bytes touch is served); the bookkeeping behind that is tests/find_classes_model.py's.  Shared by
tests/test_find_any_args.py (which checks the models against Python's `re`) and tests/test_gpu_find_any.py (which checks the
GPU against them)."""
import numpy as np

from find_classes_model import class_hits, class_table
from find_model import block_lens
from find_records_model import delimiter_values


def alt_tables(alternatives):
    """the bool [len_j][256] table of every alternative; `alternatives` is a sequence of what class_table takes"""
    tables = [class_table(a) for a in alternatives]
    assert 1 <= len(tables) <= 64, "1 to 64 alternatives"
    assert all(t.shape[0] >= 1 and t.any(axis=1).all() for t in tables), "no alternative of length 0, no empty class"
    assert sum(t.shape[0] for t in tables) <= 64, "the lengths sum to at most 64"
    return tables


def any_hits(data, tables, bs=None, served=None):
    """bool [n]: the starts at which at least one alternative lies (and, with `served`, touches served blocks only)"""
    n = int(data.size)
    hit = np.zeros(n, bool)
    bad = None if served is None else np.concatenate([[0], np.cumsum(~served)])
    for table in tables:
        m = int(table.shape[0])
        h = class_hits(data, table)
        if h.size and bad is not None:
            p = np.arange(h.size)
            h &= bad[(p + m - 1) // bs + 1] == bad[p // bs]
        hit[:h.size] |= h
    return hit


def find_any_model(data, alternatives, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block).  A start counts
    ONCE however many alternatives lie there, for the block of the start."""
    data = np.asarray(data, dtype=np.uint8)
    tables = alt_tables(alternatives)
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    pos = np.flatnonzero(any_hits(data, tables, bs, served)).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals


def find_any_records_model(data, alternatives, delims, blocksize, cap=0, max_len=0, served=None):
    """(starts written, lengths written, block counts, totals[4]) as find_records_model gives them, for the records that
    hold a match of any alternative, each record once.  No class of any alternative holds a delimiter."""
    data = np.asarray(data, dtype=np.uint8)
    tables = alt_tables(alternatives)
    values = delimiter_values(delims)
    assert not any(t[:, values].any() for t in tables), "a class holds no delimiter"
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    clip = int(max_len) or 2**32 - 1
    hit = any_hits(data, tables)                        # (a record's own rule decides: every block of its extent is served)
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

"""NumPy model of hufgpu_find_records_select (include/huffman_gpu.h): what the call reports for an input, a list of
alternatives, a set of delimiters, a layout, the blocks that are served, the caps, `invert` and the numbers.  Built on
tests/find_any_model.py (the match starts) and tests/find_records_model.py (the records and the known-extent rule).  Shared by
tests/test_find_select_args.py (which checks the model against `re` / split over `bytes`) and tests/test_gpu_find_select.py
(which checks the GPU against it)."""
import numpy as np

from find_any_model import alt_tables, any_hits
from find_model import block_lens
from find_records_model import delimiter_values

NO_UNKNOWN = -1             # HUFGPU_REC_NO_UNKNOWN, read as int64


def all_records(data, delims):
    """(starts, ends) of every record of the data, the empty ones included; a delimiter as the last byte starts no record"""
    data = np.asarray(data, dtype=np.uint8)
    n = int(data.size)
    dpos = np.flatnonzero(np.isin(data, np.asarray(delimiter_values(delims), dtype=np.uint8))).astype(np.int64)
    starts = np.concatenate([[0], dpos + 1]).astype(np.int64)
    ends = np.concatenate([dpos, [n]]).astype(np.int64)
    keep = starts < n if n else np.zeros(starts.size, bool)
    return starts[keep], ends[keep]


def known_records(s, e, n, bs, served):
    """bool per record: every block that holds a byte of [max(s - 1, 0), min(e, n - 1)] is served"""
    bad = np.concatenate([[0], np.cumsum(~served)])
    return bad[np.minimum(e, n - 1) // bs + 1] == bad[np.maximum(s - 1, 0) // bs]


def find_select_model(data, alternatives, delims, blocksize, cap=0, max_len=0, served=None, invert=False):
    """(starts written, lengths written, block counts, totals[4], numbers written) for `data` in blocks of `blocksize` (0: one
    block).  Plain: the known records that hold a match of any alternative, as find_any_records_model gives them.  `invert`:
    the known NON-EMPTY records that hold none.  numbers[i] is the count of delimiter bytes in [0, starts[i]) when every
    block in front of the start's block is served, NO_UNKNOWN otherwise."""
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
    s, e = all_records(data, delims)
    if nb:
        hits = np.concatenate([[0], np.cumsum(any_hits(data, tables))])
        has = hits[e] > hits[s]                             # (no class holds a delimiter: a match that starts in a record lies in it)
        keep = known_records(s, e, n, bs, served) & ((~has & (e > s)) if invert else has)
        s, e = s[keep], e[keep]
        delims_before = np.concatenate([[0], np.cumsum(np.isin(data, np.asarray(values, dtype=np.uint8)))])
        first_bad = int(np.flatnonzero(~served)[0]) if not served.all() else nb
        numbers = np.where(s // bs <= first_bad, delims_before[s], NO_UNKNOWN).astype(np.int64)
    else:
        s, e, numbers = s[:0], e[:0], np.zeros(0, np.int64)
    counts = np.bincount(s // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(s.size)
    written = min(total, int(cap))
    lens = np.minimum(e - s, clip)
    totals = np.array([total, written, int(nb - served.sum()), int(np.count_nonzero((e - s)[:written] > clip))], dtype=np.int64)
    return s[:written], lens[:written], counts, totals, numbers[:written]

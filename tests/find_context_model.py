"""NumPy model of hufgpu_find_records_context (include/huffman_gpu.h): what the call reports for an input, a list of
alternatives, a set of delimiters, a layout, the blocks that are served, the caps, `invert` and the two distances.  Built on
tests/find_select_model.py: S is what that model selects, a record's number is its index among ALL records, the empty ones
included, and a record of known extent that is not empty is reported when it is in S or when the nearest record of S in front
of it is at most `after` records away, or the nearest one behind it at most `before`, with every block between the two served.
(Only the nearest one matters on either side: a farther one spans the blocks the nearer one spans.)  Shared by
tests/test_find_context_args.py (which checks the model against plain Python) and tests/test_gpu_find_context.py (which checks
the GPU against it)."""
import numpy as np

from find_any_model import alt_tables, any_hits
from find_model import block_lens
from find_records_model import delimiter_values
from find_select_model import NO_UNKNOWN, all_records, known_records


def find_context_model(data, alternatives, delims, blocksize, cap=0, max_len=0, served=None, invert=False, before=0, after=0):
    """(starts written, lengths written, block counts, totals[4], numbers written, flags written) for `data` in blocks of
    `blocksize` (0: one block).  flags[i] is 1 when record i is one of S - what find_select_model reports - and 0 when it is
    there as context only; numbers as find_select_model gives them."""
    data = np.asarray(data, dtype=np.uint8)
    tables = alt_tables(alternatives)
    values = delimiter_values(delims)
    assert not any(t[:, values].any() for t in tables), "a class holds no delimiter"
    assert 0 <= before < 2**32 and 0 <= after < 2**32
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    clip = int(max_len) or 2**32 - 1
    s, e = all_records(data, delims)                        # record k has number k
    if nb:
        hits = np.concatenate([[0], np.cumsum(any_hits(data, tables))])
        has = hits[e] > hits[s]
        cand = known_records(s, e, n, bs, served) & (e > s)
        sel = cand & (~has if invert else has)
        bad = np.concatenate([[0], np.cumsum(~served)])     # blocks that are not served in front of block b
        at = np.flatnonzero(sel)
        no = np.arange(s.size)
        report = sel.copy()
        if at.size:
            p = np.searchsorted(at, no, side="right") - 1   # the nearest record of S at or in front of record k, -1: none
            m = at[np.maximum(p, 0)]
            report |= cand & (p >= 0) & (no - m <= after) & (bad[np.minimum(e, n - 1) // bs + 1] == bad[s[m] // bs])
            q = np.searchsorted(at, no, side="left")        # ... and at or behind it, at.size: none
            m = at[np.minimum(q, at.size - 1)]
            report |= cand & (q < at.size) & (m - no <= before) & (bad[np.minimum(e[m], n - 1) // bs + 1] == bad[s // bs])
        flags = sel[report].astype(np.uint8)
        s, e = s[report], e[report]
        delims_before = np.concatenate([[0], np.cumsum(np.isin(data, np.asarray(values, dtype=np.uint8)))])
        first_bad = int(np.flatnonzero(~served)[0]) if not served.all() else nb
        numbers = np.where(s // bs <= first_bad, delims_before[s], NO_UNKNOWN).astype(np.int64)
    else:
        s, e, numbers, flags = s[:0], e[:0], np.zeros(0, np.int64), np.zeros(0, np.uint8)
    counts = np.bincount(s // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(s.size)
    written = min(total, int(cap))
    lens = np.minimum(e - s, clip)
    totals = np.array([total, written, int(nb - served.sum()), int(np.count_nonzero((e - s)[:written] > clip))], dtype=np.int64)
    return s[:written], lens[:written], counts, totals, numbers[:written], flags[:written]

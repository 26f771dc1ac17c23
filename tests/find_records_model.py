"""NumPy model of hufgpu_find_records (include/huffman_gpu.h): what the call reports for an input, a pattern, a set of
delimiters, a layout, the blocks that are served, a cap on the records and a cap on their lengths.  Shared by
tests/test_find_records_args.py (which checks the model itself against a plain split / find loop over `bytes`) and
tests/test_gpu_find_records.py (which checks the GPU against it)."""
import numpy as np

from find_model import block_lens


def delimiter_values(delims):
    return sorted(set(int(v) for v in (bytes(delims) if isinstance(delims, (bytes, bytearray)) else delims)))


def find_records_model(data, pattern, delims, blocksize, cap=0, max_len=0, served=None):
    """(starts written, lengths written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block).  The
    bytes with a value in `delims` cut the data into records [s, e); a record that holds the pattern is reported once,
    by the block of s, and only when it is KNOWN: every block that holds a byte of [max(s - 1, 0), min(e, n - 1)] is
    served (served: per block, default all).  Lengths are cut at max_len (0: at 2^32 - 1); totals = matching records,
    records written, blocks not served, written records longer than the cut."""
    data = np.asarray(data, dtype=np.uint8)
    pat = np.frombuffer(bytes(pattern), dtype=np.uint8)
    values = delimiter_values(delims)
    n, m = int(data.size), int(pat.size)
    assert m >= 1 and not set(pat.tolist()) & set(values), "a pattern holds no delimiter"
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    clip = int(max_len) or 2**32 - 1
    nstarts = max(n - m + 1, 0)
    hit = np.ones(nstarts, bool)
    for k in range(m):
        hit &= data[k:k + nstarts] == pat[k]
    dpos = np.flatnonzero(np.isin(data, np.asarray(values, dtype=np.uint8))).astype(np.int64)
    # record r is [starts[r], ends[r]); a match at p lies in record (delimiters in front of p), all of it: no byte of it is one
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

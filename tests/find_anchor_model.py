"""NumPy models of hufgpu_find_any_anchored and hufgpu_find_records_anchored (include/huffman_gpu.h): what the calls report
for an input, a list of alternatives, the delimiters D, the word bytes W, the anchors, a layout, the blocks that are served and
the caps.  Built on tests/find_any_model.py (the alternatives' tables and the occurrences) and tests/find_context_model.py (the
records call is that model with "holds a match" read as "holds a qualifying occurrence").  An occurrence (p, j) qualifies when
every anchor holds for its neighbours L = data[p - 1] and R = data[p + len_j] - an absent neighbour never stands in the way -,
and counts when every block of its tested span is served: [p, p + len_j) widened by the neighbours that exist and are tested.
Shared by tests/test_find_anchor_args.py (which checks the models against Python's `re`) and tests/test_gpu_find_anchors.py
(which checks the GPU against them)."""
import numpy as np

from find_any_model import alt_tables
from find_classes_model import class_hits
from find_model import block_lens
from find_records_model import delimiter_values
from find_select_model import NO_UNKNOWN, all_records, known_records

BOL, EOL, WORD = 1, 2, 4        # HUFGPU_ANCHOR_*


def budget_ok(alternatives, anchors):
    """do the alternatives fit the matcher's 64 bits: EOL and WORD take one more an alternative"""
    lens = [len(a) for a in alternatives]
    return sum(lens) + (len(lens) if anchors & (EOL | WORD) else 0) <= 64


def anchored_hits(data, tables, delims, words, anchors, bs=None, served=None):
    """bool [n]: the starts at which at least one alternative lies and qualifies (and, with `served`, has its tested span in
    served blocks only)"""
    n = int(data.size)
    assert 0 <= anchors < 8
    in_d = np.isin(data, np.asarray(delimiter_values(delims), dtype=np.uint8)) if anchors & (BOL | EOL) else np.zeros(n, bool)
    in_w = np.isin(data, np.asarray(delimiter_values(words), dtype=np.uint8)) if anchors & WORD else np.zeros(n, bool)
    hit = np.zeros(n, bool)
    bad = None if served is None else np.concatenate([[0], np.cumsum(~served)])
    for table in tables:
        m = int(table.shape[0])
        h = class_hits(data, table)
        if not h.size:
            continue
        p = np.arange(h.size)
        has_l, has_r = p > 0, p + m < n
        left, right = np.maximum(p - 1, 0), np.minimum(p + m, n - 1)
        if anchors & BOL:
            h &= ~has_l | in_d[left]
        if anchors & EOL:
            h &= ~has_r | in_d[right]
        if anchors & WORD:
            h &= (~has_l | ~in_w[left]) & (~has_r | ~in_w[right])
        if bad is not None:
            lo = np.where(has_l & bool(anchors & (BOL | WORD)), p - 1, p)
            hi = np.where(has_r & bool(anchors & (EOL | WORD)), p + m, p + m - 1)
            h &= bad[hi // bs + 1] == bad[lo // bs]
        hit[:h.size] |= h
    return hit


def find_any_anchored_model(data, alternatives, delims, words, anchors, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) as find_any_model gives them, for the qualifying occurrences"""
    data = np.asarray(data, dtype=np.uint8)
    tables = alt_tables(alternatives)
    assert budget_ok(tables, anchors)
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    pos = np.flatnonzero(anchored_hits(data, tables, delims, words, anchors, bs, served)).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals


def find_records_anchored_model(data, alternatives, delims, words, anchors, blocksize, cap=0, max_len=0, served=None, invert=False,
                                before=0, after=0):
    """(starts written, lengths written, block counts, totals[4], numbers written, flags written) as find_context_model gives
    them, S being the non-empty records of known extent that hold a qualifying occurrence - or, with `invert`, hold none.
    (The tested span of an occurrence lies inside [s - 1, e] of its record, whose blocks are served when its extent is
    known: the records' own rule decides, as in the older models.)"""
    data = np.asarray(data, dtype=np.uint8)
    tables = alt_tables(alternatives)
    assert budget_ok(tables, anchors)
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
        hits = np.concatenate([[0], np.cumsum(anchored_hits(data, tables, delims, words, anchors))])
        has = hits[e] > hits[s]
        cand = known_records(s, e, n, bs, served) & (e > s)
        sel = cand & (~has if invert else has)
        bad = np.concatenate([[0], np.cumsum(~served)])     # blocks that are not served in front of block b
        at = np.flatnonzero(sel)
        no = np.arange(s.size)
        report = sel.copy()
        if at.size:                                         # (find_context_model's dilation, word for word)
            p = np.searchsorted(at, no, side="right") - 1
            m = at[np.maximum(p, 0)]
            report |= cand & (p >= 0) & (no - m <= after) & (bad[np.minimum(e, n - 1) // bs + 1] == bad[s[m] // bs])
            q = np.searchsorted(at, no, side="left")
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

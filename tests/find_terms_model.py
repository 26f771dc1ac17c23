"""NumPy / Python model of hufgpu_find_records_terms (include/huffman_gpu.h): what the call reports for an input, a list of
TERMS - each a list of alternatives as tests/find_any_model.py takes them -, the mode, a set of delimiters, a layout, the
blocks that are served, the caps, `invert` and the two distances.

Which records SATISFY the call is decided here, record by record and by brute force over ALL occurrences of all alternatives:
every chain of occurrences, one a term, is tried for the ordered mode (a depth-first search that remembers what it has tried),
not the first-occurrence walk of the kernel.  Everything from the satisfying records on - the known-extent rule, `invert`, the
numbers, the context, the caps and totals - is tests/find_context_model.py's, word for word: the model hands it a copy of the
data in which the delimiters stand where they stood, a satisfying record begins with a marker byte and no other byte is one,
and asks for the marker.  Shared by tests/test_find_terms_args.py (which checks the model against Python's `re`) and
tests/test_gpu_find_terms.py (which checks the GPU against it)."""
import numpy as np

from find_any_model import alt_tables
from find_classes_model import class_hits
from find_context_model import find_context_model
from find_records_model import delimiter_values
from find_select_model import all_records

ALL, ORDERED = 0, 1             # HUFGPU_TERMS_ALL, HUFGPU_TERMS_ORDERED


def term_occurrences(data, terms):
    """per term the occurrences (p, p + len) of all its alternatives, as two sorted arrays (by p, then by the end)"""
    tables = alt_tables([a for term in terms for a in term])        # (the checks of the whole table: 64 positions in all)
    out, j = [], 0
    for term in terms:
        assert len(term) >= 1, "a term has an alternative"
        ps, es = [], []
        for _ in term:
            table = tables[j]
            j += 1
            p = np.flatnonzero(class_hits(data, table)).astype(np.int64)
            ps.append(p)
            es.append(p + int(table.shape[0]))
        p, e = np.concatenate(ps), np.concatenate(es)
        order = np.lexsort((e, p))
        out.append((p[order], e[order]))
    return out


def in_order(occ, s, e):
    """is there a chain of occurrences inside [s, e), one a term, each starting at or behind the end of the one before: every
    occurrence of every term is tried"""
    inside = []
    for p, end in occ:
        lo, hi = np.searchsorted(p, s), np.searchsorted(p, e)       # (a match that starts in a record lies in it)
        inside.append(list(zip(p[lo:hi].tolist(), end[lo:hi].tolist())))
    tried = {}

    def chain(t, x):
        if t == len(inside):
            return True
        if (t, x) not in tried:
            tried[t, x] = any(chain(t + 1, end) for p, end in inside[t] if p >= x)
        return tried[t, x]

    return chain(0, s)


_memo = {}


def satisfying(data, terms, delims, mode):
    """(starts, ends, bool: does the record satisfy the call) of every record of the data, the empty ones included.  The last
    few answers are kept: a test asks for one input's answer at several caps, distances and sets of served blocks"""
    data = np.asarray(data, dtype=np.uint8)
    key = (data.tobytes(), repr(terms), bytes(delimiter_values(delims)), mode)
    if key not in _memo:
        if len(_memo) >= 4:
            _memo.pop(next(iter(_memo)))
        _memo[key] = _satisfying(data, terms, delims, mode)
    return _memo[key]


def _satisfying(data, terms, delims, mode):
    assert mode in (ALL, ORDERED) and 1 <= len(terms) <= 4
    s, e = all_records(data, delims)
    occ = term_occurrences(data, terms)
    ok = np.ones(s.size, bool)
    for p, _ in occ:                                                # every term has an occurrence that starts in the record
        before = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=data.size + 1))])
        ok &= before[e] > before[s]
    if mode == ORDERED:
        if any(len({len(a) for a in term}) > 1 for term in terms):
            raise ValueError("an ordered call needs one length a term")
        for k in np.flatnonzero(ok):
            ok[k] = in_order(occ, int(s[k]), int(e[k]))
    return s, e, ok


def find_terms_model(data, terms, delims, blocksize, cap=0, max_len=0, served=None, invert=False, before=0, after=0, mode=ALL):
    """(starts written, lengths written, block counts, totals[4], numbers written, flags written) as find_context_model gives
    them, S being the records of known extent that satisfy the call"""
    data = np.asarray(data, dtype=np.uint8)
    values = delimiter_values(delims)
    for term in terms:
        assert not any(t[:, values].any() for t in alt_tables(term)), "a class holds no delimiter"
    free = [v for v in range(256) if v not in set(values)]
    assert len(free) >= 2, "two byte values that are no delimiter"
    marker, other = free[0], free[1]
    s, e, ok = satisfying(data, terms, delims, mode)
    marks = np.where(np.isin(data, np.asarray(values, dtype=np.uint8)), data, np.uint8(other)).astype(np.uint8)
    marks[s[ok & (e > s)]] = marker
    return find_context_model(marks, [[bytes([marker])]], delims, blocksize, cap, max_len, served, invert, before, after)

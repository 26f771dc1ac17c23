"""NumPy models of hufgpu_find_any_expr and hufgpu_find_records_expr (include/huffman_gpu.h): what the calls report for an
input, a list of TERMS, the delimiters D, the word bytes W, the anchors, the mode, a layout, the blocks that are served and the
caps.  A term is a list of alternatives, an alternative a list of items as tests/find_quant_model.py takes them: a class -
required - or (class, True) - may be left out.  The positions call has one term.

No bit tricks.  The matcher is an NFA simulation, state by state: can[p][L] says that SOME form of the alternative lies at p
with L bytes.  The byte behind an occurrence is a required last step - "R is absent or allowed" -, which the data's end
satisfies, so for every start the shortest QUALIFYING form is the first L with can[p][L] and that step; the byte in front is
looked at start by start.  A start counts when the tested span of that form - [p, p + L), widened by the neighbours that exist
and are tested - lies in served blocks: a shorter span touches no more blocks, so the shortest qualifying form decides.

Which records are SELECTED is decided record by record: with one term a record that holds a qualifying occurrence; with
HUFGPU_TERMS_ALL one that holds an occurrence of every term; with HUFGPU_TERMS_ORDERED one in which a chain of occurrences, one
a term, each starting at or behind the end of the one before, exists among ALL occurrences of ALL forms - a depth-first search
that remembers what it has tried, not the kernel's first-occurrence walk -, the first one's L and the last one's R qualifying
(the anchors bind the outer edges).  Everything from the selected records on is tests/find_context_model.py's, word for word,
handed over as tests/find_terms_model.py does: a copy of the data in which a selected record begins with a marker byte.
Shared by tests/test_find_expr_args.py (which checks the models against Python's `re`) and tests/test_gpu_find_expr.py (which
checks the GPU against them)."""
import numpy as np

from find_context_model import find_context_model
from find_model import block_lens
from find_quant_model import split
from find_records_model import delimiter_values
from find_select_model import all_records

BOL, EOL, WORD = 1, 2, 4        # HUFGPU_ANCHOR_*
ALL, ORDERED = 0, 1             # HUFGPU_TERMS_*


def expr_tables(terms, anchors, mode):
    """per term the (table, flags) of its alternatives; the checks of the calls"""
    assert 1 <= len(terms) <= 4 and 0 <= anchors < 8 and mode in (ALL, ORDERED)
    parts = [[split(a) for a in term] for term in terms]
    flat = [p for term in parts for p in term]
    assert all(len(term) >= 1 for term in parts) and len(flat) <= 64
    assert all(t.shape[0] >= 1 and t.any(axis=1).all() for t, _ in flat), "no alternative of length 0, no empty class"
    assert all(not o.all() for _, o in flat), "no alternative that is all optional"
    assert not (mode == ALL and len(terms) > 1 and anchors), "anchors with ALL of several terms"
    if mode == ORDERED:
        for term in parts[:-1]:
            assert not any(o.any() for _, o in term) and len({t.shape[0] for t, _ in term}) == 1, "a term in front of another has one length"
    behind = len(parts[-1]) if anchors & (EOL | WORD) else 0
    assert sum(t.shape[0] for t, _ in flat) + behind <= 64, "the positions and the boundary positions sum to at most 64"
    return parts


def form_lengths(data, table, optional):
    """bool [n + 1][m + 1]: can[p][L] - some form of the alternative lies at p with exactly L bytes"""
    n, m = int(data.size), int(table.shape[0])
    after = np.zeros((n + 1, m + 1), bool)                  # behind the last position: a form is complete, 0 bytes more
    after[:, 0] = True
    for k in range(m - 1, -1, -1):
        here = np.zeros((n + 1, m + 1), bool)
        took = table[k][data]                               # position k takes byte p, the rest goes on at p + 1
        here[:n, 1:] = after[1:, :-1] & took[:, None]
        if optional[k]:
            here |= after                                   # ... or it is left out
        after = here
    after[:, 0] = False                                     # (no alternative is all optional)
    return after


def neighbours(data, delims, words, anchors):
    """(bool [n]: may the byte in front of start p stand there, bool [n + 1]: may the byte AT q stand behind a form that ends
    there); an absent neighbour never stands in the way"""
    n = int(data.size)
    in_d = np.isin(data, np.asarray(delimiter_values(delims), dtype=np.uint8)) if anchors & (BOL | EOL) else np.zeros(n, bool)
    in_w = np.isin(data, np.asarray(delimiter_values(words), dtype=np.uint8)) if anchors & WORD else np.zeros(n, bool)
    left, right = np.ones(n, bool), np.ones(n + 1, bool)
    if anchors & BOL:
        left[1:] &= in_d[:-1]
    if anchors & EOL:
        right[:n] &= in_d
    if anchors & WORD:
        left[1:] &= ~in_w[:-1]
        right[:n] &= ~in_w
    return left, right


def qualifying_lengths(data, part, right):
    """int [n]: the length of the alternative's shortest form at each start whose right neighbour qualifies, 0: none"""
    table, optional = part
    n, m = int(data.size), int(table.shape[0])
    can = form_lengths(data, table, optional)
    best = np.zeros(n, np.int64)
    p = np.arange(n)
    for length in range(m, 0, -1):
        ok = can[:n, length] & (p + length <= n)
        ok[ok] = right[p[ok] + length]
        best[ok] = length
    return best


def expr_hits(data, term, delims, words, anchors, bs=None, served=None, front=True):
    """bool [n]: the starts at which a form of an alternative of the term lies and qualifies (and, with `served`, the
    shortest qualifying one has its tested span in served blocks only); front = False: the byte in front is not looked at"""
    n = int(data.size)
    left, right = neighbours(data, delims, words, anchors)
    if not front:
        left[:] = True
    hit = np.zeros(n, bool)
    bad = None if served is None else np.concatenate([[0], np.cumsum(~served)])
    for part in term:
        length = qualifying_lengths(data, part, right)
        h = (length > 0) & left
        if bad is not None and h.any():
            p = np.flatnonzero(h)
            lo = np.where((p > 0) & bool(front and anchors & (BOL | WORD)), p - 1, p)
            end = p + length[p]
            hi = np.where((end < n) & bool(anchors & (EOL | WORD)), end, end - 1)
            h[p] = bad[hi // bs + 1] == bad[lo // bs]
        hit |= h
    return hit


def find_any_expr_model(data, alternatives, delims, words, anchors, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block), as find_any_model"""
    data = np.asarray(data, dtype=np.uint8)
    (term,) = expr_tables([alternatives], anchors, ORDERED)
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    pos = np.flatnonzero(expr_hits(data, term, delims, words, anchors, bs, served)).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals


def occurrences(data, term, left, right):
    """every (p, end) of every form of every alternative of the term with left[p] and right[end], sorted by p"""
    n = int(data.size)
    ps, es = [], []
    for table, optional in term:
        can = form_lengths(data, table, optional)
        for length in range(1, int(table.shape[0]) + 1):
            p = np.flatnonzero(can[:n, length] & left)
            p = p[p + length <= n]
            p = p[right[p + length]]
            ps.append(p)
            es.append(p + length)
    p, e = np.concatenate(ps).astype(np.int64), np.concatenate(es).astype(np.int64)
    order = np.lexsort((e, p))
    return p[order], e[order]


def in_order(occ, s, e):
    """is there a chain of occurrences that start inside [s, e), one a term, each at or behind the end of the one before"""
    inside = []
    for p, end in occ:
        lo, hi = np.searchsorted(p, s), np.searchsorted(p, e)
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


def selected(data, terms, delims, words, anchors, mode):
    """(starts, ends, bool: is the record selected) of every record of the data, the empty ones included; the last few
    answers are kept, as tests/find_terms_model.py keeps them"""
    data = np.asarray(data, dtype=np.uint8)
    key = (data.tobytes(), repr(terms), bytes(delimiter_values(delims)), bytes(delimiter_values(words)) if anchors & WORD else b"", anchors, mode)
    if key not in _memo:
        if len(_memo) >= 4:
            _memo.pop(next(iter(_memo)))
        _memo[key] = _selected(data, terms, delims, words, anchors, mode)
    return _memo[key]


def _selected(data, terms, delims, words, anchors, mode):
    parts = expr_tables(terms, anchors, mode)
    n = int(data.size)
    s, e = all_records(data, delims)
    left, right = neighbours(data, delims, words, anchors)
    free_l, free_r = np.ones(n, bool), np.ones(n + 1, bool)
    last = len(parts) - 1
    occ = [occurrences(data, term, left if t == 0 else free_l, right if t == last else free_r) for t, term in enumerate(parts)]
    ok = np.ones(s.size, bool)
    for p, _ in occ:                                        # every term has an occurrence that starts in the record
        before = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=n + 1))])
        ok &= before[e] > before[s]
    if mode == ORDERED and len(parts) > 1:
        for k in np.flatnonzero(ok):
            ok[k] = in_order(occ, int(s[k]), int(e[k]))
    return s, e, ok


def find_records_expr_model(data, terms, delims, words, anchors, mode, blocksize, cap=0, max_len=0, served=None, invert=False, before=0,
                            after=0):
    """(starts written, lengths written, block counts, totals[4], numbers written, flags written) as find_context_model gives
    them, S being the non-empty records of known extent that are selected - or, with `invert`, are not.  (The tested span of
    an occurrence lies inside [s - 1, e] of its record, whose blocks are served when its extent is known: the records' own
    rule decides, as in the older models.)"""
    data = np.asarray(data, dtype=np.uint8)
    values = delimiter_values(delims)
    for term in expr_tables(terms, anchors, mode):
        assert not any(t[:, values].any() for t, _ in term), "a class holds no delimiter"
    free = [v for v in range(256) if v not in set(int(x) for x in values)]
    assert len(free) >= 2, "two byte values that are no delimiter"
    marker, other = free[0], free[1]
    s, e, ok = selected(data, terms, delims, words, anchors, mode)
    marks = np.where(np.isin(data, np.asarray(values, dtype=np.uint8)), data, np.uint8(other)).astype(np.uint8)
    marks[s[ok & (e > s)]] = marker
    return find_context_model(marks, [[bytes([marker])]], delims, blocksize, cap, max_len, served, invert, before, after)

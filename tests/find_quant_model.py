"""NumPy models of hufgpu_find_any_quant and hufgpu_find_records_quant (include/huffman_gpu.h): what the calls report for an
input, a list of alternatives whose positions may be OPTIONAL, a layout, the blocks that are served and the caps.

An alternative is a list of items: a class as tests/find_classes_model.py's class_table takes it - required -, or
(class, True) - may be left out.  The matcher is an NFA simulation, state by state, and no bit trick: for every position k of
an alternative, short[k][p] is the length of the SHORTEST way to match the positions k ... end from byte p on (INF: none) -
position k takes byte p when that is in its class, or is skipped when it is optional.  A start is a match when the shortest
form of some alternative that lies there ends inside the data and touches served blocks only: a shorter span touches no more
blocks, so the shortest form decides.  The records' calls come through the existing models: which record holds a match is all
that they ask of the matcher, so they get the data with a marker byte at every start that matches.  Shared by
tests/test_find_quant_args.py (which checks the models against Python's `re`) and tests/test_gpu_find_quant.py (which checks
the GPU against them)."""
import numpy as np

from find_classes_model import class_table
from find_context_model import find_context_model
from find_model import block_lens
from find_records_model import delimiter_values

INF = 1 << 20


def split(alternative):
    """(the bool [len][256] table, the bool [len] flags) of one alternative"""
    items = [(c[0], True) if isinstance(c, tuple) and len(c) == 2 and c[1] is True else (c, False) for c in alternative]
    table = class_table([c for c, _ in items])
    return table, np.array([o for _, o in items], bool)


def quant_tables(alternatives):
    parts = [split(a) for a in alternatives]
    assert 1 <= len(parts) <= 64, "1 to 64 alternatives"
    assert all(t.shape[0] >= 1 and t.any(axis=1).all() for t, _ in parts), "no alternative of length 0, no empty class"
    assert all(not o.all() for _, o in parts), "no alternative that is all optional"
    assert sum(t.shape[0] for t, _ in parts) <= 64, "the positions sum to at most 64"
    return parts


def shortest_form(data, table, optional, end=None):
    """int [n]: the length of the shortest form of the alternative that lies at each start and ends at or in front of `end`
    (the data's end when not given), INF where none does"""
    n = int(data.size)
    end = n if end is None else end
    after = np.full(n + 1, INF, np.int64)                   # behind the last position: a form is complete, 0 bytes more
    after[:end + 1] = 0
    for k in range(table.shape[0] - 1, -1, -1):
        here = np.full(n + 1, INF, np.int64)
        took = table[k][data] & (after[1:] < INF)           # position k takes byte p, the rest goes on at p + 1
        here[:n][took] = after[1:][took] + 1
        if optional[k]:
            here = np.minimum(here, after)                  # ... or it is left out
        after = here
    return after[:n]


def quant_lengths(data, parts):
    """int [n]: the length of the shortest form of any alternative at each start, INF: no match"""
    best = np.full(int(data.size), INF, np.int64)
    for table, optional in parts:
        best = np.minimum(best, shortest_form(data, table, optional))
    return best


def quant_hits(data, parts, bs=None, served=None):
    """bool [n]: the starts at which a form lies (and, with `served`, the shortest one touches served blocks only)"""
    length = quant_lengths(data, parts)
    hit = length < INF
    if served is not None and hit.any():
        bad = np.concatenate([[0], np.cumsum(~served)])
        p = np.flatnonzero(hit)
        hit[p] = bad[(p + length[p] - 1) // bs + 1] == bad[p // bs]
    return hit


def find_quant_model(data, alternatives, blocksize, cap=0, served=None):
    """(positions written, block counts, totals[4]) for `data` in blocks of `blocksize` (0: one block), as find_any_model"""
    data = np.asarray(data, dtype=np.uint8)
    parts = quant_tables(alternatives)
    n = int(data.size)
    bs = blocksize or n
    nb = len(block_lens(n, blocksize))
    served = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    assert served.size == nb
    pos = np.flatnonzero(quant_hits(data, parts, bs, served)).astype(np.int64)
    counts = np.bincount(pos // bs, minlength=nb).astype(np.int64) if nb else np.zeros(0, np.int64)
    total = int(pos.size)
    written = min(total, int(cap))
    totals = np.array([total, written, int(nb - served.sum()), 0], dtype=np.int64)
    return pos[:written], counts, totals


def marked(data, alternatives, delims):
    """(the data with HIT at every start that matches and MISS at every other byte that is no delimiter, [[HIT]]): what the
    records' models need to know of the matcher"""
    data = np.asarray(data, dtype=np.uint8)
    parts = quant_tables(alternatives)
    values = delimiter_values(delims)
    assert not any(t[:, values].any() for t, _ in parts), "a class holds no delimiter"
    hit_v, miss_v = [v for v in range(256) if v not in set(int(x) for x in values)][:2]
    is_delim = np.isin(data, np.asarray(values, dtype=np.uint8))
    out = np.where(quant_hits(data, parts), hit_v, miss_v).astype(np.uint8)
    out[is_delim] = data[is_delim]
    return out, [[bytes([hit_v])]]


def find_quant_records_model(data, alternatives, delims, blocksize, cap=0, max_len=0, served=None, invert=False, before=0, after=0):
    """what find_context_model gives - (starts, lengths, counts, totals, numbers, flags) - for the records that hold a match"""
    out, alts = marked(data, alternatives, delims)
    return find_context_model(out, alts, delims, blocksize, cap, max_len, served, invert, before, after)

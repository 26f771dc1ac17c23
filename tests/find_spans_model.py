"""The model of hufgpu_find_any_spans (include/huffman_gpu.h): hufgpu_find_any_expr's answer with, for every reported start,
the length of the LONGEST form that lies there, qualifies and has its tested span in served bytes, and the flag "a longer one
could not be ruled out".  Not a test.

The starts are tests/find_expr_model.py's.  For each of them a forward NFA simulation runs, state by state and without a bit
trick: a state (j, i) says "position i of alternative j takes the next byte", (j, len_j) that a form of j is complete, and an
optional position may be left out.  A complete form of k bytes qualifies when its right neighbour is not tested, is absent
(the data ends there) or is allowed (find_expr_model.neighbours); the left neighbour belongs to the start, not to a form, and
find_any_expr_model has looked at it.  The simulation stops at the first byte of a block that is not served: the span is open
when a state could still take that byte, or when a complete form waits for it as its right neighbour.
Shared by tests/test_find_spans_args.py (which checks it against Python's `re`) and tests/test_gpu_find_spans.py."""
import numpy as np

from find_expr_model import BOL, EOL, WORD, find_any_expr_model, neighbours  # noqa: F401  (the tests import the bits from here)
from find_model import block_lens
from find_quant_model import split


def _closure(states, parts):
    out, todo = set(states), list(states)
    while todo:
        j, i = todo.pop()
        table, optional = parts[j]
        if i < table.shape[0] and optional[i] and (j, i + 1) not in out:
            out.add((j, i + 1))
            todo.append((j, i + 1))
    return out


def span_at(data, parts, right, tested, p, bs, served):
    """(length, open) of the longest qualifying form at start p whose tested span is served"""
    n = int(data.size)
    lens = [int(t.shape[0]) for t, _ in parts]
    states = _closure({(j, 0) for j in range(len(parts))}, parts)
    best, k, waiting = 0, 0, False
    while True:
        q = p + k
        if q >= n:
            return (k if waiting else best), False
        if not served[q // bs]:
            return best, bool(waiting or any(i < lens[j] for j, i in states))
        x = int(data[q])
        if waiting and right[q]:
            best = k
        states = _closure({(j, i + 1) for j, i in states if i < lens[j] and parts[j][0][i][x]}, parts)
        k += 1
        complete = any(i == lens[j] for j, i in states)
        if complete and not tested:
            best = k
        waiting = complete and tested
        if not waiting and not any(i < lens[j] for j, i in states):
            return best, False


def find_spans_model(data, alternatives, delims, words, anchors, blocksize, cap=0, served=None):
    """(positions, lengths int32, open uint8, block counts, totals[4]) - the first three cut at the cap; totals[3]: the open
    spans among the written ones"""
    data = np.asarray(data, dtype=np.uint8)
    n = int(data.size)
    bs = blocksize or max(n, 1)
    nb = len(block_lens(n, blocksize))
    srv = np.ones(nb, bool) if served is None else np.asarray(served, bool)
    pos, counts, totals = find_any_expr_model(data, alternatives, delims, words, anchors, blocksize, cap, served)
    parts = [split(a) for a in alternatives]
    right = neighbours(data, delims, words, anchors)[1]
    tested = bool(anchors & (EOL | WORD))
    got = [span_at(data, parts, right, tested, int(p), bs, srv) for p in pos]
    lengths = np.array([g[0] for g in got], np.int32)
    opened = np.array([g[1] for g in got], np.uint8)
    totals = totals.copy()
    totals[3] = int(opened.sum())
    return pos, lengths, opened, counts, totals

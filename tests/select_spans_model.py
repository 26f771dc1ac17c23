"""The model of hufgpu_select_spans (include/huffman_gpu.h): the greedy loop.  Rank 0 is selected; behind a selected rank s the
next one is the least r > s with pos[r] >= pos[s] + len[s] - one numpy.searchsorted for every rank's successor, then the walk.
Not a test.  Shared by tests/test_select_spans_args.py (which checks it against Python's `re` and against grep) and
tests/test_gpu_select_spans.py."""
import numpy as np

HUFE_ARGUMENT = 2
LEN_MAX = 64


def offending_rank(pos, lens):
    """the lowest rank r with a length outside 1 ... 64 or, r > 0, pos[r] <= pos[r - 1]; None: the input is valid"""
    pos, lens = np.asarray(pos, np.uint64), np.asarray(lens, np.int64)
    bad = (lens < 1) | (lens > LEN_MAX)
    bad[1:] |= pos[1:] <= pos[:-1]
    at = np.flatnonzero(bad)
    return int(at[0]) if at.size else None


def select_model(pos, lens, n=None, cap=None):
    """(selected positions uint64, lengths int32, ranks int64, totals[4]) of the first `n` spans (default: all), the three
    arrays cut at `cap` (default: nothing is cut).  Invalid input: empty arrays and totals [0, 0, status, the rank]."""
    pos, lens = np.asarray(pos, np.uint64), np.asarray(lens, np.int32)
    n = pos.size if n is None else min(int(n), pos.size)
    pos, lens = pos[:n], lens[:n]
    bad = offending_rank(pos, lens)
    if bad is not None:
        return pos[:0], lens[:0], np.zeros(0, np.int64), np.array([0, 0, HUFE_ARGUMENT, bad], np.int64)
    succ = np.searchsorted(pos, pos + lens.astype(np.uint64), side="left")
    ranks, r = [], 0
    while r < n:
        ranks.append(r)
        r = int(succ[r])
    ranks = np.array(ranks, np.int64)
    written = ranks.size if cap is None else min(ranks.size, int(cap))
    totals = np.array([ranks.size, written, 0, 0], np.int64)
    ranks = ranks[:written]
    return pos[ranks], lens[ranks], ranks, totals

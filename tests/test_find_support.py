"""The checker of tests/find_support.py, without a device: it accepts a result that is the model's answer word for word, and
raises for every single difference - a written entry, a guard word in front of the entries, behind them or right at
totals[1], a total, a status, a block count, a number, a flag, and an output that the model does not have.

The result is made from tests/find_context_model.py at a cap of 5 with three records written, in the layout that
find_support.find_call gives: LEAD guard words, `cap` slots, TAIL guard words.
"""
import numpy as np
import pytest

from find_context_model import find_context_model
from find_records_model import find_records_model
from find_support import GUARD8, GUARD32, GUARD64, LEAD, TAIL, check, positions_of

CAP = 5
DATA = np.frombuffer(b"one\ntwo ab\nthree\nab four\nfive\nsix ab\nseven", np.uint8)
ALTS = [[b"a", b"b"]]
BS = 16


def answer():
    """(the model's answer, the 7-tuple that holds exactly it)"""
    want = find_context_model(DATA, ALTS, b"\n", BS, CAP)
    starts, lengths, counts, totals, numbers, flags = want
    assert totals.tolist() == [3, 3, 0, 0] and starts.size == 3

    def guarded(values, guard, dtype):
        buf = np.full(LEAD + CAP + TAIL, guard, dtype)
        buf[LEAD:LEAD + values.size] = values
        return buf

    res = [guarded(starts, GUARD64, np.int64), guarded(lengths, GUARD32, np.int32), totals.copy(), np.zeros(counts.size, np.int32),
           counts.copy(), guarded(numbers, GUARD64, np.int64), guarded(flags, GUARD8, np.uint8)]
    return want, res


def test_the_exact_answer_is_accepted():
    want, res = answer()
    check(tuple(res), want, CAP)
    check(tuple(res[:6]), want[:5], CAP)                    # the select call's six, the records calls' five, a positions call's four
    check(tuple(res[:5]), want[:4], CAP)
    check(positions_of(res), (want[0], want[2], want[3]), CAP)
    res[5] = res[6] = None                                  # outputs that were not asked for are not compared
    check(tuple(res), want, CAP)
    assert np.array_equal(want[0], find_records_model(DATA, b"ab", b"\n", BS, CAP)[0])


PERTURBATIONS = {
    "a start": (0, LEAD + 1, 1),
    "a length": (1, LEAD + 2, 1),
    "a guard word in front": (0, LEAD - 1, 1),
    "a guard word in front of the lengths": (1, 0, 1),
    "a guard word behind": (0, LEAD + CAP, 1),
    "the last guard word behind the flags": (6, LEAD + CAP + TAIL - 1, 1),
    "the word at totals[1]": (0, LEAD + 3, 1),
    "the number at totals[1]": (5, LEAD + 3, 1),
    "totals[0]": (2, 0, 1),
    "totals[3]": (2, 3, 1),
    "a status": (3, 1, 3),
    "a block count": (4, 0, 1),
    "a number": (5, LEAD, 1),
    "a flag": (6, LEAD + 2, 1),
}


@pytest.mark.parametrize("what", list(PERTURBATIONS))
def test_one_difference_is_found(what):
    want, res = answer()
    output, at, xor = PERTURBATIONS[what]
    res[output] = res[output].copy()
    res[output][at] ^= xor
    with pytest.raises(AssertionError):
        check(tuple(res), want, CAP, what)


def test_an_output_the_model_does_not_have():
    want, res = answer()
    with pytest.raises(AssertionError):
        check(tuple(res), want[:5], CAP)                    # flags, and the model has none
    with pytest.raises(AssertionError):
        check(tuple(res[:6]), want[:4], CAP)                # numbers, and the model has none
    with pytest.raises(AssertionError):
        check(tuple(res), (want[0], want[2], want[3]), CAP)  # lengths, and a positions model has none

"""hufgpu_find_bytes: the argument check of its own and the NumPy model of its result (no GPU needed).  The checks it shares
with the other calls of the search family are the functions of tests/find_args_cases.py.
"""
import numpy as np
import pytest

import find_args_cases as cases
from find_args_support import HUFE_ARGUMENT, LAYOUTS, call, lib
from find_model import block_lens, byte_set, find_model

NAME = "find_bytes"


def test_symbol_is_exported_and_declared(lib):
    cases.the_symbol_is_exported_and_declared(lib, NAME)


@pytest.mark.parametrize("missing", ["st", "totals"])
def test_null_set_or_totals(lib, missing):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, "find_bytes", nblocks=nblocks, raw_size=raw_size, **{missing: None})
        assert rc == HUFE_ARGUMENT and "set and d_totals are required" in msg


# ---- the checks that every call shares (tests/find_args_cases.py), under the names they have always had here -----------------
def test_valid_arguments_still_need_a_context(lib):
    cases.valid_arguments_still_need_a_context(lib, NAME, {})


@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, missing):
    cases.null_device_arrays(lib, NAME, {}, missing)


def test_a_cap_without_positions(lib):
    cases.a_cap_without_its_outputs(lib, NAME, {})


def test_missing_or_misaligned_sub_index(lib):
    cases.missing_or_misaligned_sub_index(lib, NAME, {})


@pytest.mark.parametrize("kw", cases.BAD_LAYOUTS)
def test_a_layout_that_does_not_give_nblocks(lib, kw):
    cases.a_layout_that_does_not_give_nblocks(lib, NAME, {}, kw)


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_byte_set_bits():
    assert byte_set([]) == bytes(32)
    assert byte_set(range(256)) == b"\xff" * 32
    s = byte_set([10, 255, 8])
    assert s[1] == 0b101 and s[31] == 0x80 and sum(s) == 5 + 0x80


def test_model_positions_counts_and_caps():
    data = np.array([1, 2, 1, 3, 1, 1, 2], np.uint8)
    assert block_lens(7, 3) == [3, 3, 1] and block_lens(7, 0) == [7] and block_lens(0, 3) == []
    pos, counts, totals = find_model(data, [1], 3, cap=10)
    assert pos.tolist() == [0, 2, 4, 5] and counts.tolist() == [2, 2, 0] and totals.tolist() == [4, 4, 0, 0]
    pos, counts, totals = find_model(data, [1, 2], 3, cap=3)
    assert pos.tolist() == [0, 1, 2] and counts.tolist() == [3, 2, 1] and totals.tolist() == [6, 3, 0, 0]
    pos, counts, totals = find_model(data, [1], 0, cap=0)
    assert pos.size == 0 and counts.tolist() == [4] and totals.tolist() == [4, 0, 0, 0]
    pos, counts, totals = find_model(data, [], 3, cap=5)
    assert pos.size == 0 and counts.tolist() == [0, 0, 0] and totals.tolist() == [0, 0, 0, 0]


def test_model_blocks_that_are_not_served():
    data = np.array([1, 2, 1, 3, 1, 1, 2], np.uint8)
    pos, counts, totals = find_model(data, [1], 3, cap=10, served=[True, False, True])
    assert pos.tolist() == [0, 2] and counts.tolist() == [2, 0, 0] and totals.tolist() == [2, 2, 1, 0]
    pos, counts, totals = find_model(np.zeros(0, np.uint8), [1], 3, cap=10)
    assert pos.size == 0 and counts.size == 0 and totals.tolist() == [0, 0, 0, 0]

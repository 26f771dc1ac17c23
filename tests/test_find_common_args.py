"""The argument checks that the eleven C calls of the search family share (tests/find_args_cases.py), run for every call they
apply to, with the call's own prefix in front of the message.  What only one call has - its new arguments, its identity with
the older call, its model, its Python keywords - is in that call's tests/test_find_*args.py.  No GPU needed.

A call whose own arguments change what is looked at is tried under each setting of them (`settings`): the select call plain and
inverted, the context call with three windows and both, the anchored calls with every combination of the three anchors.
"""
import pytest

import find_args_cases as cases
from find_args_support import FAR, lib
from find_calls import ANY_OF_CALLS, CALLS, RECORD_CALLS


def settings(name):
    """[(id, keywords)]: the settings of the call's own arguments under which every shared case must hold"""
    slots = CALLS[name]
    if "anchors" in slots:
        return [("anchors%d" % a, dict(anchors=a)) for a in range(8)]
    if "before" in slots:
        return [(f"{w}-{s}", dict(ba=ba, select=sel)) for w, ba in (("select", (0, 0)), ("2-3", (2, 3)), ("all", (FAR, FAR)))
                for s, sel in (("plain", 0), ("invert", 1))]
    if "select" in slots:
        return [("plain", dict(select=0)), ("invert", dict(select=1))]
    return [("", {})]


def every(names):
    """parametrize over (call, setting) for these calls"""
    targets = [(name, kw, f"{name}-{sid}" if sid else name) for name in names for sid, kw in settings(name)]
    return pytest.mark.parametrize("name,kw", [t[:2] for t in targets], ids=[t[2] for t in targets])


def lens_id(lens):
    return "+".join(map(str, lens)) if len(lens) < 5 else f"{lens[0]}x{len(lens) - 1}+{lens[-1]}"


def fits_the_budget(name, kw, lens, *_):
    """an anchored call with EOL or WORD keeps a bit an alternative for the boundary, and says so in front of the checks of
    the classes (its own tests try that budget): such a table is tried with the anchors that cost nothing"""
    return not ("anchors" in CALLS[name] and kw["anchors"] & 6 and sum(lens) + len(lens) > 64)


def every_any_of_call_with(argnames, tables, fits=lambda *a: True):
    """parametrize over (any-of call, setting, table): `tables` are tuples that start with the alternatives' lengths"""
    cases = [((name, kw) + tuple(t), f"{name}-{sid}-" + "-".join([lens_id(t[0])] + [str(x) for x in t[1:]]))
             for name in ANY_OF_CALLS for sid, kw in settings(name) for t in tables if fits(name, kw, *t)]
    return pytest.mark.parametrize("name,kw," + argnames, [c[0] for c in cases], ids=[c[1].replace("--", "-") for c in cases])


EVERY_CALL = every(list(CALLS))


EVERY_RECORDS_CALL = every(RECORD_CALLS)


EVERY_ANY_OF_CALL = every(ANY_OF_CALLS)


# ---- the symbol ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CALLS))
def test_the_symbol_is_exported_and_declared(lib, name):
    cases.the_symbol_is_exported_and_declared(lib, name)


# ---- what every call checks ------------------------------------------------------------------------------------------------
@EVERY_CALL
def test_valid_arguments_still_need_a_context(lib, name, kw):
    cases.valid_arguments_still_need_a_context(lib, name, kw)


@EVERY_CALL
@pytest.mark.parametrize("missing", cases.NULL_ARRAYS)
def test_null_device_arrays(lib, name, kw, missing):
    cases.null_device_arrays(lib, name, kw, missing)


@EVERY_CALL
def test_null_totals(lib, name, kw):
    cases.null_totals(lib, name, kw)


@EVERY_CALL
def test_a_cap_without_its_outputs(lib, name, kw):
    cases.a_cap_without_its_outputs(lib, name, kw)


@EVERY_RECORDS_CALL
def test_a_null_delimiter_set(lib, name, kw):
    cases.a_null_delimiter_set(lib, name, kw)


@EVERY_CALL
def test_missing_or_misaligned_sub_index(lib, name, kw):
    cases.missing_or_misaligned_sub_index(lib, name, kw)


@EVERY_CALL
@pytest.mark.parametrize("layout", cases.BAD_LAYOUTS, ids=["five", "three", "no-bytes", "one-block", "no-blocks", "huge"])
def test_a_layout_that_does_not_give_nblocks(lib, name, kw, layout):
    cases.a_layout_that_does_not_give_nblocks(lib, name, kw, layout)


@pytest.mark.parametrize("name", list(CALLS))
def test_the_call_keeps_its_wording(lib, name):
    cases.the_call_keeps_its_wording(lib, name)


@EVERY_ANY_OF_CALL
def test_null_arrays_and_counts_of_0_and_65(lib, name, kw):
    cases.null_arrays_and_counts_of_0_and_65(lib, name, kw)


@every_any_of_call_with("lens,at", cases.LENGTHS_OF_0)
def test_an_alternative_of_length_0(lib, name, kw, lens, at):
    cases.an_alternative_of_length_0(lib, name, kw, lens, at)


@every_any_of_call_with("lens", [(lens,) for lens in cases.TOTALS_ABOVE_64])
def test_a_total_above_64(lib, name, kw, lens):
    cases.a_total_above_64(lib, name, kw, lens)


@every_any_of_call_with("lens,j,k", cases.EMPTY_CLASSES, fits_the_budget)
def test_an_empty_class(lib, name, kw, lens, j, k):
    cases.an_empty_class(lib, name, kw, lens, j, k)


@every_any_of_call_with("lens,j,k", cases.DELIMITER_CLASSES, fits_the_budget)
def test_a_class_that_meets_the_delimiter_set(lib, name, kw, lens, j, k):
    cases.a_class_that_meets_the_delimiter_set(lib, name, kw, lens, j, k)


@EVERY_ANY_OF_CALL
def test_the_full_class_and_the_delimiter_set(lib, name, kw):
    cases.the_full_class_and_the_delimiter_set(lib, name, kw)

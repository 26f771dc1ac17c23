"""The argument checks that the eleven C calls of the search family share (tests/find_calls.py), each written once as a plain
function of (lib, the call's name, the keywords of a setting of its own arguments, the case's parameters).
tests/test_find_common_args.py runs every one of them for every call and setting it applies to; a call's own
tests/test_find_*args.py runs them under the names and parameters its module has always had.  Not a test module.
"""
import numpy as np

from find_args_support import EMPTY, FULL, HUFE_ARGUMENT, LAYOUTS, alts_of, byte_set, call, declaration, valid
from find_calls import CALLS, RECORD_CALLS, who
from libhuffman_amd import _native

# the parameters of the cases that have some.  (The last table of EMPTY_CLASSES and of DELIMITER_CLASSES is the one that the
# context and the anchored calls' tests always used.)
NULL_ARRAYS = ["stream", "index", "errs"]
BAD_LAYOUTS = [
    dict(raw_size=5 * 4096),                            # five blocks
    dict(raw_size=3 * 4096),                            # three
    dict(raw_size=0),
    dict(blocksize=0),                                  # one block
    dict(nblocks=0),                                    # no blocks, but bytes
    dict(blocksize=(1 << 38) + 1, raw_size=4 * ((1 << 38) + 1)),
]
LENGTHS_OF_0 = [([0], 0), ([3, 0, 2], 1), ([1, 1, 0], 2), ([1] * 63 + [0], 63), ([0, 70], 0)]
TOTALS_ABOVE_64 = [[65], [64, 1], [32, 33], [1] * 63 + [2], [2, 5, 33, 25], [0xFFFFFFFF, 2], [0x80000000, 0x80000000]]
EMPTY_CLASSES = [([5], 0, 0), ([5], 0, 4), ([2, 5, 33], 1, 2), ([2, 5, 33], 2, 32), ([31, 33], 1, 0), ([1] * 64, 63, 0), ([1, 63], 1, 62),
                 ([32, 32], 0, 31), ([2, 3], 1, 2)]
DELIMITER_CLASSES = [([5], 0, 0), ([2, 5, 33], 1, 4), ([2, 5, 33], 2, 0), ([31, 33], 1, 32), ([1] * 64, 40, 0), ([1, 63], 0, 0), ([2, 2], 1, 1)]

# what the first check of the searched-for thing and d_totals says, and the slot of that thing
REQUIRED = {"st": "set and d_totals are required", "pattern": "pattern and d_totals are required", "cls": "classes and d_totals are required",
            "lens": "classes, alt_lens and d_totals are required"}


def key_slot(name):
    return next(s for s in ("lens", "st", "pattern", "cls") if s in CALLS[name])


def required(name):
    return REQUIRED[key_slot(name)]


OUTPUTS = ("pos", "rlens", "no", "sel")


def outputs_of(name):
    return [s for s in OUTPUTS if s in CALLS[name]]


def key_none(name):
    """the keywords that make the searched-for thing NULL"""
    return {"cls" if key_slot(name) == "lens" else key_slot(name): None}


def the_symbol_is_exported_and_declared(lib, name):
    """... with as many arguments as the table of calls lists, in the loader and in the header"""
    symbol = "hufgpu_" + name
    assert symbol in _native.GPU_SYMBOLS and hasattr(lib, symbol)
    assert len(getattr(lib, symbol).argtypes) == len(CALLS[name])
    _, m = declaration(name)
    assert m and m.group(0).count(",") == len(CALLS[name]) - 1


def valid_arguments_still_need_a_context(lib, name, kw):
    prefix = who(name)
    assert valid(*call(lib, name, **kw), prefix)
    no_outputs = dict.fromkeys(outputs_of(name))
    assert valid(*call(lib, name, cap=0, counts=None, **no_outputs, **kw), prefix)
    if "max_len" in CALLS[name]:
        assert valid(*call(lib, name, max_len=0, **kw), prefix)
    assert valid(*call(lib, name, blocksize=0, nblocks=1, **kw), prefix)
    # nblocks = 0 is success only with a context to enqueue the zeroing of d_totals on
    no_blocks = dict(stream=None, index=None, sub=None, errs=None, nblocks=0, raw_size=0)
    assert valid(*call(lib, name, **no_blocks, **kw), prefix)
    assert valid(*call(lib, name, counts=None, **no_blocks, **kw), prefix)


def null_device_arrays(lib, name, kw, missing):
    rc, msg = call(lib, name, **{missing: None}, **kw)
    assert rc == HUFE_ARGUMENT and "are required" in msg and "needs a context" not in msg and msg.startswith(who(name))


def null_totals(lib, name, kw):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, totals=None, **kw)
        assert rc == HUFE_ARGUMENT and required(name) in msg and msg.startswith(who(name)) and "needs a context" not in msg


def a_cap_without_its_outputs(lib, name, kw):
    """a positions call needs d_pos, a records call both d_rec_pos and d_rec_len; with a cap of 0 they may be NULL"""
    prefix = who(name)
    if name in RECORD_CALLS:
        for bad in (dict(pos=None), dict(rlens=None), dict(pos=None, rlens=None)):
            for cap in (1, 3, 16):
                rc, msg = call(lib, name, cap=cap, **bad, **kw)
                assert rc == HUFE_ARGUMENT and msg.startswith(prefix) and "needs d_rec_pos and d_rec_len" in msg, (bad, msg)
                assert f"rec_cap {cap}" in msg and "needs a context" not in msg
            assert valid(*call(lib, name, cap=0, **bad, **kw), prefix)
    else:
        for cap in (1, 3, 16):
            rc, msg = call(lib, name, pos=None, cap=cap, **kw)
            assert rc == HUFE_ARGUMENT and f"pos_cap {cap} needs d_pos" in msg and msg.startswith(prefix) and "needs a context" not in msg
        assert valid(*call(lib, name, pos=None, cap=0, **kw), prefix)


def a_null_delimiter_set(lib, name, kw):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, delims=None, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who(name)) and "delim_set is required" in msg, msg
        assert "needs a context" not in msg
    assert valid(*call(lib, name, delims=EMPTY, **kw), who(name))        # the empty set is valid
    rc, msg = call(lib, name, delims=byte_set(range(256)), **key_none(name), **kw)
    assert required(name) in msg


def missing_or_misaligned_sub_index(lib, name, kw):
    for sub in (None, 0x30004, 0x30001):
        rc, msg = call(lib, name, sub=sub, **kw)
        assert rc == HUFE_ARGUMENT and "8-byte aligned" in msg and msg.startswith(who(name))


def a_layout_that_does_not_give_nblocks(lib, name, kw, layout):
    rc, msg = call(lib, name, **layout, **kw)
    assert rc == HUFE_ARGUMENT and "must be those of the encode" in msg and msg.startswith(who(name))


# a mistake of each call and the whole message, or its beginning, that it has always answered with: a later call's wording
# must not show in an earlier one's
WORDING = {
    "find_bytes": (dict(st=None), "find_bytes: the set and d_totals are required", True),
    "find_pattern": (dict(pattern=b"a\nb", pos=None, cap=1), "find_pattern: pos_cap 1 needs d_pos", True),
    "find_records": (dict(pattern=b"a\nb", cap=1, max_len=0), "find_records: byte 1 of the pattern (value 10)", False),
    "find_classes": (dict(cls=None, plen=3, cap=1), "find_classes: the classes and d_totals are required", True),
    "find_records_classes": (dict(cls=byte_set(b"a") + byte_set(b"\n"), cap=1, max_len=0),
                             "find_records_classes: class 1 of the pattern holds a delimiter (value 10)", False),
    "find_any": (dict(cls=None), "find_any: the classes, alt_lens and d_totals are required", True),
    "find_records_any": (dict(cls=None, lens=None, n=1, cap=1, max_len=0), "find_records_any: the classes, alt_lens and d_totals are required", True),
    "find_records_select": (dict(cls=None, lens=None, n=1, cap=1, max_len=0),
                            "find_records_select: the classes, alt_lens and d_totals are required", True),
    "find_records_context": (dict(cls=None), "find_records_context: the classes, alt_lens and d_totals are required", True),
    "find_any_anchored": (dict(cls=None), "find_any_anchored: the classes, alt_lens and d_totals are required", True),
    "find_records_anchored": (dict(cls=None), "find_records_anchored: the classes, alt_lens and d_totals are required", True),
}


def the_call_keeps_its_wording(lib, name):
    mistake, message, whole = WORDING[name]
    rc, msg = call(lib, name, **mistake)
    assert rc == HUFE_ARGUMENT and (msg == message if whole else msg.startswith(message)), msg


# ---- the any-of table ------------------------------------------------------------------------------------------------------
def table_ends(name):
    """tables at the ends of what is allowed: they reach the last check.  (An anchored call keeps a bit an alternative for the
    boundary - its own tests try that budget -, so it gets a table that fits either way)"""
    if "anchors" in CALLS[name]:
        return [alts_of([b"xy"] * 20, [b"x"] * 31)]
    return [alts_of([b"xy"]), alts_of([b"xy"] * 64), alts_of(*[[b"xy"]] * 64), alts_of([b"x"] * 31, [b"y"] * 33), alts_of([b"x"], [b"y"] * 63)]


def null_arrays_and_counts_of_0_and_65(lib, name, kw):
    prefix = who(name)
    for bad in (dict(cls=None), dict(lens=None), dict(cls=None, lens=None), dict(n=0), dict(n=65), dict(n=0xFFFFFFFF),
                dict(alts=alts_of(*[[b"x"]] * 65))):
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, **bad, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(prefix) and "needs a context" not in msg, (bad, msg)
    for nblocks, raw_size in LAYOUTS:
        for bad in (dict(cls=None), dict(lens=None), dict(totals=None)):
            assert "classes, alt_lens and d_totals are required" in call(lib, name, nblocks=nblocks, raw_size=raw_size, **bad, **kw)[1]
        assert "n_alts 0 is not 1 to 64" in call(lib, name, nblocks=nblocks, raw_size=raw_size, n=0, **kw)[1]
        assert "n_alts 65 is not 1 to 64" in call(lib, name, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*[[b"x"]] * 65), **kw)[1]
    for alts in table_ends(name):
        assert valid(*call(lib, name, alts=alts, **kw), prefix)


SIXTY_FOUR = b"".join([byte_set(b"ab")] * 64)


def an_alternative_of_length_0(lib, name, kw, lens, at):
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, cls=SIXTY_FOUR, lens=np.array(lens, np.uint32).tobytes(), n=len(lens), **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who(name)) and "needs a context" not in msg, msg
        assert f"alternative {at} has length 0" in msg


def a_total_above_64(lib, name, kw, lens):
    """(the classes are never read past their end: the total is looked at first)"""
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, cls=SIXTY_FOUR, lens=np.array(lens, np.uint32).tobytes(), n=len(lens), **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who(name)) and "needs a context" not in msg, msg
        assert f"sum to {sum(lens)}" in msg and "above 64" in msg


def an_empty_class(lib, name, kw, lens, j, k):
    alts = [[b"ab"] * m for m in lens]
    alts[j][k] = b""
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts), **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who(name)) and "is empty" in msg and "needs a context" not in msg, msg
        assert f"class {k} of alternative {j} " in msg


def a_class_that_meets_the_delimiter_set(lib, name, kw, lens, j, k):
    """a records call refuses it; a positions call has no delimiters, or may look for one"""
    alts = [[b"ab"] * m for m in lens]
    alts[j][k] = b"a\nz"
    prefix = who(name)
    for nblocks, raw_size in LAYOUTS:
        rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts), **kw)
        if name not in RECORD_CALLS:
            assert valid(rc, msg, prefix)
            continue
        assert rc == HUFE_ARGUMENT and msg.startswith(prefix) and "holds a delimiter" in msg, msg
        assert "needs a context" not in msg and f"class {k} of alternative {j} " in msg and "(value 10)" in msg
        assert valid(*call(lib, name, nblocks=nblocks, raw_size=raw_size, alts=alts_of(*alts), delims=byte_set(b"\r\x00"), **kw), prefix)
    if name in RECORD_CALLS:
        rc, msg = call(lib, name, alts=alts_of([b"a"], [b"b", [3, 255]]), delims=byte_set([255]), **kw)
        assert rc == HUFE_ARGUMENT and "class 1 of alternative 1 holds a delimiter (value 255)" in msg


def the_full_class_and_the_delimiter_set(lib, name, kw):
    prefix = who(name)
    for alts, j, k in (((FULL + byte_set(b"a"), np.array([1, 1], np.uint32).tobytes(), 2), 0, 0),
                       ((byte_set(b"a") + byte_set(b"b") + FULL, np.array([1, 2], np.uint32).tobytes(), 2), 1, 1)):
        if name not in RECORD_CALLS:
            assert valid(*call(lib, name, alts=alts, **kw), prefix)
            continue
        for nblocks, raw_size in LAYOUTS:
            rc, msg = call(lib, name, nblocks=nblocks, raw_size=raw_size, alts=alts, **kw)
            assert rc == HUFE_ARGUMENT and "holds a delimiter" in msg and f"class {k} of alternative {j} " in msg and "(value 10)" in msg
            assert "needs a context" not in msg and msg.startswith(prefix)
        assert valid(*call(lib, name, alts=alts, delims=EMPTY, **kw), prefix)      # the empty delimiter set: valid

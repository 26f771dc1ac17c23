"""hufgpu_find_any_quant and hufgpu_find_records_quant: their declarations, every argument error - the new ones and the older
calls' in the new wording, each with no context at all -, the NumPy models of their results, GpuCodec.Opt / Rep /
quant_classes and GpuCodec.regex (no GPU needed).  The models are checked against Python's `re` on `bytes`: the alternation of
the alternatives, an optional position a '?', under a look-ahead for the positions - the shortest form at a start, which
decides on the served rule, is the shortest slice that re.fullmatch takes -, bytes.split and re.search for the records.
"""
import re

import numpy as np
import pytest

from find_any_model import find_any_model
from find_args_support import HUFE_ARGUMENT, LAYOUTS, NEWLINE, alts_of, bracket, declaration, lib, members, valid  # noqa: F401
from find_context_model import find_context_model
from find_quant_model import find_quant_model, find_quant_records_model
from find_quant_support import COLOUR, NAMES, OLDER, POS_NAME, REC_NAME, SLOTS, O, arrays, call, forms, lit, rep
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec

AnyOf, Opt, Rep = GpuCodec.AnyOf, GpuCodec.Opt, GpuCodec.Rep
EACH = pytest.mark.parametrize("name", NAMES, ids=["positions", "records"])


# ---- the symbols ---------------------------------------------------------------------------------------------------------
@EACH
def test_symbols_are_exported_and_declared(lib, name):
    """the older call's argument list with `const uint8_t *optional` behind n_alts"""
    symbol = "hufgpu_" + name
    assert symbol in _native.GPU_SYMBOLS and hasattr(lib, symbol)
    older = getattr(lib, "hufgpu_" + OLDER[name]).argtypes
    assert len(getattr(lib, symbol).argtypes) == len(SLOTS[name]) == len(older) + 1
    header, m = declaration(name)
    _, s = declaration(OLDER[name])
    want = re.sub(r"\s+", " ", s.group(1)).replace("uint32_t n_alts,", "uint32_t n_alts, const uint8_t *optional,")
    assert m and want == re.sub(r"\s+", " ", m.group(1))
    assert "OUT OF SCOPE: anchors together with optional positions" in header


# ---- the new errors ------------------------------------------------------------------------------------------------------
@EACH
def test_valid_arguments_still_need_a_context(lib, name):
    for kw in ({}, {"opt": None}, {"opt": bytes(9)}, {"cap": 0, "pos": None, "rlens": None} if name == REC_NAME else {"cap": 0, "pos": None}):
        assert valid(*call(lib, name, **kw), name + ":"), kw
    for nblocks, raw_size in LAYOUTS:
        assert valid(*call(lib, name, nblocks=nblocks, raw_size=raw_size), name + ":")


@EACH
@pytest.mark.parametrize("at,value", [(0, 2), (4, 255), (5, 7), (6, 2), (8, 128)])
def test_an_optional_byte_above_1(lib, name, at, value):
    opt = bytearray(arrays(COLOUR)[3])
    opt[at] = value
    j, k = (0, at) if at < 6 else (1, at - 6)
    rc, msg = call(lib, name, opt=bytes(opt))
    assert rc == HUFE_ARGUMENT and msg.startswith(name + ": optional is %d at position %d of alternative %d" % (value, k, j)), msg


@EACH
@pytest.mark.parametrize("quant,j", [([[O(b"a")]], 0), ([lit(b"ab"), [O(b"a"), O(b"b"), O(b"c")]], 1), ([rep(b"x", 0, 64)], 0),
                                     ([lit(b"ab", (0, 1)), lit(b"cd")], 0)])
def test_an_alternative_that_is_all_optional(lib, name, quant, j):
    cls, lens, n, _ = arrays([[c[0] if isinstance(c, tuple) else c for c in a] for a in quant])
    opt = b"".join(bytes([int(isinstance(c, tuple)) for c in a]) for a in quant)
    rc, msg = call(lib, name, alts=(cls, lens, n), opt=opt)
    assert rc == HUFE_ARGUMENT and msg.startswith(name + ": every position of alternative %d is optional: it would match everywhere" % j), msg


# ---- the older calls' errors in the new wording, in their order ---------------------------------------------------------------
@EACH
def test_the_table_errors_come_first_and_keep_their_order(lib, name):
    who = name + ":"
    bad_opt = bytes([2] * 9)
    cls, lens, n, _ = arrays(COLOUR)
    for kw, words in (({"cls": None}, "the classes, alt_lens and d_totals are required"),
                      ({"lens": None}, "the classes, alt_lens and d_totals are required"),
                      ({"n": 0}, "n_alts 0 is not 1 to 64"), ({"n": 65}, "n_alts 65 is not 1 to 64"),
                      ({"alts": alts_of([b"a"], [], [b"b"])}, "alternative 1 has length 0"),
                      ({"alts": (cls * 8, np.array([32, 33], np.uint32).tobytes(), 2)}, "the lengths of the 2 alternatives sum to 65, above 64"),
                      ({"alts": alts_of([b"a", b""], [b"b"])}, "class 1 of alternative 0 is empty")):
        rc, msg = call(lib, name, opt=bad_opt * 8, **kw)           # (the bad `optional` is not reached, or not read)
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and words in msg, (kw.keys(), msg)
    rc, msg = call(lib, name, opt=bad_opt, totals=None)             # behind the table, in front of the older call's other checks
    assert rc == HUFE_ARGUMENT and "optional is 2 at position 0 of alternative 0" in msg
    for kw, words in (({"totals": None}, "the classes, alt_lens and d_totals are required"),
                      ({"stream": None}, "the stream, its block index and d_block_errs are required"),
                      ({"index": None}, "the stream, its block index and d_block_errs are required"),
                      ({"errs": None}, "the stream, its block index and d_block_errs are required"),
                      ({"sub": None}, "needs the stream's sub-index in an 8-byte aligned buffer"),
                      ({"sub": 0x30004}, "needs the stream's sub-index in an 8-byte aligned buffer"),
                      ({"raw_size": 4 * 4096 + 1}, "must be those of the encode that wrote these 4 blocks"),
                      ({"nblocks": 0}, "must be those of the encode that wrote these 0 blocks"),
                      ({"pos": None}, "needs d_rec_pos and d_rec_len" if name == REC_NAME else "pos_cap 16 needs d_pos")):
        rc, msg = call(lib, name, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and words in msg, (kw, msg)


def test_the_records_call_has_the_context_calls_checks(lib):
    who = REC_NAME + ":"
    rc, msg = call(lib, REC_NAME, select=2, cls=None, opt=bytes([2] * 9))
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " select 0x2 has a bit other than HUFGPU_SELECT_INVERT")
    rc, msg = call(lib, REC_NAME, delims=None)
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " the delim_set is required")
    rc, msg = call(lib, REC_NAME, rlens=None)
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " rec_cap 16 needs d_rec_pos and d_rec_len")
    rc, msg = call(lib, REC_NAME, quant=[[b"a", O(b"\n")]])
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " class 1 of alternative 0 holds a delimiter (value 10)")
    assert valid(*call(lib, POS_NAME, quant=[[b"a", O(b"\n")]]), POS_NAME + ":")     # (the positions' call has no delimiters)
    for kw in ({"select": 1}, {"ba": (0, 0)}, {"ba": (2**32 - 1, 2**32 - 1)}, {"no": None}, {"sel": None}, {"max_len": 0}):
        assert valid(*call(lib, REC_NAME, **kw), who), kw


# ---- Opt, Rep and quant_classes ------------------------------------------------------------------------------------------
def test_quant_classes():
    colour = list(b"colo") + [Opt(b"u"), ord("r")]
    assert "Opt(" in repr(Opt(b"u")) and "Rep(" in repr(Rep(b"x", 1, 2))
    classes, lens, optional = GpuCodec.quant_classes(colour)
    assert classes.dtype == np.uint8 and lens.dtype == np.uint32 and optional.dtype == np.uint8
    assert lens.tolist() == [6] and optional.tolist() == [0, 0, 0, 0, 1, 0]
    assert np.array_equal(classes, GpuCodec.byte_classes(b"colour"))
    classes, lens, optional = GpuCodec.quant_classes(AnyOf(colour, b"ab", [Rep(b"09", 1, 3), ord("."), Rep({1, 2}, 2, 2), Rep(7, 0, 2), 8]))
    assert lens.tolist() == [6, 2, 9] and optional.tolist() == [0, 0, 0, 0, 1, 0] + [0, 0] + [0, 1, 1, 0, 0, 0, 1, 1, 0]
    assert [members(r) for r in classes[8:]] == [[48, 57]] * 3 + [[46], [1, 2], [1, 2], [7], [7], [8]]
    classes, _, _ = GpuCodec.quant_classes([Opt(b"a"), ord("b")], ignore_case=True)
    assert [members(r) for r in classes] == [[65, 97], [66, 98]]
    classes, lens, optional = GpuCodec.quant_classes([Rep(b"x", 1, 64)])
    assert classes.shape == (64, 32) and optional.tolist() == [0] + [1] * 63
    plain = GpuCodec.quant_classes(AnyOf(b"ERROR", [b"fF", 1]))
    assert not plain[2].any() and all(np.array_equal(a, b) for a, b in zip(plain[:2], GpuCodec.alt_classes(AnyOf(b"ERROR", [b"fF", 1]))))


def test_quant_classes_errors():
    for bad, words in (([Rep(b"x", 3, 2)], "alternative 0, item 0: Rep from 3 to 2"), ([1, Rep(b"x", -1, 2)], "alternative 0, item 1"),
                       (AnyOf(b"a", [1, Rep(b"x", 0, 0)]), "alternative 1, item 1: Rep of at most 0 copies"),
                       ([Rep(b"x", 1, 65)], "alternative 0, item 0: the positions come to 65, above 64"),
                       (AnyOf([Rep(b"x", 1, 60)], [1, 2, Opt(3), 4, 5]), "sum to 65"),
                       (AnyOf(b"ab", [Opt(1), Rep(2, 0, 3)]), "alternative 1: every position is optional"),
                       ([1, Opt(b"")], "class 1 "), (AnyOf(b"a", [Opt(1), 2, Rep(b"", 1, 2)]), "alternative 1: class 2 "),
                       (AnyOf(b"a", []), "alternative 1 has length 0")):
        with pytest.raises(ValueError, match=re.escape(words)):
            GpuCodec.quant_classes(bad)
    with pytest.raises(TypeError):
        GpuCodec.quant_classes("text")


def test_the_routes():
    colour = list(b"colo") + [Opt(b"u"), ord("r")]
    for pattern in (colour, AnyOf(b"x", colour), [Rep(b"ab", 2, 2)]):
        route, key, st = GpuCodec._find_route(pattern, False, b"\n")
        assert route == "quant" and len(key) == 4 and len(key[3]) * 32 == len(key[0]) and st == NEWLINE
        assert GpuCodec._find_route(pattern, False, b"\n", True)[0] == "quant"
        assert GpuCodec._find_route(pattern, False, anchors=(False, False, False, False, None))[:1] == ("quant",)
        for anchors in ((True, False, False, False, None), (False, True, False, False, None), (False, False, True, False, None),
                        (False, False, False, True, None)):
            with pytest.raises(ValueError, match="do not go with Opt / Rep"):
                GpuCodec._find_route(pattern, False, b"\n", False, anchors)
        for terms in (GpuCodec.AllOf(b"a", pattern), GpuCodec.Seq(pattern, b"b")):
            with pytest.raises(ValueError, match="holds an Opt or a Rep"):
                GpuCodec._find_terms(terms, False, b"\n", (False, False, False, False, None))
    with pytest.raises(ValueError, match="class 1 of alternative 1 holds a delimiter"):
        GpuCodec._find_route(AnyOf(b"x", [1, Opt(b"\n")]), False, b"\n")
    # every pattern without Opt / Rep makes the call it made before
    assert GpuCodec._find_route(b"abc", False)[0] == "literal" and GpuCodec._find_route([1, 2], False)[0] == "classes"
    assert GpuCodec._find_route(AnyOf(b"a", [1, 2]), False)[0] == "any" and len(GpuCodec._find_route(AnyOf(b"a"), False)[1]) == 3


# ---- the models against re -----------------------------------------------------------------------------------------------
def text(alt):
    """one alternative as a regular expression; a run of optional positions of one class is written x{0,k}, which `re` takes
    without trying every subset of the run"""
    out, k = b"", 0
    while k < len(alt):
        c = alt[k]
        if not isinstance(c, tuple):
            out += bracket(c)
            k += 1
            continue
        run = 1
        while k + run < len(alt) and alt[k + run] == c:
            run += 1
        out += bracket(c[0]) + b"{0,%d}" % run
        k += run
    return out


def re_quant_positions(data, alts, blocksize, cap=0, served=None):
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    each = [re.compile(text(a), re.DOTALL) for a in alts]
    look = re.compile(b"(?=(?:" + b"|".join(b"(?:" + text(a) + b")" for a in alts) + b"))", re.DOTALL)
    pos, counts = [], [0] * nb
    for hit in look.finditer(raw):
        p = hit.start()
        shortest = next(m for m in range(1, 65) if any(r.fullmatch(raw, p, p + m) for r in each))
        if all(served[b] for b in range(p // bs, (p + shortest - 1) // bs + 1)):
            pos.append(p)
            counts[p // bs] += 1
    written = min(len(pos), cap)
    return pos[:written], counts, [len(pos), written, nb - sum(served), 0]


def re_quant_records(data, alts, delims, blocksize, cap=0, max_len=0, served=None):
    """tests/find_args_support.py's re_records with the alternation of the quantified alternatives"""
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    pieces = raw.split(bytes(delims)) if delims else [raw]
    want = re.compile(b"|".join(b"(?:" + text(a) + b")" for a in alts), re.DOTALL)
    pos, lens, counts, cut = [], [], [0] * nb, []
    s = 0
    for piece in pieces if n else []:
        e = s + len(piece)
        if want.search(piece) and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            pos.append(s)
            lens.append(min(e - s, clip))
            cut.append(e - s > clip)
            counts[s // bs] += 1
        s = e + 1
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])]


def same_positions(data, alts, blocksize, cap=0, served=None):
    got = find_quant_model(data, alts, blocksize, cap, served)
    want = re_quant_positions(data, alts, blocksize, cap, served)
    assert tuple(g.tolist() for g in got) == want, (alts, bytes(data), blocksize, served)
    return want


def same_records(data, alts, delims, blocksize, cap=0, max_len=0, served=None):
    got = find_quant_records_model(data, alts, delims, blocksize, cap, max_len, served)[:4]
    want = re_quant_records(data, alts, delims, blocksize, cap, max_len, served)
    assert tuple(g.tolist() for g in got) == want, (alts, bytes(data), blocksize, served)
    return want


def test_models_by_hand():
    data = np.frombuffer(b"color colour colouur ab b", np.uint8)
    colour = [lit(b"colour", (4,))]
    assert same_positions(data, colour, 4, cap=9) == ([0, 6], [1, 1, 0, 0, 0, 0, 0], [2, 2, 0, 0])
    assert same_positions(data, [[O(b"a"), b"b"]], 0, cap=9)[0] == [21, 22, 24]            # a leading a?: both starts of "ab"
    assert same_positions(data, [[b"o", O(b"u"), O(b"u")]], 0, cap=9)[0] == [1, 3, 7, 9, 14, 16]       # a trailing run: a start once
    # the long form reaches block 1, which is not served, the short one does not: the start stays; both reach it: dropped
    abc = [[b"a", b"b", O(b"c"), O(b"x")]]
    assert same_positions(np.frombuffer(b"abcxxx", np.uint8), abc, 3, cap=9, served=[True, False])[0] == [0]
    assert same_positions(np.frombuffer(b"xabcxx", np.uint8), abc, 3, cap=9, served=[True, False])[0] == [1]
    assert same_positions(np.frombuffer(b"xxabcx", np.uint8), abc, 3, cap=9, served=[True, False])[0] == []
    assert same_positions(np.frombuffer(b"xxabcx", np.uint8), [[b"a", O(b"q"), b"b", b"c"]], 3, cap=9, served=[True, False])[0] == []
    # a match at n - len_short where the long form would pass the end, none at n - len_min + 1
    assert same_positions(np.frombuffer(b"xxabab", np.uint8), [[b"a", b"b", O(b"a")]], 4, cap=9)[0] == [2, 4]
    assert same_positions(np.frombuffer(b"xxabaa", np.uint8), [[b"a", O(b"b"), b"a"]], 4, cap=9)[0] == [2, 4]
    # x{2,5} over runs of 1 to 7
    data = np.frombuffer(b"x.xx.xxx.xxxx.xxxxx.xxxxxx.xxxxxxx", np.uint8)
    assert same_positions(data, [rep(b"x", 2, 5)], 5, cap=99)[2][0] == sum(range(1, 7))
    data = np.frombuffer(b"took 5ms\ntook ms\n\ntook 123456ms and took 77ms\nms", np.uint8)
    took = [lit(b"took ") + rep(b"0123456789", 1, 5) + lit(b"ms")]
    assert same_records(data, took, b"\n", 8, cap=9, max_len=10) == ([0, 18], [8, 10], [1, 0, 1, 0, 0, 0], [2, 2, 0, 1])
    assert find_quant_records_model(data, took, b"\n", 8, cap=9, invert=True)[0].tolist() == [9, 46]
    got = find_quant_records_model(data, took, b"\n", 8, cap=9, before=1)
    assert all(np.array_equal(g, w) for g, w in zip(got, find_context_model(data, [lit(b"took 5ms"), lit(b"took 77ms")], b"\n", 8, cap=9, before=1)))


def flags_of(kind, m, rng):
    if kind == "none":
        return [False] * m
    if kind in ("first", "middle", "last"):
        at = {"first": 0, "middle": m // 2, "last": m - 1}[kind]
        return [k == at for k in range(m)]
    if kind == "alternating":
        return [k % 2 == 1 for k in range(m)]
    at = int(rng.integers(0, m))                            # all but one
    return [k != at for k in range(m)]


def alternative(rng, values, flags):
    """classes for the flags: required positions narrow, a run of optional positions of ONE narrow class (`re` is then quick
    where nothing matches), all of it without the last value, the delimiter"""
    alt, k = [], 0
    while k < len(flags):
        cls = bytes(sorted(set(int(v) for v in rng.choice(values[:-1], int(rng.integers(1, 3))))))
        if not flags[k]:
            alt.append(cls)
            k += 1
            continue
        while k < len(flags) and flags[k]:
            alt.append(O(cls))
            k += 1
    return alt


def random_form(rng, alt):
    return bytes(int(rng.choice(list(c[0] if isinstance(c, tuple) else c))) for c in alt if not isinstance(c, tuple) or rng.integers(0, 2))


def quant_case(rng, alts, values, trial):
    """noise with forms of the alternatives in it, whole and cut, and lines; every other trial has room for a whole form"""
    n, bs = int(rng.integers(1 if trial % 2 else 70, 500)), int(rng.integers(0, 90))
    data = rng.choice(values, n).astype(np.uint8)
    data[rng.integers(0, n, n // 40 + 1)] = values[-1]
    for i in range(int(rng.integers(1, 12)), -1, -1):               # (the last one is whole where there is room)
        form = np.frombuffer(random_form(rng, alts[int(rng.integers(0, len(alts)))]), np.uint8)
        at = int(rng.integers(0, n if i or trial % 2 else n - form.size))
        form = form[:n - at]
        data[at:at + form.size] = form
    if trial % 2:
        data[n - 1] = values[-1]
    return data, n, bs


def check_case(rng, alts, values, trials):
    hits = 0
    for trial in range(trials):
        data, n, bs = quant_case(rng, alts, values, trial)
        nb = (n + (bs or n) - 1) // (bs or n)
        for served in (None, rng.integers(0, 5, nb) != 0):
            cap = int(rng.integers(0, 50))
            hits += same_positions(data, alts, bs, cap=cap, served=served)[2][0]
            for delims in (bytes([int(values[-1])]), b""):
                hits += same_records(data, alts, delims, bs, cap=cap, max_len=int(rng.integers(0, 12)), served=served)[3][0]
    assert hits > 0, "no trial had a match"


ALPHABETS = {"four letters": np.array([97, 98, 99, 10]), "all values": np.concatenate([np.arange(10), np.arange(11, 256), [10]])}
ONE = [(m, kind) for m in (1, 2, 5, 33, 64) for kind in ("none", "first", "middle", "last", "alternating", "all but one")
       if (m > 1 or kind == "none") and not (m == 2 and kind in ("middle", "all but one"))]


@pytest.mark.parametrize("m,kind", ONE, ids=lambda v: str(v).replace(" ", "_"))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_models_of_one_alternative(m, kind, alphabet):
    rng = np.random.default_rng(1000 * m + len(kind) + len(alphabet))
    values = ALPHABETS[alphabet]
    for _ in range(3):
        flags = flags_of(kind, m, rng)
        if m == 2 and kind == "alternating":
            flags = [False, True]
        check_case(rng, [alternative(rng, values, flags)], values, 4)


def few_runs(rng, m):
    """random flags: single positions in a short alternative, a few runs in a long one; never all of them"""
    if m == 1:
        return [False]
    flags = [bool(rng.integers(0, 2)) for _ in range(m)] if m <= 5 else [False] * m
    for _ in range(3 if m > 5 else 0):
        at, run = int(rng.integers(0, m)), int(rng.integers(1, 9))
        flags[at:at + run] = [True] * len(flags[at:at + run])
    if all(flags):
        flags[int(rng.integers(0, m))] = False
    return flags


@pytest.mark.parametrize("mix", [(2, 5, 33), (31, 33), (32, 32), (1, 63)], ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_models_of_several_alternatives(mix, alphabet):
    rng = np.random.default_rng(100 * sum(mix) + len(mix) + len(alphabet))
    values = ALPHABETS[alphabet]
    for _ in range(3):
        check_case(rng, [alternative(rng, values, few_runs(rng, m)) for m in mix], values, 4)


def test_with_no_flag_set_the_models_are_the_any_of_models():
    rng = np.random.default_rng(23)
    values = ALPHABETS["four letters"]
    for trial in range(40):
        alts = [alternative(rng, values, [False] * int(rng.integers(1, 7))) for _ in range(int(rng.integers(1, 5)))]
        data, n, bs = quant_case(rng, alts, values, trial)
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 5, nb) != 0
        cap = int(rng.integers(0, 60))
        got, want = find_quant_model(data, alts, bs, cap, served), find_any_model(data, alts, bs, cap, served)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        got = find_quant_records_model(data, alts, b"\n", bs, cap, 5, served, trial % 2 == 1, 1, 2)
        want = find_context_model(data, alts, b"\n", bs, cap, 5, served, trial % 2 == 1, 1, 2)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_written_out_forms_give_the_same_positions():
    rng = np.random.default_rng(29)
    values = ALPHABETS["four letters"]
    for trial in range(30):
        alts = [alternative(rng, values, few_runs(rng, int(rng.integers(1, 6)))) for _ in range(int(rng.integers(1, 3)))]
        data, n, bs = quant_case(rng, alts, values, trial)
        served = rng.integers(0, 5, (n + (bs or n) - 1) // (bs or n)) != 0
        written = forms(alts)
        if sum(len(f) for f in written) <= 64 and len(written) <= 64:
            assert all(np.array_equal(g, w) for g, w in zip(find_quant_model(data, alts, bs, 40, served), find_any_model(data, written, bs, 40, served)))


# ---- regex() -------------------------------------------------------------------------------------------------------------
def items_of(pattern):
    """an AnyOf of lists with Opt / Rep items as the models take it"""
    out = []
    for alt in pattern:
        items = []
        for c in alt:
            items += rep(c.cls, c.lo, c.hi) if isinstance(c, Rep) else [O(c.cls)] if isinstance(c, Opt) else [c]
        out.append(items)
    return out


def starts_of(expr, data, flags=re.DOTALL):
    return [m.start() for m in re.finditer(b"(?=(?:" + expr + b"))", bytes(data), flags)]


def test_regex_by_hand():
    rx = GpuCodec.regex
    assert repr(rx(rb"colou?r")) == repr(AnyOf([b"c", b"o", b"l", b"o", Opt(b"u"), b"r"]))
    assert repr(rx(rb"https?://|ftp")) == repr(AnyOf([b"h", b"t", b"t", b"p", Opt(b"s"), b":", b"/", b"/"], [b"f", b"t", b"p"]))
    assert repr(rx(rb"[0-9]{1,3}\.x{2}y{,2}")) == repr(AnyOf([Rep(b"0123456789", 1, 3), b".", Rep(b"x", 2, 2), Rep(b"y", 0, 2)]))
    assert repr(rx(rb"\n\t\r\x41\\\?\|\.")) == repr(AnyOf([b"\n", b"\t", b"\r", b"A", b"\\", b"?", b"|", b"."]))
    digits, word = b"0123456789", GpuCodec.WORD_BYTES
    (alt,) = rx(rb"\d\w\s\D\W\S.")
    assert alt[0] == digits and set(alt[1]) == set(word) and alt[2] == b"\t\n\x0b\x0c\r "
    assert set(alt[3]) == set(range(256)) - set(digits) - {10} and set(alt[4]) == set(range(256)) - set(word) - {10}
    assert set(alt[5]) == set(range(256)) - set(b" \t\n\r\f\v") and set(alt[6]) == set(range(256)) - {10}
    (alt,) = rx(rb"[abc][a-c0-2_][^a-y][]x][^]x][a-][\d.][|.?*+(){}^$]")
    assert alt[:2] == [b"abc", b"012_abc"] and set(alt[2]) == set(range(256)) - set(range(97, 122)) - {10}
    assert alt[3] == b"]x" and set(alt[4]) == set(range(256)) - set(b"]x\n") and alt[5] == b"-a" and alt[6] == b".0123456789"
    assert set(alt[7]) == set(b"|.?*+(){}^$")
    (alt,) = rx(rb".[^a]\D", delimiters=b"\n;")
    assert all(10 not in c and 59 not in c for c in alt)
    (alt,) = rx(rb".[^a]", delimiters=b"")
    assert len(alt[0]) == 256 and len(alt[1]) == 255
    (alt,) = rx(rb"a[b-d]{2}\x4a?", ignore_case=True)
    assert alt[0] == b"Aa" and alt[1].cls == b"BCDbcd" and alt[2].cls == b"Jj"
    assert len(GpuCodec.quant_classes(rx(rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"))[2]) == 15
    assert GpuCodec.quant_classes(rx(b"a{64}"))[1].tolist() == [64]
    data = np.frombuffer(b"10.0.0.1 and 192.168.1.254, not 1.2.3 or .1.2.3.4", np.uint8)
    address = rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}"
    assert find_quant_model(data, items_of(rx(address)), 0, 99)[0].tolist() == starts_of(address, data)


ATOMS = [b"a", b"b", b"c", b"d", rb"\.", rb"\?", b".", b"[ab]", b"[^a]", b"[a-c]", b"[^b-d.]", rb"\d", rb"\w", rb"\D", rb"\S", rb"\x61", b"[]a]",
         rb"[\d_]", b"_", b" "]
QUANTS = [b"", b"", b"", b"?", b"{2}", b"{1,3}", b"{,2}", b"{0,1}", b"{2,2}"]


def test_regex_on_random_expressions():
    rng = np.random.default_rng(31)
    letters = np.frombuffer(b"abcd01._? \n", np.uint8)
    hits = tried = 0
    while tried < 400:
        alts = []
        for _ in range(int(rng.integers(1, 4))):
            parts = [ATOMS[int(rng.integers(0, len(ATOMS)))] + QUANTS[int(rng.integers(0, len(QUANTS)))] for _ in range(int(rng.integers(1, 6)))]
            alts.append(b"".join(parts))
        expr = b"|".join(alts)
        ignore_case = tried % 5 == 0
        try:
            pattern = GpuCodec.regex(expr, delimiters=b"", ignore_case=ignore_case)
        except ValueError as e:
            assert "every position of the alternative is optional" in str(e), (expr, e)
            continue
        tried += 1
        data = rng.choice(letters, int(rng.integers(1, 120))).astype(np.uint8)
        if ignore_case:
            data = np.where(rng.integers(0, 2, data.size) == 1, np.frombuffer(bytes(data).upper(), np.uint8), data)
        want = starts_of(expr, data, re.DOTALL | (re.IGNORECASE if ignore_case else 0))
        got = find_quant_model(data, items_of(pattern), 0, data.size)[0].tolist()
        assert got == want, (expr, bytes(data))
        hits += len(want)
    assert hits > 1000


@pytest.mark.parametrize("expr,at,words", [
    (rb"ab*", 2, "unbounded"), (rb"a+b", 1, "unbounded"), (rb"abc{2,}", 3, "unbounded: not in this matcher"), (rb"a(b)", 1, "groups"),
    (rb"ab)", 2, "groups"), (rb"^ab", 0, "anchors"), (rb"ab$", 2, "anchors"), (rb"?ab", 0, "nothing to repeat"), (rb"a|*b", 2, "nothing to repeat"),
    (rb"a|{2}", 2, "nothing to repeat"), (rb"ab??", 3, "nothing to repeat"), (rb"ab{2}{3}", 5, "nothing to repeat"), (rb"ab?+", 3, "nothing to repeat"),
    (rb"x[z-a]", 2, "bad range"), (rb"[a-\d]", 1, "bad range"), (rb"ab[cd", 2, "without its ']'"), (rb"ab[", 2, "without its ']'"),
    (rb"a{x}", 1, "bad '{...}'"), (rb"a{1,2,3}", 1, "bad '{...}'"), (rb"a{1", 1, "bad '{...}'"), (rb"a{}", 1, "bad '{...}'"),
    (rb"a{3,2}", 1, "from 3 to 2"), (rb"a{0}", 1, "at most 0 copies"), (rb"a{,0}", 1, "at most 0 copies"), (rb"ab\q", 2, "escape"),
    (rb"ab\x4", 2, "hex"), (b"ab\\", 2, "at the end"), (rb"[\D]", 1, "inside a set"), (rb"a||b", 2, "empty alternative"), (rb"|a", 0, "empty alternative"),
    (rb"a|", 2, "empty alternative"), (b"", 0, "empty alternative"), (rb"ab|c?d{,3}", 3, "every position of the alternative is optional"),
    (rb"a{65}", 0, "come to 65, above 64"), (rb"a{60}|bcdef", 10, "come to 65, above 64"), (b"a" * 64 + b"|b", 65, "come to 65, above 64")])
def test_regex_rejects(expr, at, words):
    with pytest.raises(ValueError, match=re.escape(f"offset {at}: ")) as e:
        GpuCodec.regex(expr)
    assert words in str(e.value), e.value

"""hufgpu_find_any_expr and hufgpu_find_records_expr: their declarations, every argument error - the new ones, each in its
place in the order, and the older calls' in the new wording, each with no context at all -, the NumPy models of their
results, GpuCodec.Expr / expr_arrays and GpuCodec.egrep (no GPU needed).  The models are checked against Python's `re` on
`bytes`: for the positions the alternation of the alternatives under a look-ahead, between '(?:^|(?<=\\n))', '(?:$|(?=\\n))' and
'(?<!\\w)...(?!\\w)' for the anchors; for the records bytes.split and re.search of 'A[^\\n]*B' a line.
"""
import itertools
import re

import numpy as np
import pytest

from find_anchor_model import find_any_anchored_model, find_records_anchored_model
from find_args_support import HUFE_ARGUMENT, LAYOUTS, alts_of, declaration, lib, valid  # noqa: F401
from find_expr_model import ALL, BOL, EOL, ORDERED, WORD, find_any_expr_model, find_records_expr_model
from find_expr_support import COLOUR, NAMES, POS_NAME, REC_NAME, SLOTS, TOOK, O, arrays, call, counts_of, lit, rep
from find_quant_model import find_quant_model, find_quant_records_model
from find_terms_model import find_terms_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec
from test_find_quant_args import text

AnyOf, Opt, Rep, Expr = GpuCodec.AnyOf, GpuCodec.Opt, GpuCodec.Rep, GpuCodec.Expr
EACH = pytest.mark.parametrize("name", NAMES, ids=["positions", "records"])
W = GpuCodec.WORD_BYTES
ANCHORS = list(range(8))


# ---- the symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(lib):
    """the anchored positions call with `optional` behind n_alts; the context call with `optional`, the terms' three and the
    anchors' two behind n_alts"""
    for name in NAMES:
        symbol = "hufgpu_" + name
        assert symbol in _native.GPU_SYMBOLS and hasattr(lib, symbol)
        assert len(getattr(lib, symbol).argtypes) == len(SLOTS[name])
    assert len(lib.hufgpu_find_any_expr.argtypes) == len(lib.hufgpu_find_any_anchored.argtypes) + 1
    assert len(lib.hufgpu_find_records_expr.argtypes) == len(lib.hufgpu_find_records_context.argtypes) + 6
    squeeze = lambda s: re.sub(r"\s+", " ", s)                      # noqa: E731
    header, m = declaration(POS_NAME)
    _, s = declaration("find_any_anchored")
    assert m and squeeze(m.group(1)) == squeeze(s.group(1)).replace("uint32_t n_alts,", "uint32_t n_alts, const uint8_t *optional,")
    _, m = declaration(REC_NAME)
    _, s = declaration("find_records_context")
    more = ("uint32_t n_alts, const uint8_t *optional, const uint32_t *term_alts, uint32_t n_terms, uint32_t terms_mode, "
            "const uint8_t word_set[32], uint32_t anchors,")
    assert m and squeeze(m.group(1)) == squeeze(s.group(1)).replace("uint32_t n_alts,", more)
    for words in ("anchors with HUFGPU_TERMS_ALL of several terms", "optional positions in a term", "anchors per alternative",
                  "\\b INSIDE a pattern", "unbounded repeats", "groups", "which form matched"):
        assert words in header[header.index("FIND, ONE grep -E LINE"):], words


# ---- valid arguments -----------------------------------------------------------------------------------------------------
@EACH
def test_valid_arguments_still_need_a_context(lib, name):
    for kw in ({}, {"opt": None}, {"opt": bytes(9)}, {"anchors": 7}, {"anchors": 1, "words": None}, {"anchors": 4},
               {"cap": 0, "pos": None, "rlens": None} if name == REC_NAME else {"cap": 0, "pos": None}):
        assert valid(*call(lib, name, **kw), name + ":"), kw
    assert valid(*call(lib, POS_NAME, delims=None, anchors=4), POS_NAME + ":")
    for nblocks, raw_size in LAYOUTS:
        assert valid(*call(lib, name, nblocks=nblocks, raw_size=raw_size), name + ":")


def test_valid_terms(lib):
    who = REC_NAME + ":"
    for kw in ({"expr": TOOK}, {"expr": TOOK, "anchors": 7}, {"expr": TOOK, "mode": ALL}, {"mode": ALL, "anchors": 7},
               {"expr": [[lit(b"ab", (1,))], [lit(b"cd", (0,)), lit(b"x")]], "mode": ALL},
               {"expr": [[lit(b"a")], [lit(b"bb"), lit(b"cc")], [lit(b"d"), lit(b"eee", (2,))]], "anchors": 3},
               {"expr": [[lit(b"a")]] * 4}, {"select": 1}, {"ba": (0, 0)}, {"no": None}, {"sel": None}, {"max_len": 0}):
        assert valid(*call(lib, REC_NAME, **kw), who), kw


# ---- the new errors ------------------------------------------------------------------------------------------------------
@EACH
@pytest.mark.parametrize("at,value", [(0, 2), (4, 255), (6, 2), (8, 128)])
@pytest.mark.parametrize("anchors", [0, 7])
def test_an_optional_byte_above_1(lib, name, at, value, anchors):
    opt = bytearray(arrays(COLOUR)[3])
    opt[at] = value
    j, k = (0, at) if at < 6 else (1, at - 6)
    rc, msg = call(lib, name, opt=bytes(opt), anchors=anchors)
    assert rc == HUFE_ARGUMENT and msg.startswith(name + ": optional is %d at position %d of alternative %d" % (value, k, j)), msg


@EACH
@pytest.mark.parametrize("quant,j", [([[O(b"a")]], 0), ([lit(b"ab"), [O(b"a"), O(b"b"), O(b"c")]], 1), ([rep(b"x", 0, 60)], 0)])
@pytest.mark.parametrize("anchors", [0, 6])
def test_an_alternative_that_is_all_optional(lib, name, quant, j, anchors):
    """also with a boundary position behind it, which is required: the alternative's OWN positions are what counts"""
    rc, msg = call(lib, name, expr=[quant], anchors=anchors)
    assert rc == HUFE_ARGUMENT and msg.startswith(name + ": every position of alternative %d is optional: it would match everywhere" % j), msg


@EACH
def test_the_anchors_errors(lib, name):
    who = name + ":"
    for bad in (8, 0x10, 0xffffffff):
        rc, msg = call(lib, name, anchors=bad)
        assert rc == HUFE_ARGUMENT and msg.startswith(who + " anchors 0x%x has a bit other than" % bad), msg
    for anchors in (4, 5, 7):
        rc, msg = call(lib, name, anchors=anchors, words=None)
        assert rc == HUFE_ARGUMENT and msg.startswith(who + " HUFGPU_ANCHOR_WORD needs the word_set"), msg
    for anchors in (1, 2, 3, 7):
        rc, msg = call(lib, name, anchors=anchors, delims=None)
        words = " HUFGPU_ANCHOR_BOL and HUFGPU_ANCHOR_EOL need the delim_set" if name == POS_NAME else " the delim_set is required"
        assert rc == HUFE_ARGUMENT and msg.startswith(who + words), msg


@EACH
def test_the_budget_of_one_term(lib, name):
    who = name + ":"
    fits = [[rep(b"x", 1, 31), rep(b"y", 2, 31)]]                   # 62 positions and two boundary positions
    over = [[rep(b"x", 1, 31), rep(b"y", 2, 32)]]
    for anchors in ANCHORS:
        assert valid(*call(lib, name, expr=fits, anchors=anchors), who), anchors
        rc, msg = call(lib, name, expr=over, anchors=anchors)
        if anchors & (EOL | WORD):
            assert rc == HUFE_ARGUMENT and msg.startswith(who + " the lengths of the 2 alternatives and one boundary position each sum to 65, above 64"), msg
        else:
            assert valid(rc, msg, who), anchors
    assert valid(*call(lib, name, expr=[[rep(b"x", 1, 64)]], anchors=BOL), who)


def test_the_budget_of_ordered_terms_counts_the_last_terms_alternatives(lib):
    who = REC_NAME + ":"
    head = [[lit(b"a" * 30)], [lit(b"b" * 15), lit(b"c" * 15)]]
    fits = head + [[rep(b"x", 1, 1), rep(b"y", 1, 1)]]             # 62 + 2
    assert valid(*call(lib, REC_NAME, expr=fits, anchors=7), who)
    assert valid(*call(lib, REC_NAME, expr=head + [[rep(b"x", 1, 2), rep(b"y", 1, 2)]], anchors=BOL), who)      # 64, no boundary position
    rc, msg = call(lib, REC_NAME, expr=head + [[rep(b"x", 1, 2), rep(b"y", 1, 1)]], anchors=EOL)
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " the lengths of the 5 alternatives and one boundary position for each of the last "
                                                  "term's 2 sum to 65, above 64"), msg


def test_the_terms_errors(lib):
    who = REC_NAME + ":"
    for kw, words in (({"mode": 2}, " terms_mode 2 is neither HUFGPU_TERMS_ALL (0) nor HUFGPU_TERMS_ORDERED (1)"),
                      ({"terms": None}, " term_alts is required"), ({"nt": 0}, " n_terms 0 is not 1 to 4"),
                      ({"nt": 5, "terms": counts_of(1, 1, 1, 1, 1)}, " n_terms 5 is not 1 to 4"),
                      ({"terms": counts_of(1, 0, 2), "nt": 3}, " term 1 has no alternative"),
                      ({"terms": counts_of(1, 1), "nt": 2}, " the 2 terms have 2 alternatives, and n_alts is 3")):
        rc, msg = call(lib, REC_NAME, expr=TOOK, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who + words), (kw, msg)
    unequal = [[lit(b"ab"), lit(b"abc")], [lit(b"x")]]
    rc, msg = call(lib, REC_NAME, expr=unequal)
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " the alternatives of term 0 have the lengths 2 and 3: an ordered call needs one length a term"), msg
    assert valid(*call(lib, REC_NAME, expr=unequal, mode=ALL), who)
    assert valid(*call(lib, REC_NAME, expr=unequal[::-1]), who)                         # the LAST term may have several lengths
    rc, msg = call(lib, REC_NAME, expr=[[lit(b"x")], [lit(b"ab"), lit(b"abc")], [lit(b"y")]])
    assert rc == HUFE_ARGUMENT and "term 1 have the lengths 2 and 3" in msg


def test_an_optional_position_in_front_of_another_term(lib):
    who = REC_NAME + ":"
    rc, msg = call(lib, REC_NAME, expr=[[lit(b"ab"), lit(b"cd", (1,))], [lit(b"x")]])
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " position 1 of alternative 1, in term 0, is optional: an ordered call allows optional "
                                                  "positions in its last term only"), msg
    rc, msg = call(lib, REC_NAME, expr=[[lit(b"ab")], [lit(b"cde", (0,))], [lit(b"x", ())]], anchors=3)
    assert rc == HUFE_ARGUMENT and msg.startswith(who + " position 0 of alternative 1, in term 1, is optional"), msg
    assert valid(*call(lib, REC_NAME, expr=[[lit(b"ab"), lit(b"cd", (1,))], [lit(b"x")]], mode=ALL), who)
    assert valid(*call(lib, REC_NAME, expr=[[lit(b"ab")], [lit(b"cde", (0,))]], anchors=3), who)
    assert valid(*call(lib, REC_NAME, expr=[[lit(b"ab"), lit(b"cd", (1,))], [lit(b"x")]], opt=None), who)       # (NULL: all required)


def test_anchors_with_all_of_several_terms(lib):
    who = REC_NAME + ":"
    for anchors in range(1, 8):
        rc, msg = call(lib, REC_NAME, expr=TOOK, mode=ALL, anchors=anchors)
        assert rc == HUFE_ARGUMENT and msg.startswith(who + " anchors 0x%x with HUFGPU_TERMS_ALL of 2 terms" % anchors), msg
        assert valid(*call(lib, REC_NAME, expr=COLOUR, mode=ALL, anchors=anchors), who)     # one term: either mode


def test_the_order_of_the_checks(lib):
    """select, the anchors' three, the terms' six, anchors with ALL, the table (the budget inside it), `optional`, an optional
    position in front of another term, then the older calls' other checks: each error hides the ones behind it"""
    who = REC_NAME + ":"
    front = [[lit(b"ab", (1,))], [lit(b"x")]]                       # an optional position in term 0
    two = bytes([2, 0, 0])
    steps = [({"select": 2}, "select 0x2"), ({"anchors": 8}, "anchors 0x8 has a bit"), ({"anchors": 4, "words": None}, "needs the word_set"),
             ({"mode": 2}, "terms_mode 2"), ({"terms": None}, "term_alts is required"), ({"nt": 5}, "n_terms 5"),
             ({"terms": counts_of(0, 2)}, "term 0 has no alternative"), ({"terms": counts_of(2, 1)}, "have 3 alternatives, and n_alts is 2"),
             ({"alts": alts_of([b"a", b"b"], [b"c"], [b"x"]), "terms": counts_of(2, 1)}, "have the lengths 2 and 1"),
             ({"mode": ALL, "anchors": 1}, "with HUFGPU_TERMS_ALL of 2 terms"), ({"n": 65, "terms": counts_of(64, 1)}, "n_alts 65 is not 1 to 64"),
             ({"alts": alts_of([b"a", b""], [b"x"])}, "class 1 of alternative 0 is empty"), ({"opt": two}, "optional is 2 at position 0"),
             ({}, "position 1 of alternative 0, in term 0, is optional"), ({"opt": None, "totals": None}, "d_totals are required")]
    for k, (kw, words) in enumerate(steps):                         # step k's error next to the one of every step behind it, one at a time
        for later, _ in steps[k + 1:] + [({}, "")]:
            values = dict(later, **kw)
            if k == 13:
                values.pop("opt", None)                             # (the pattern's own flags are step 13's error)
            if set(later) & set(kw) or ("n" in later and "terms" in kw) or ("mode" in values and values["mode"] == ALL and k < 9):
                continue                                            # (one slot cannot hold two errors)
            rc, msg = call(lib, REC_NAME, expr=front, **values)
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and words in msg, (k, values, msg)
    # the positions call: the anchors, the table, the budget, `optional`, the older checks
    who = POS_NAME + ":"
    over = arrays([[rep(b"x", 1, 32), rep(b"y", 2, 32)]])
    for kw, words in (({"anchors": 8, "n": 0, "opt": two}, "anchors 0x8"), ({"anchors": 2, "delims": None, "n": 0}, "need the delim_set"),
                      ({"anchors": 2, "n": 0, "opt": two}, "n_alts 0"), ({"anchors": 2, "alts": over[:3], "opt": bytes([2] * 64)}, "one boundary position each sum to 66"),
                      ({"anchors": 2, "opt": two, "totals": None}, "optional is 2"), ({"anchors": 2, "totals": None}, "d_totals are required")):
        rc, msg = call(lib, POS_NAME, **kw)
        assert rc == HUFE_ARGUMENT and msg.startswith(who) and words in msg, (kw, msg)


# ---- the older calls' errors in the new wording ----------------------------------------------------------------------------
@EACH
def test_the_older_errors_under_the_new_prefix(lib, name):
    who = name + ":"
    cls, lens, n, _, _, _ = arrays(COLOUR)
    for kw, words in (({"cls": None}, "the classes, alt_lens and d_totals are required"),
                      ({"lens": None}, "the classes, alt_lens and d_totals are required"),
                      ({"n": 0}, "n_alts 0 is not 1 to 64" if name == POS_NAME else "have 2 alternatives, and n_alts is 0"),
                      ({"alts": alts_of([b"a"], [], [b"b"]), **({"terms": counts_of(3)} if name == REC_NAME else {})}, "alternative 1 has length 0"),
                      ({"alts": (cls * 8, np.array([32, 33], np.uint32).tobytes(), 2), "opt": None}, "the lengths of the 2 alternatives sum to 65, above 64"),
                      ({"alts": alts_of([b"a", b""], [b"b"]), "opt": None}, "class 1 of alternative 0 is empty"),
                      ({"totals": None}, "the classes, alt_lens and d_totals are required"),
                      ({"stream": None}, "the stream, its block index and d_block_errs are required"),
                      ({"errs": None}, "the stream, its block index and d_block_errs are required"),
                      ({"sub": None}, "needs the stream's sub-index in an 8-byte aligned buffer"),
                      ({"sub": 0x30004}, "needs the stream's sub-index in an 8-byte aligned buffer"),
                      ({"raw_size": 4 * 4096 + 1}, "must be those of the encode that wrote these 4 blocks"),
                      ({"nblocks": 0}, "must be those of the encode that wrote these 0 blocks"),
                      ({"pos": None}, "needs d_rec_pos and d_rec_len" if name == REC_NAME else "pos_cap 16 needs d_pos")):
        for anchors in (0, 7):
            rc, msg = call(lib, name, anchors=anchors, **kw)
            assert rc == HUFE_ARGUMENT and msg.startswith(who) and words in msg, (kw, anchors, msg)
    if name == REC_NAME:
        for expr, words in (([[[b"a", O(b"\n")]]], " class 1 of alternative 0 holds a delimiter (value 10)"),
                            ([[lit(b"ab")], [lit(b"c"), [b"d", O(b"x\n")]]], " class 1 of alternative 2 holds a delimiter (value 10)")):
            rc, msg = call(lib, name, expr=expr, anchors=3)
            assert rc == HUFE_ARGUMENT and msg.startswith(who + words), msg
        rc, msg = call(lib, name, rlens=None)
        assert rc == HUFE_ARGUMENT and msg.startswith(who + " rec_cap 16 needs d_rec_pos and d_rec_len")
    else:
        assert valid(*call(lib, name, expr=[[[b"a", O(b"\n")]]], anchors=3), who)      # (D is the boundary's, not the classes')


# ---- the models against re -----------------------------------------------------------------------------------------------
LEFT = {0: b"", BOL: rb"(?:^|(?<=\n))", WORD: rb"(?<!\w)", BOL | WORD: rb"(?:^|(?<=\n))(?<!\w)"}
RIGHT = {0: b"", EOL: rb"(?:$|(?=\n))", WORD: rb"(?!\w)", EOL | WORD: rb"(?:$|(?=\n))(?!\w)"}
LETTERS = np.array([97, 98, 99, 32, 10])                    # three word bytes, one that is none, the delimiter


def alternation(alts):
    return b"(?:" + b"|".join(b"(?:" + text(a) + b")" for a in alts) + b")"


def anchored(body, anchors, first=True, last=True):
    return (LEFT[anchors & (BOL | WORD)] if first else b"") + body + (RIGHT[anchors & (EOL | WORD)] if last else b"")


def re_expr_positions(data, alts, anchors, blocksize, cap=0, served=None):
    """the starts from ONE look-ahead of `re`, which tries every form; the served rule on the shortest qualifying form, the
    shortest slice that some alternative matches in full and whose right neighbour - a plain look at the byte - qualifies"""
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    look = re.compile(b"(?=" + anchored(alternation(alts), anchors) + b")")
    each = [re.compile(text(a), re.DOTALL) for a in alts]

    def right_ok(q):
        return q == n or ((not anchors & EOL or raw[q] == 10) and (not anchors & WORD or raw[q] not in W))

    pos, counts, found = [], [0] * nb, 0
    for hit in look.finditer(raw):
        p = hit.start()
        found += 1
        shortest = next(m for m in range(1, 65) if right_ok(p + m) and any(r.fullmatch(raw, p, p + m) for r in each))
        lo = p - 1 if p > 0 and anchors & (BOL | WORD) else p
        hi = p + shortest if p + shortest < n and anchors & (EOL | WORD) else p + shortest - 1
        if all(served[b] for b in range(lo // bs, hi // bs + 1)):
            pos.append(p)
            counts[p // bs] += 1
    written = min(len(pos), cap)
    return (pos[:written], counts, [len(pos), written, nb - sum(served), 0]), found


def re_expr_records(data, terms, anchors, mode, blocksize, cap=0, max_len=0, served=None):
    """bytes.split and, a line, re.search of 'A[^\\n]*B' with the anchors at the outer edges - or of every term in turn"""
    raw, n = bytes(data), len(data)
    bs = blocksize or n
    nb = (n + bs - 1) // bs if n else 0
    served = [True] * nb if served is None else list(served)
    clip = max_len or 2**32 - 1
    if mode == ORDERED:
        last = len(terms) - 1
        want = [re.compile(rb"[^\n]*".join(anchored(alternation(t), anchors, k == 0, k == last) for k, t in enumerate(terms)))]
    else:
        want = [re.compile(anchored(alternation(t), anchors)) for t in terms]
    pos, lens, counts, cut = [], [], [0] * nb, []
    s = 0
    for piece in raw.split(b"\n") if n else []:
        e = s + len(piece)
        if all(w.search(piece) for w in want) and all(served[b] for b in range(max(s - 1, 0) // bs, min(e, n - 1) // bs + 1)):
            pos.append(s)
            lens.append(min(e - s, clip))
            cut.append(e - s > clip)
            counts[s // bs] += 1
        s = e + 1
    written = min(len(pos), cap)
    return pos[:written], lens[:written], counts, [len(pos), written, nb - sum(served), sum(cut[:written])]


def same_positions(data, alts, anchors, blocksize, cap=0, served=None):
    got = find_any_expr_model(data, alts, b"\n", W, anchors, blocksize, cap, served)
    want, found = re_expr_positions(data, alts, anchors, blocksize, cap, served)
    assert tuple(g.tolist() for g in got) == want, (alts, anchors, bytes(data), blocksize, served)
    return found


def same_records(data, terms, anchors, mode, blocksize, cap=0, max_len=0, served=None):
    got = find_records_expr_model(data, terms, b"\n", W, anchors, mode, blocksize, cap, max_len, served)[:4]
    want = re_expr_records(data, terms, anchors, mode, blocksize, cap, max_len, served)
    assert tuple(g.tolist() for g in got) == want, (terms, anchors, mode, bytes(data), blocksize, served)
    return want[3][0]


def test_models_by_hand():
    d = lambda s: np.frombuffer(s, np.uint8)                        # noqa: E731
    ab_ = [lit(b"ab", (1,))]                                        # 'ab?'
    # 'ab?$' on "ab\n": "a" lies at 0 and does not qualify, "ab" does; the reverse: 'ab?' with -w on "a b": the long form does not lie there
    assert find_any_expr_model(d(b"ab\nabb\na"), ab_, b"\n", W, EOL, 0, 9)[0].tolist() == [0, 7]
    assert find_any_expr_model(d(b"ab abb a"), ab_, b"\n", W, WORD, 0, 9)[0].tolist() == [0, 7]
    assert find_any_expr_model(d(b"ab\nxab\nab"), ab_, b"\n", W, BOL, 0, 9)[0].tolist() == [0, 7]
    assert find_any_expr_model(d(b"ab\nabx\na"), ab_, b"\n", W, BOL | EOL, 0, 9)[0].tolist() == [0, 7]
    # the served rule: blocks of 3, block 1 is not served.  "xab\n": 'ab?$' at 1 needs the byte at 3; 'ab?' alone does not
    served = [True, False, True]
    assert find_any_expr_model(d(b"xab\nxxxx"), ab_, b"\n", W, EOL, 3, 9, served)[0].tolist() == []
    assert find_any_expr_model(d(b"xab\nxxxx"), ab_, b"\n", W, 0, 3, 9, served)[0].tolist() == [1]
    assert find_any_expr_model(d(b"xa\nbxxxx"), ab_, b"\n", W, EOL, 3, 9, served)[0].tolist() == [1]           # "a" and its '\n' lie in block 0
    assert find_any_expr_model(d(b"xx\nabxab"), ab_, b"\n", W, BOL, 3, 9, [False, True, True])[0].tolist() == []    # the byte in front is not served
    for anchors in ANCHORS:                                         # a form that ends where the data ends, with and without a delimiter
        assert same_positions(d(b"xx\nab"), ab_, anchors, 2, 9) and same_positions(d(b"xx\nab\n"), ab_, anchors, 2, 9)
        assert same_positions(d(b"a"), ab_, anchors, 0, 9) == 1 and same_positions(d(b"ab"), ab_, anchors, 1, 9) >= 1
    took = [[lit(b"ERROR")], [lit(b"took ") + rep(b"0123456789", 1, 5) + lit(b"ms")]]
    log = d(b"ERROR took 5ms\nERROR took 123456ms\ntook 7ms ERROR\nERROR x took 12ms\n\nxERROR took 1ms")
    assert same_records(log, took, 0, ORDERED, 8, 9) == 3 and same_records(log, took, 0, ALL, 8, 9) == 4
    assert find_records_expr_model(log, took, b"\n", W, BOL | EOL, ORDERED, 8, 9)[0].tolist() == [0, 50]
    assert find_records_expr_model(log, took, b"\n", W, WORD, ORDERED, 8, 9)[0].tolist() == [0, 50]
    assert find_records_expr_model(log, took, b"\n", W, EOL, ORDERED, 8, 9)[0].tolist() == [0, 50, 69]


def random_alternative(rng, m, quantified):
    """classes of one or two of the three letters and the space; runs of optional positions of ONE class"""
    alt, k = [], 0
    flags = [quantified and bool(rng.integers(0, 3) == 0) for _ in range(m)]
    if all(flags):
        flags[int(rng.integers(0, m))] = False
    while k < m:
        cls = bytes(sorted(set(int(v) for v in rng.choice(LETTERS[:4], int(rng.integers(1, 3)), p=[0.3, 0.3, 0.3, 0.1]))))
        if not flags[k]:
            alt.append(cls)
            k += 1
            continue
        while k < m and flags[k]:
            alt.append(O(cls))
            k += 1
    return alt


def random_lines(rng, trial):
    n, bs = int(rng.integers(1 if trial % 2 else 40, 400)), int(rng.integers(0, 60))
    data = rng.choice(LETTERS, n, p=[0.25, 0.25, 0.2, 0.15, 0.15]).astype(np.uint8)
    if trial % 3 == 0:
        data[0] = 10
    data[n - 1] = 10 if trial % 2 else 97                   # the data ends with and without a delimiter
    return data, n, bs


def test_the_positions_model_against_re():
    """seed 41, 30 trials an anchor combination: `re` alone finds more than 1 000 qualifying starts, some for every combination"""
    rng = np.random.default_rng(41)
    total = 0
    for anchors in ANCHORS:
        found = 0
        for trial in range(30):
            alts = [random_alternative(rng, int(rng.integers(1, 6)), True) for _ in range(int(rng.integers(1, 4)))]
            data, n, bs = random_lines(rng, trial)
            nb = (n + (bs or n) - 1) // (bs or n)
            for served in (None, rng.integers(0, 5, nb) != 0):
                found += same_positions(data, alts, anchors, bs, int(rng.integers(0, 50)), served)
        assert found > 0, anchors
        total += found
    assert total >= 1000, total


def test_the_records_model_against_re():
    """one term, ALL and ORDERED with a quantified last term, every anchor combination where the call has it"""
    rng = np.random.default_rng(43)
    total = 0
    for anchors, mode, nt in itertools.product(ANCHORS, (ORDERED, ALL), (1, 2, 3)):
        if mode == ALL and nt > 1 and anchors:
            continue
        found = 0
        for trial in range(8):
            terms = []
            for t in range(nt):
                inner = mode == ORDERED and t + 1 < nt
                m = int(rng.integers(1, 4))
                terms.append([random_alternative(rng, m if inner else int(rng.integers(1, 5)), not inner) for _ in range(int(rng.integers(1, 3)))])
            data, n, bs = random_lines(rng, trial)
            nb = (n + (bs or n) - 1) // (bs or n)
            for served in (None, rng.integers(0, 5, nb) != 0):
                found += same_records(data, terms, anchors, mode, bs, int(rng.integers(0, 30)), int(rng.integers(0, 9)), served)
        assert found > 0, (anchors, mode, nt)
        total += found
    assert total >= 1000, total


# ---- the identities, at model level ----------------------------------------------------------------------------------------
def plain(alt):
    return [c[0] if isinstance(c, tuple) else c for c in alt]


def test_with_the_other_dimensions_off_the_models_are_the_older_models():
    rng = np.random.default_rng(47)
    same = lambda got, want: all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)     # noqa: E731
    for trial in range(40):
        data, n, bs = random_lines(rng, trial)
        nb = (n + (bs or n) - 1) // (bs or n)
        served = rng.integers(0, 5, nb) != 0
        cap, kw = int(rng.integers(0, 40)), dict(invert=trial % 2 == 1, before=int(rng.integers(0, 3)), after=int(rng.integers(0, 3)))
        quant = [random_alternative(rng, int(rng.integers(1, 6)), True) for _ in range(int(rng.integers(1, 4)))]
        fixed = [plain(a) for a in quant]
        anchors = int(rng.integers(0, 8))
        # no optional position, one term: the anchored models
        assert same(find_any_expr_model(data, fixed, b"\n", W, anchors, bs, cap, served),
                    find_any_anchored_model(data, fixed, b"\n", W, anchors, bs, cap, served))
        assert same(find_records_expr_model(data, [fixed], b"\n", W, anchors, trial % 2, bs, cap, 5, served, **kw),
                    find_records_anchored_model(data, fixed, b"\n", W, anchors, bs, cap, 5, served, **kw))
        # no anchor, one term: the quant models
        assert same(find_any_expr_model(data, quant, b"\n", W, 0, bs, cap, served), find_quant_model(data, quant, bs, cap, served))
        assert same(find_records_expr_model(data, [quant], b"\n", W, 0, trial % 2, bs, cap, 5, served, **kw),
                    find_quant_records_model(data, quant, b"\n", bs, cap, 5, served, **kw))
        # no anchor, no optional position: the terms' model
        terms = [[plain(random_alternative(rng, m, False)) for _ in range(int(rng.integers(1, 3)))] for m in rng.integers(1, 4, int(rng.integers(2, 4)))]
        for mode in (ALL, ORDERED):
            assert same(find_records_expr_model(data, terms, b"\n", W, 0, mode, bs, cap, 5, served, **kw),
                        find_terms_model(data, terms, b"\n", bs, cap, 5, served, mode=mode, **kw))


# ---- Expr ------------------------------------------------------------------------------------------------------------------
def test_expr_arrays():
    colour = list(b"colo") + [Opt(b"u"), ord("r")]
    x = GpuCodec.expr_arrays(Expr(colour, word=True))
    assert x["anchors"] == WORD and x["ordered"] and x["term_alts"].tolist() == [1] and x["alt_lens"].tolist() == [6]
    assert x["optional"].tolist() == [0, 0, 0, 0, 1, 0] and x["word_set"] == GpuCodec.byte_set(W) and x["delim_set"] == GpuCodec.byte_set(b"\n")
    x = GpuCodec.expr_arrays(Expr(b"ERROR", AnyOf(list(b"took ") + [Rep(b"0123456789", 1, 5)], b"ms"), bol=True, eol=True))
    assert x["anchors"] == BOL | EOL and x["term_alts"].tolist() == [1, 2] and x["alt_lens"].tolist() == [5, 10, 2] and x["word_set"] is None
    assert x["optional"].tolist() == [0] * 5 + [0] * 6 + [1] * 4 + [0, 0] and x["classes"].shape == (17, 32)
    assert GpuCodec.expr_arrays(Expr(b"a", whole_line=True))["anchors"] == BOL | EOL
    assert GpuCodec.expr_arrays(Expr(b"a", b"b", ordered=False))["ordered"] is False
    assert GpuCodec.expr_arrays(Expr([1, Opt(b"\n")]), delimiters=None)["delim_set"] is None
    assert GpuCodec.expr_arrays(Expr(b"a", word=True, word_bytes=b"ab"))["word_set"] == GpuCodec.byte_set(b"ab")
    assert [m for m in GpuCodec.expr_arrays(Expr(b"a"), ignore_case=True)["classes"][0].nonzero()[0]] == [8, 12]
    assert "Expr(" in repr(Expr(b"a", bol=True)) and len(Expr(b"a", b"b")) == 2
    assert GpuCodec._FIND_CALLS["expr"] == ("hufgpu_find_any_expr", "hufgpu_find_records_expr")


def test_expr_errors():
    for bad, words in ((Expr(), "Expr has 1 to 4 terms, not 0"), (Expr(*[b"a"] * 5), "Expr has 1 to 4 terms, not 5"),
                       (Expr(b"a", word_bytes=b"a"), "give `word=True`"), (Expr(b"a", b"b", ordered=False, bol=True), "anchors do not go with `ordered=False`"),
                       (Expr(AnyOf(b"ab", [1, Opt(2)]), b"x"), "term 0, alternative 1, item 1 is Opt(2)"),
                       (Expr(b"x", [Rep(b"a", 1, 2)], b"y", eol=True), "term 1, alternative 0, item 0 is Rep("),
                       (Expr(AnyOf(b"ab", b"abc"), b"x"), "term 0 has alternatives of the lengths [2, 3]"),
                       (Expr(b"x", [1, Rep(b"a", 3, 2)]), "term 1: alternative 0, item 1: Rep from 3 to 2"),
                       (Expr(b"x", [Opt(1), Opt(2)]), "term 1: alternative 0: every position is optional"),
                       (Expr(b"x", AnyOf()), "term 1 has no alternative"), (Expr(b"x", b""), "term 1: alternative 0 has length 0"),
                       (Expr(b"a" * 40, b"b" * 25), "sum to 65, above 64"), (Expr(b"a" * 40, AnyOf(b"b" * 11, b"c" * 12), eol=True), "sum to 65, above 64"),
                       (Expr(b"a" * 32, b"b" * 32, word=True), "and one position behind each of the 1 whose byte behind is tested sum to 65"),
                       (Expr(b"ab", AnyOf(b"c", [1, Opt(b"x\n")])), "term 1: class 1 of alternative 1 holds a delimiter (value 10)")):
        with pytest.raises(ValueError, match=re.escape(words)):
            GpuCodec.expr_arrays(bad)
    GpuCodec.expr_arrays(Expr(b"a" * 40, AnyOf(b"b" * 11, b"c" * 11), eol=True))
    GpuCodec.expr_arrays(Expr(b"a" * 32, b"b" * 32, bol=True))
    GpuCodec.expr_arrays(Expr(AnyOf(b"ab", [1, Opt(2)]), b"x", ordered=False))
    GpuCodec.expr_arrays(Expr(b"x", AnyOf(b"ab", b"abc")))
    for bad in (Expr("text"), Expr(GpuCodec.Seq(b"a", b"b")), Expr(Expr(b"a")), b"a"):
        with pytest.raises(TypeError):
            GpuCodec.expr_arrays(bad)


# ---- egrep() ---------------------------------------------------------------------------------------------------------------
def items_of(expr):
    """an Expr as the models take it: a list of terms, a term a list of alternatives of items"""
    out = []
    for term in expr:
        alts = []
        for alt in term if isinstance(term, AnyOf) else [term]:
            items = []
            for c in alt:
                c = bytes([c]) if isinstance(c, int) else c
                items += rep(c.cls, c.lo, c.hi) if isinstance(c, Rep) else [O(c.cls)] if isinstance(c, Opt) else [c]
            alts.append(items)
        out.append(alts)
    return out


def anchors_of(expr):
    return (BOL if expr.bol else 0) | (EOL if expr.eol else 0) | (WORD if expr.word else 0)


def test_egrep_by_hand():
    eg = GpuCodec.egrep
    digits = b"0123456789"
    x = eg(rb"^[0-9]{1,3}\.[0-9]{1,3}")
    assert (x.bol, x.eol, x.word, x.ordered) == (True, False, False, True) and repr(x.terms) == repr(([Rep(digits, 1, 3), b".", Rep(digits, 1, 3)],))
    x = eg(rb"\<colou?r\>")
    assert anchors_of(x) == WORD and repr(x.terms) == repr(([b"c", b"o", b"l", b"o", Opt(b"u"), b"r"],))
    assert repr(eg(rb"\bcolou?r\b")) == repr(x)
    x = eg(rb"refused [0-9]{1,5} times$")
    assert anchors_of(x) == EOL and len(x) == 1 and len(x.terms[0]) == 8 + 1 + 6
    x = eg(rb"^2026-10-19.*ERROR")
    assert anchors_of(x) == BOL and [len(t) for t in x] == [10, 5]
    x = eg(rb"ERROR.*took [0-9]{1,5}ms")
    assert anchors_of(x) == 0 and [len(t) for t in x] == [5, 8] and isinstance(x.terms[1][5], Rep)
    x = eg(rb"^\<a.*b.*c.*d?e\>$")
    assert anchors_of(x) == 7 and [len(t) for t in x] == [1, 1, 1, 2]
    x = eg(rb"^foo$|^ba?r$")
    assert anchors_of(x) == 3 and len(x) == 1 and isinstance(x.terms[0], AnyOf) and len(x.terms[0]) == 2
    # a leading '.*' goes with the '^' in front of it, a trailing one with the '$' behind it
    assert anchors_of(eg(rb"^.*foo$")) == EOL and anchors_of(eg(rb"^foo.*$")) == BOL and anchors_of(eg(rb"^.*foo.*$")) == 0
    assert [len(t) for t in eg(rb".*a.*.*bc.*")] == [1, 2] and repr(eg(rb".*foo")) == repr(eg(rb"foo"))
    assert repr(eg(rb"ab?.*")) == repr(eg(rb"ab?"))                 # (a quantified term in front of a '.*' that goes)
    assert repr(GpuCodec.regex(rb"colou?r|x{1,2}")) == repr(eg(rb"colou?r|x{1,2}").terms[0])
    (alt,) = eg(rb"^.[^a]$", delimiters=b"\n;").terms
    assert all(10 not in c and 59 not in c for c in alt)
    assert eg(rb"^a", ignore_case=True).terms[0] == [b"Aa"]
    data = np.frombuffer(b"10.0.0.1 ok\nx 10.0.0.1\n1234.5\n7.7", np.uint8)
    x = eg(rb"^[0-9]{1,3}\.[0-9]{1,3}")
    assert find_records_expr_model(data, items_of(x), b"\n", W, anchors_of(x), ORDERED, 0, 9)[0].tolist() == [0, 30]


WORD_ATOMS = [b"a", b"b", b"c", b"d", b"[ab]", b"[a-c]", rb"\d", rb"\w", b"_", rb"\x61"]
ATOMS = WORD_ATOMS + [rb"\.", b".", b"[^a]", rb"\D", rb"\S", b" ", b"[^b-d.]"]
QUANTS = [b"", b"", b"", b"?", b"{2}", b"{1,3}", b"{,2}"]


def random_term(rng, atoms, quantified):
    parts = [atoms[int(rng.integers(0, len(atoms)))] + (QUANTS[int(rng.integers(0, len(QUANTS)))] if quantified else b"")
             for _ in range(int(rng.integers(1, 5)))]
    return b"".join(parts)


def test_egrep_on_random_expressions():
    """the expression's text compiled by `re` - MULTILINE, so that '^' and '$' are a line's - against the models on the Expr
    that egrep makes of it: the lines that match, and for one term the starts.  With '\\b' every atom is a word atom: grep
    -w's rule and '\\b' agree when a form begins and ends with a word byte."""
    rng = np.random.default_rng(53)
    letters = np.frombuffer(b"abcd01._ \n", np.uint8)
    hits = tried = 0
    while tried < 420:
        bol, eol, word = (bool(rng.integers(0, 3) == 0) for _ in range(3))
        atoms = WORD_ATOMS if word else ATOMS
        wrap = lambda body: (b"^" if bol else b"") + (rb"\b" if word else b"") + body + (rb"\b" if word else b"") + (b"$" if eol else b"")     # noqa: E731
        if tried % 3 == 0:
            nt = int(rng.integers(2, 5))
            expr = wrap(b".*".join(random_term(rng, atoms, t + 1 == nt) for t in range(nt)))
        else:
            expr = b"|".join(wrap(random_term(rng, atoms, True)) for _ in range(int(rng.integers(1, 4))))
        ignore_case = tried % 5 == 0
        try:
            x = GpuCodec.egrep(expr, ignore_case=ignore_case)
            GpuCodec.expr_arrays(x)
        except ValueError as e:
            assert "is optional: it would match everywhere" in str(e) or "above 64" in str(e), (expr, e)
            continue
        tried += 1
        assert anchors_of(x) == (BOL if bol else 0) | (EOL if eol else 0) | (WORD if word else 0), expr
        data = rng.choice(letters, int(rng.integers(1, 160))).astype(np.uint8)
        if ignore_case:
            data = np.where(rng.integers(0, 2, data.size) == 1, np.frombuffer(bytes(data).upper(), np.uint8), data)
        flags = re.MULTILINE | (re.IGNORECASE if ignore_case else 0)
        rx = re.compile(expr, flags)
        want, s = [], 0
        for piece in bytes(data).split(b"\n"):
            if rx.search(piece) and piece:
                want.append(s)
            s += len(piece) + 1
        got = find_records_expr_model(data, items_of(x), b"\n", W, anchors_of(x), ORDERED, 0, data.size)[0].tolist()
        assert got == want, (expr, bytes(data))
        hits += len(want)
        if len(x) == 1 and b"[^" not in expr and rb"\D" not in expr:     # (those hold '\n' for `re`, and never for egrep)
            want = [m.start() for m in re.finditer(b"(?=(?:" + expr + b"))", bytes(data), flags)]
            got = find_any_expr_model(data, items_of(x)[0], b"\n", W, anchors_of(x), 0, data.size)[0].tolist()
            assert got == want, (expr, bytes(data))
            hits += len(want)
    assert hits > 1000


@pytest.mark.parametrize("expr,at,words", [
    (rb"ab*", 2, "unbounded"), (rb"a+b", 1, "unbounded"), (rb"a.+b", 2, "unbounded"), (rb"abc{2,}", 3, "unbounded: not in this matcher"),
    (rb"a(b)", 1, "groups"), (rb"^(a|b)$", 1, "groups"), (rb"a\bb", 1, "inside a term"), (rb"a.*\bb", 3, "inside a term"), (rb"a\b.*b", 1, "inside a term"),
    (rb"a\<b", 1, "inside a term"), (rb"\>ab", 0, "inside a term"), (rb"ab\<", 2, "inside a term"), (rb"\<\<ab", 2, "inside a term"),
    (rb"ab?.*c", 3, "a quantified term in front of a '.*'"), (rb"a{1,2}.*b.*c", 6, "a quantified term in front of a '.*'"),
    (rb"a.*b|c", 1, "'.*' next to '|'"), (rb"c|a.*b", 3, "'.*' next to '|'"), (rb".*a|b", 0, "'.*' next to '|'"), (rb"a|b.*", 3, "'.*' next to '|'"),
    (rb"^a|b", 3, "do not carry the same anchors"), (rb"a$|b", 3, "do not carry the same anchors"), (rb"\ba\b|^\bb\b", 6, "do not carry the same anchors"),
    (rb"a^b", 1, "'^' stands at the start"), (rb"^^a", 1, "'^' stands at the start"), (rb"\<^a", 2, "'^' stands at the start"), (rb"a.*^b", 3, "'^' stands at the start"),
    (rb"a$b", 1, "'$' stands at the end"), (rb"$", 0, "'$' stands at the end"), (rb"a$$", 1, "'$' stands at the end"), (rb"a$.*b", 1, "'$' stands at the end"),
    (rb"\<ab", 0, "at one end of the alternative only"), (rb"a|b\b", 2, "at one end of the alternative only"),
    (rb"a.*b.*c.*d.*e", 10, "more than 4 terms"), (rb"\<.*a\>", 2, "behind a word's start"), (rb"\<a.*\>", 3, "in front of a word's end"),
    (rb"a.**b", 3, "nothing to repeat"), (rb"a.*?b", 3, "nothing to repeat"), (rb"^?a", 1, "nothing to repeat"), (rb"^", 0, "empty alternative"),
    (rb".*", 0, "empty alternative"), (rb"^.*$", 0, "empty alternative"), (rb"a.*b?", 0, "every position of a term is optional"),
    (rb"ab\q", 2, "escape"), (rb"a{65}", 0, "come to 65, above 64")])
def test_egrep_rejects(expr, at, words):
    with pytest.raises(ValueError, match=re.escape(f"egrep: offset {at}: ")) as e:
        GpuCodec.egrep(expr)
    assert words in str(e.value), e.value


def test_regex_keeps_its_rejections():
    for expr, at in ((rb"^ab", 0), (rb"ab$", 2), (rb"a.*b", 2), (rb"a.+", 2), (rb"\bab", 0), (rb"\<ab", 0)):
        with pytest.raises(ValueError, match=re.escape(f"regex: offset {at}: ")):
            GpuCodec.regex(expr)

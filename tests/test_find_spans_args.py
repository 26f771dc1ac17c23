"""hufgpu_find_any_spans: its declaration, every argument error - hufgpu_find_any_expr's under the new prefix, word for word,
and the new one in its place, each with no context at all -, the model of its result against Python's `re`, and the Python
layer: GpuCodec.find_spans, extract and redact(spans=True) (no GPU needed).

The model against `re`: for every start p the expected length is the largest L <= 64 for which some alternative `fullmatch`es
data[p:p + L] and the anchors hold for that L - BOL: p = 0 or a newline in front; EOL: p + L = n or a newline behind; WORD: no
word byte on either side -, and the starts are the p that have such an L.  The data is bytes over four letters, space and
newline (a, b, e, x: the letters of 'ab?', 'a?b', 'ab?c?d?e' and 'x{2,5}'); a second input adds c and d, so that the optional
middle of 'ab?c?d?e' is taken as well as left out.
"""
import re

import numpy as np
import pytest

from find_args_support import DEFAULTS, HUFE_ARGUMENT, LAYOUTS, SEL, alts_of, declaration, lib, valid  # noqa: F401
from find_calls import ANY_OF, HEAD, TAIL
from find_expr_support import COLOUR, O, arrays, call as expr_call, lit, rep
from find_spans_model import BOL, EOL, WORD, find_spans_model
from libhuffman_amd import _native
from libhuffman_amd.codec import GpuCodec
from test_find_quant_args import text

AnyOf, Opt, Rep, Expr = GpuCodec.AnyOf, GpuCodec.Opt, GpuCodec.Rep, GpuCodec.Expr
W = GpuCodec.WORD_BYTES
NAME, OLDER = "find_any_spans", "find_any_expr"
SLOTS = HEAD + ANY_OF + ("opt", "delims", "words", "anchors", "pos", "rlens", "open", "cap") + TAIL


def call(lib, **kw):
    """the span call with a NULL context and made-up pointers, as tests/find_expr_support.py's `call` makes the expr call"""
    values = dict(DEFAULTS, anchors=0, open=SEL)
    cls, lens, n, opt, _, _ = arrays(kw.pop("expr", COLOUR))
    values.update(cls=cls, lens=lens, n=n, opt=opt)
    if "alts" in kw:
        values["cls"], values["lens"], values["n"] = kw.pop("alts")
    unknown = set(kw) - set(SLOTS)
    assert not unknown, sorted(unknown)
    values.update(kw)
    rc = lib.hufgpu_find_any_spans(*[values[slot] for slot in SLOTS])
    return rc, lib.hufgpu_last_error(None).decode()


# ---- the symbol ----------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_declared(lib):
    """the expr positions call with (d_len, d_open) directly behind d_pos.  The symbol stands in GPU_EXTRA_SYMBOLS: GPU_SYMBOLS
    is read by tests/test_gpu_streams.py as the closed list of the search calls that have a stream case there"""
    assert "hufgpu_" + NAME in _native.GPU_EXTRA_SYMBOLS and hasattr(lib, "hufgpu_" + NAME)
    older, mine = lib.hufgpu_find_any_expr.argtypes, lib.hufgpu_find_any_spans.argtypes
    assert len(mine) == len(SLOTS) == len(older) + 2
    assert list(mine[:16]) + list(mine[18:]) == list(older) and mine[16] is mine[17] is mine[15]
    squeeze = lambda s: re.sub(r"\s+", " ", s)                      # noqa: E731
    header, m = declaration(NAME)
    _, s = declaration(OLDER)
    assert m and squeeze(m.group(1)) == squeeze(s.group(1)).replace("uint64_t *d_pos,", "uint64_t *d_pos, uint32_t *d_len, uint8_t *d_open,")
    about = header[header.index("FIND, MATCH SPANS"):header.index("int hufgpu_find_any_spans")]
    for words in ("leftmost-longest", "spans for the records calls", "quantified middle term", "unbounded repeats", "groups"):
        assert words in about[about.index("OUT OF SCOPE"):], words


# ---- the argument errors -------------------------------------------------------------------------------------------------
def test_valid_arguments_still_need_a_context(lib):
    for kw in ({}, {"opt": None}, {"anchors": 7}, {"anchors": 4, "delims": None}, {"open": None}, {"cap": 0, "pos": None, "rlens": None, "open": None},
               {"expr": [[lit(b"abc")]]}, {"expr": [[lit(b"ab"), lit(b"abc")]]}):
        assert valid(*call(lib, **kw), NAME + ":"), kw
    for nblocks, raw_size in LAYOUTS:
        assert valid(*call(lib, nblocks=nblocks, raw_size=raw_size), NAME + ":")


OVER = arrays([[rep(b"x", 1, 32), rep(b"y", 2, 32)]])
EXPR_ERRORS = [({"anchors": 8}, "anchors 0x8 has a bit"), ({"anchors": 4, "words": None}, "needs the word_set"),
               ({"anchors": 2, "delims": None}, "need the delim_set"), ({"cls": None}, "the classes, alt_lens and d_totals are required"),
               ({"lens": None}, "are required"), ({"n": 0}, "n_alts 0 is not 1 to 64"), ({"n": 65}, "n_alts 65"),
               ({"alts": alts_of([b"a"], [], [b"b"]), "opt": None}, "alternative 1 has length 0"),
               ({"alts": (arrays(COLOUR)[0] * 8, np.array([32, 33], np.uint32).tobytes(), 2), "opt": None}, "sum to 65, above 64"),
               ({"anchors": 2, "alts": OVER[:3], "opt": None}, "one boundary position each sum to 66"),
               ({"alts": alts_of([b"a", b""], [b"b"]), "opt": None}, "class 1 of alternative 0 is empty"),
               ({"opt": bytes([2]) + bytes(8)}, "optional is 2 at position 0 of alternative 0"),
               ({"expr": [[lit(b"ab"), [O(b"a"), O(b"b")]]]}, "every position of alternative 1 is optional"),
               ({"totals": None}, "d_totals are required"), ({"pos": None}, "pos_cap 16 needs d_pos"),
               ({"nblocks": 0}, "wrote these 0 blocks"), ({"stream": None}, "the stream, its block index and d_block_errs are required"),
               ({"index": None}, "are required"), ({"errs": None}, "are required"), ({"sub": None}, "8-byte aligned"), ({"sub": 0x30004}, "8-byte aligned"),
               ({"raw_size": 0}, "must be those of the encode"), ({"nblocks": 5}, "must be those of the encode"),
               ({"blocksize": 1 << 40, "raw_size": 1 << 42}, "must be those of the encode")]


@pytest.mark.parametrize("kw,words", EXPR_ERRORS, ids=[w[:24] for _, w in EXPR_ERRORS])
def test_the_expr_calls_errors_under_the_new_prefix(lib, kw, words):
    """every one of them, word for word: the same arguments give the expr call's message with the other name in front"""
    rc, msg = call(lib, **kw)
    want_rc, want = expr_call(lib, OLDER, **kw)
    assert rc == want_rc == HUFE_ARGUMENT and words in msg, msg
    assert msg == want.replace(OLDER + ":", NAME + ":", 1) and msg.startswith(NAME + ":"), (msg, want)


def test_a_cap_needs_d_len(lib):
    rc, msg = call(lib, rlens=None)
    assert rc == HUFE_ARGUMENT and msg == "find_any_spans: pos_cap 16 needs d_len", msg
    assert valid(*call(lib, rlens=None, cap=0), NAME + ":")
    # its place: with the required pointers - behind the patterns' checks and d_pos, in front of the geometry and the context
    for kw, words in (({"opt": bytes([2]) + bytes(8)}, "optional is 2"), ({"totals": None}, "d_totals are required"), ({"pos": None}, "needs d_pos")):
        rc, msg = call(lib, rlens=None, **kw)
        assert rc == HUFE_ARGUMENT and words in msg, msg
    for kw in ({"stream": None}, {"sub": None}, {"nblocks": 5}, {"raw_size": 0}):
        rc, msg = call(lib, rlens=None, **kw)
        assert rc == HUFE_ARGUMENT and msg.endswith("needs d_len"), msg


# ---- the model against `re` ----------------------------------------------------------------------------------------------
LETTERS = b"abex"


def words_input(letters, seed, final_newline):
    """lines of words over `letters`: one word a line for every length that a pattern below can end at, lines of several
    short words, words of one repeated letter - the runs that 'x{2,5}' and the class patterns of 33 and 64 positions need -, and
    "x ab" as the last line: with `final_newline` a delimiter ends the data, without it a form does"""
    rng = np.random.default_rng(seed)
    word = lambda k: bytes(rng.choice(np.frombuffer(letters, np.uint8), k))     # noqa: E731
    lines = [word(k) for k in (1, 2, 3, 4, 5, 6, 17, 31, 32, 33, 34, 62, 63, 64, 65, 70)]
    lines += [b"ab", b"a", b"b", b"abe", b"ae", b"abcde", b"acde", b"abde", b"ade", b"x", b"xx", b"xxx", b"xxxxx", b"xxxxxxx"]
    lines += [b" ".join(word(int(k)) for k in rng.integers(1, 7, 4)) for _ in range(6)]
    lines += [b"ab abe a", b"xx xxxx x", b"b ab", b" ae ", word(40) + b" " + word(33)]
    order = rng.permutation(len(lines))
    data = b"\n".join([lines[i] for i in order] + [b"x ab"]) + (b"\n" if final_newline else b"")
    return np.frombuffer(data, np.uint8)


def quantified(m, how):
    """one alternative of m positions of the class LETTERS: `how` says which of them are optional"""
    opt = {"none": (), "one": (m // 2,) if m > 1 else (), "alternating": tuple(range(1, m, 2)), "all-but-one": tuple(range(1, m))}[how]
    return [O(LETTERS) if k in opt else LETTERS for k in range(m)]


PATTERNS = {"%d-%s" % (m, how): [quantified(m, how)] for m in (1, 2, 5, 33, 64) for how in ("none", "one", "alternating", "all-but-one")}
PATTERNS.update({"ab?": [lit(b"ab", (1,))], "a?b": [lit(b"ab", (0,))], "ab?c?d?e": [lit(b"abcde", (1, 2, 3))], "x{2,5}": [rep(b"x", 2, 5)],
                 "unequal": [lit(b"ab"), lit(b"abe"), lit(b"x"), lit(b"xxxx")], "mixed": [lit(b"ab", (1,)), rep(b"x", 1, 3) + lit(b"a")]})


def several_lengths(alts):
    return len({len(a) for a in alts}) > 1 or any(isinstance(c, tuple) for a in alts for c in a)


def one_class(alt):
    """an alternative whose positions all have ONE class as 'c{required,all}': its forms are exactly the runs of those lengths,
    and `re` does not try every subset of 32 optional positions; None for any other alternative"""
    from find_args_support import bracket
    classes = {c[0] if isinstance(c, tuple) else c for c in alt}
    if len(classes) != 1:
        return None
    required = sum(not isinstance(c, tuple) for c in alt)
    return bracket(classes.pop()) + b"{%d,%d}" % (required, len(alt))


def re_spans(data, alts, anchors):
    """{start: the longest qualifying length} by fullmatch, length by length"""
    raw, n = bytes(data), len(data)
    each = [re.compile(one_class(a) or text(a), re.DOTALL) for a in alts]
    longest = max(len(a) for a in alts)
    word = set(W)
    out = {}
    for p in range(n):
        if anchors & BOL and p > 0 and raw[p - 1] != 10:
            continue
        if anchors & WORD and p > 0 and raw[p - 1] in word:
            continue
        for L in range(min(longest, 64, n - p), 0, -1):
            if anchors & EOL and p + L < n and raw[p + L] != 10:
                continue
            if anchors & WORD and p + L < n and raw[p + L] in word:
                continue
            if any(e.fullmatch(raw, p, p + L) for e in each):
                out[p] = L
                break
    return out


INPUTS = {"abex": words_input(LETTERS, 1, False), "abex-nl": words_input(LETTERS, 2, True), "abcdex": words_input(b"abcdex", 3, False)}


@pytest.mark.parametrize("anchors", range(8))
@pytest.mark.parametrize("name", PATTERNS)
def test_the_model_against_re(name, anchors):
    alts = PATTERNS[name]
    if name.startswith("64-") and anchors & (EOL | WORD):
        alts = [alts[0][:63]]                                       # (the byte behind takes the 64th bit of the matcher's state: the budget)
    for which, data in INPUTS.items():
        if which == "abex-nl" and name[0].isdigit() and name[:2] not in ("1-", "5-"):
            continue                                                # (the long class patterns: one input ends with the data, that is enough)
        if which == "abcdex" and name != "ab?c?d?e":
            continue                                                # (the third input is that pattern's)
        want = re_spans(data, alts, anchors)
        pos, lengths, opened, _, totals = find_spans_model(data, alts, b"\n", W, anchors, 0, data.size)
        assert dict(zip(pos.tolist(), lengths.tolist())) == want, (name, anchors, which)
        assert not opened.any() and totals.tolist() == [len(want), len(want), 0, 0]
        # re's own count: the combination is not an empty one, and where forms differ in length so do the answers
        assert len(set(want.values())) >= (2 if several_lengths(alts) else 1), (name, anchors, which, sorted(set(want.values())))
        if which != "abex-nl" and name in ("ab?", "a?b", "unequal") and not anchors & BOL:
            assert want[data.size - 2] == 2, "the form that ends with the data"


def test_the_model_by_hand():
    d = lambda s: np.frombuffer(s, np.uint8)                        # noqa: E731
    ab_ = [lit(b"ab", (1,))]
    m = lambda *a, **k: tuple(x.tolist() for x in find_spans_model(*a, **k)[:3])        # noqa: E731
    # 'ab?$': at 0 the short form fails its anchor and the long one qualifies; at 3 the reverse: "ab" does not lie there
    assert m(d(b"ab\na\n"), ab_, b"\n", W, EOL, 0, 9) == ([0, 3], [2, 1], [0, 0])
    assert m(d(b"ab a"), ab_, b"\n", W, WORD, 0, 9) == ([0, 3], [2, 1], [0, 0])         # ... and the form that ends with the data
    assert m(d(b"abb ab"), ab_, b"\n", W, 0, 0, 9) == ([0, 4], [2, 2], [0, 0])
    # blocks of 3, block 1 is not served: the short form is served, the long one reaches into block 1 - open
    served = [True, False, True]
    assert m(d(b"xxabxxxxx"), ab_, b"\n", W, 0, 3, 9, served) == ([2], [1], [1])
    assert m(d(b"xaxbxxxxx"), ab_, b"\n", W, 0, 3, 9, served) == ([1], [1], [0])        # ruled out by a served byte
    assert m(d(b"xa\nbxxab"), ab_, b"\n", W, EOL, 3, 9, served) == ([1, 6], [1, 2], [0, 0])    # '\n' is no 'b': nothing longer
    assert find_spans_model(d(b"xxabxxxxx"), ab_, b"\n", W, 0, 3, 9, served)[4].tolist() == [1, 1, 1, 1]
    # a complete form that waits for its right neighbour in a block that is not served: not reported at all (the expr rule)
    assert m(d(b"xxaxxxxab"), ab_, b"\n", W, EOL, 3, 9, served) == ([7], [2], [0])
    # the cap cuts all three, and totals[3] counts the written ones only
    assert m(d(b"a a a"), ab_, b"\n", W, 0, 0, 2) == ([0, 2], [1, 1], [0, 0])


# ---- the Python layer ----------------------------------------------------------------------------------------------------
@pytest.fixture()
def bare():
    """a GpuCodec without a context: what raises before the first device call needs none"""
    return GpuCodec.__new__(GpuCodec)


def key_of(pattern, **kw):
    args = dict(ignore_case=False, bol=False, eol=False, whole_line=False, word=False, word_bytes=None, delimiters=b"\n")
    args.update(kw)
    return GpuCodec._span_key(pattern, **args)


def test_fixed_length_patterns_give_the_constant():
    for pattern, length in ((b"ERROR", 5), ([b"ab", b"c"], 2), (AnyOf(b"GET", b"PUT"), 3), ([b"a", Rep(b"b", 2, 2)], 3), (GpuCodec.egrep(rb"^abc$"), 3)):
        assert key_of(pattern)[1] == length, pattern
    assert key_of(b"Error", ignore_case=True)[1] == 5 and key_of(b"ab", word=True)[1] == 2
    for pattern in (AnyOf(b"GET", b"POST"), GpuCodec.regex(rb"colou?r"), [Rep(b"0123456789", 1, 3)], GpuCodec.egrep(rb"\<colou?r\>")):
        assert key_of(pattern)[1] is None, pattern
    # every pattern becomes the one argument list: classes, alt_lens, n_alts, optional, delim_set, word_set, anchors
    key, _ = key_of(GpuCodec.regex(rb"colou?r"), word=True) if False else key_of(GpuCodec.regex(rb"colou?r"))
    assert len(key) == 7 and np.frombuffer(key[1], np.uint32).tolist() == [6] and key[2] == 1 and list(key[3]) == [0, 0, 0, 0, 1, 0] and key[6] == 0
    key, _ = key_of(b"ab", bol=True, word=True)
    assert key[3] is None and key[6] == _native.ANCHOR_BOL | _native.ANCHOR_WORD and key[5] == GpuCodec.byte_set(W)
    assert GpuCodec.SPAN_MAX == _native.FIND_PATTERN_MAX == 64


def spans(bare, pattern, **kw):
    return bare.find_spans(None, 0, None, 0, None, 100, 10, pattern, max_positions=4, **kw)


def pattern_call(bare, pattern, **kw):
    return bare.find_pattern(None, 0, None, 0, None, 100, 10, pattern, max_positions=4, **kw)


def test_find_spans_rejects_what_find_pattern_rejects(bare):
    G = GpuCodec
    cases = [(G.AllOf(b"a", b"b"), {}), (G.Seq(b"a", b"b"), {}), (G.egrep(rb"ab.*cd"), {}), ("text", {}), (b"", {}), (b"x" * 65, {}),
             (b"ab", {"word_bytes": b"ab"}), (G.regex(rb"colou?r"), {"word": True}), (G.egrep(rb"^ab"), {"bol": True}),
             (AnyOf(b"a" * 32, b"b" * 32), {"eol": True}), ([b"a", b""], {}), ([Opt(b"a")], {})]
    for pattern, kw in cases:
        with pytest.raises((TypeError, ValueError)) as want:
            pattern_call(bare, pattern, **kw)
        with pytest.raises(type(want.value)) as got:
            spans(bare, pattern, **kw)
        assert str(got.value) == str(want.value), (pattern, kw)
    with pytest.raises(TypeError, match="selects records"):
        spans(bare, G.AllOf(b"a", b"b"))


def redact(bare, pattern, **kw):
    return bare.redact(None, 0, None, 0, None, 100, 10, pattern, max_matches=4, **kw)


def test_redact_with_spans_validates_on_a_bare_codec(bare):
    G = GpuCodec
    with pytest.raises(ValueError, match="give one"):
        redact(bare, b"abc", spans=True, lines=True, max_len=8)
    with pytest.raises(TypeError, match="selects records"):
        redact(bare, G.Seq(b"a", b"b"), spans=True)
    with pytest.raises(ValueError, match="Opt / Rep"):
        redact(bare, G.regex(rb"colou?r"), spans=True, word=True)   # (an anchored Opt / Rep is an Expr's, as for find_pattern)
    with pytest.raises(TypeError, match="selects records"):
        bare.extract(None, 0, None, 0, None, 100, 10, G.AllOf(b"a", b"b"), 4)


def test_redact_without_the_keyword_still_refuses(bare):
    G = GpuCodec
    for pattern, word in (([b"a", G.Opt(b"b"), b"c"], "Opt / Rep"), ([G.Rep(b"0123456789", 1, 3)], "Opt / Rep"), (G.regex(rb"colou?r"), "Opt / Rep"),
                          (G.AnyOf(b"GET", b"POST"), "lengths [3, 4]"), (G.egrep(rb"^ab"), "Expr")):
        for kw in ({}, {"spans": False}):
            with pytest.raises(ValueError, match=re.escape(word)) as e:
                redact(bare, pattern, **kw)
            assert "lines=True" in str(e.value) and "where a match ends is not reported" in str(e.value)

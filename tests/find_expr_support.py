"""Helpers of the tests of hufgpu_find_any_expr and hufgpu_find_records_expr (tests/test_find_expr_args.py,
tests/test_gpu_find_expr.py): the two calls' slot lists next to the eleven of tests/find_calls.py, ONE caller with made-up
pointers for the argument tests and ONE with guarded device buffers for the GPU tests, both built on the older helpers.  Not a
test module.

A test names a pattern as tests/find_expr_model.py takes it: a list of terms, a term a list of alternatives, an alternative a
list of items, an item a class (required) or (class, True) (may be left out); the positions call takes one term's
alternatives.  `arrays` makes the C arrays of it."""
import numpy as np

from find_args_support import DEFAULTS
from find_calls import ANY_OF, HEAD, POSITIONS, TAIL
from find_model import byte_set
from find_quant_support import O, arrays as quant_arrays, lit, rep  # noqa: F401

BOL, EOL, WORD = 1, 2, 4
ALL, ORDERED = 0, 1
POS_NAME, REC_NAME = "find_any_expr", "find_records_expr"
NAMES = (POS_NAME, REC_NAME)
# hufgpu_find_any_anchored's slots with `optional` behind n_alts; hufgpu_find_records_context's with `optional`, the terms
# call's three and the anchored call's two
SLOTS = {POS_NAME: HEAD + ANY_OF + ("opt", "delims", "words", "anchors") + POSITIONS + TAIL,
         REC_NAME: HEAD + ("delims",) + ANY_OF + ("opt", "terms", "nt", "mode", "words", "anchors", "select", "before", "after", "pos", "rlens",
                                                  "no", "sel", "cap", "max_len") + TAIL}


def counts_of(*counts):
    """the host array term_alts"""
    return np.array(counts, np.uint32).tobytes()


def arrays(terms):
    """(classes, alt_lens, n_alts, optional, term_alts, n_terms): the C arrays as bytes"""
    cls, lens, n, opt = quant_arrays([a for term in terms for a in term])
    return cls, lens, n, opt, counts_of(*[len(term) for term in terms]), len(terms)


def invoke(lib, name, values):
    return getattr(lib, "hufgpu_" + name)(*[values[slot] for slot in SLOTS[name]])


# ---- made-up pointers --------------------------------------------------------------------------------------------------------
COLOUR = [[lit(b"colour", optional=(4,)), [b"eE", b"rR", O(b"rR")]]]          # one term
TOOK = [[lit(b"ERROR")], [lit(b"took ") + rep(b"0123456789", 1, 5) + lit(b"ms"), lit(b"ms", optional=(1,))]]   # 'ERROR.*(took [0-9]{1,5}ms|ms?)'


def call(lib, name, **kw):
    """the call with a NULL context and tests/find_args_support.py's DEFAULTS in every slot that `kw` does not name: (status,
    the message).  `expr` = terms as above stand for the six slots of the pattern (default: COLOUR; the positions call takes
    the alternatives of all terms); `alts` = (classes, alt_lens, n_alts), `opt`, `terms` and `nt` set them apart; `ba` =
    (before, after).  The default anchors are 0 and the default mode is ORDERED."""
    values = dict(DEFAULTS, anchors=0, mode=ORDERED)
    cls, lens, n, opt, terms, nt = arrays(kw.pop("expr", COLOUR))
    values.update(cls=cls, lens=lens, n=n, opt=opt, terms=terms, nt=nt)
    if "alts" in kw:
        values["cls"], values["lens"], values["n"] = kw.pop("alts")
    if "ba" in kw:
        values["before"], values["after"] = kw.pop("ba")
    unknown = set(kw) - set(SLOTS[name])
    assert not unknown, (name, "has no", sorted(unknown))
    values.update(kw)
    rc = invoke(lib, name, values)
    return rc, lib.hufgpu_last_error(None).decode()


# ---- guarded device buffers --------------------------------------------------------------------------------------------------
def expr_call(torch, codec, enc, name, terms, cap, anchors=0, mode=ORDERED, delims=b"\n", words=None, max_len=0, invert=False, before=0,
              after=0, numbers=True, flags=True, counts=True, sub=None, optional="as the pattern says", fetch=True):
    """one call as tests/find_support.py's find_call makes the older ones: guarded buffers - LEAD guard words in front, `cap`
    slots, TAIL behind - for every output the call has, the 7-tuple of host arrays back.  `terms`: the positions call takes
    the alternatives of all of them.  `optional`: None or bytes in the place of the pattern's own flags"""
    from find_support import GUARD8, GUARD32, GUARD64, LEAD, W, TAIL as BEHIND

    rec = name == REC_NAME
    cls, lens, n, opt, term_alts, nt = arrays(terms)
    if optional != "as the pattern says":
        opt = optional
    sub = enc.sub if sub is None else sub
    words = W if words is None else words

    def guarded(guard, dtype, wanted):
        return torch.full((LEAD + cap + BEHIND,), guard, dtype=dtype, device="cuda") if wanted else None

    def ptr(buf):
        return None if buf is None else buf[LEAD:].data_ptr()

    pbuf, lbuf = guarded(GUARD64, torch.int64, cap), guarded(GUARD32, torch.int32, cap and rec)
    nbuf, sbuf = guarded(GUARD64, torch.int64, rec and numbers), guarded(GUARD8, torch.uint8, rec and flags)
    totals = torch.empty(4, dtype=torch.int64, device="cuda")
    errs = torch.empty(enc.nb, dtype=torch.int32, device="cuda")
    cnt = torch.empty(enc.nb, dtype=torch.int64, device="cuda") if counts else None
    values = dict(ctx=codec._ctx, stream=enc.stream.data_ptr(), stream_len=enc.length, index=enc.offsets.data_ptr(), nblocks=enc.nb,
                  sub=sub.data_ptr(), raw_size=enc.raw_size, blocksize=enc.row_bs, cls=cls, lens=lens, n=n, opt=opt, terms=term_alts, nt=nt,
                  mode=mode, delims=None if delims is None else byte_set(delims), words=byte_set(words), anchors=anchors,
                  select=1 if invert else 0, before=before, after=after, pos=ptr(pbuf), rlens=ptr(lbuf), no=ptr(nbuf), sel=ptr(sbuf),
                  cap=cap, max_len=max_len, counts=cnt.data_ptr() if counts else None, totals=totals.data_ptr(), errs=errs.data_ptr(),
                  flags=0, hip_stream=codec._stream())
    codec._check(invoke(codec.lib, name, values), "Failed to enqueue the search")

    bufs = (pbuf, lbuf, totals, errs, cnt, nbuf, sbuf)
    if not fetch:                       # the device tensors, without a wait: find_support's find_fetch brings them to the host
        return bufs
    return tuple(None if t is None else t.cpu().numpy() for t in bufs)

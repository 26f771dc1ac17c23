"""Helpers of the tests of hufgpu_find_any_quant and hufgpu_find_records_quant (tests/test_find_quant_args.py,
tests/test_gpu_find_quant.py): the two calls' slot lists next to the eleven of tests/find_calls.py, ONE caller with made-up
pointers for the argument tests and ONE with guarded device buffers for the GPU tests, both built on the older helpers.  Not a
test module.

A test names a pattern as tests/find_quant_model.py takes it: a list of alternatives, an alternative a list of items, an item a
class (required) or (class, True) (may be left out).  `arrays` makes the three C arrays of it, `forms` writes every form out."""
import itertools

import numpy as np

from find_args_support import DEFAULTS
from find_calls import ANY_OF, HEAD, POSITIONS, TAIL
from find_model import byte_set
from find_quant_model import split

POS_NAME, REC_NAME = "find_any_quant", "find_records_quant"
NAMES = (POS_NAME, REC_NAME)
# hufgpu_find_any's and hufgpu_find_records_context's slots with `optional` behind n_alts
SLOTS = {POS_NAME: HEAD + ANY_OF + ("opt",) + POSITIONS + TAIL,
         REC_NAME: HEAD + ("delims",) + ANY_OF + ("opt", "select", "before", "after", "pos", "rlens", "no", "sel", "cap", "max_len") + TAIL}
OLDER = {POS_NAME: "find_any", REC_NAME: "find_records_context"}


def O(cls):
    """an optional item"""
    return (cls, True)


def rep(cls, lo, hi):
    """x{lo,hi} as items"""
    return [cls] * lo + [O(cls)] * (hi - lo)


def lit(word, optional=()):
    """a literal as items, the letters at the indexes `optional` optional"""
    return [O(bytes([v])) if k in optional else bytes([v]) for k, v in enumerate(word)]


def arrays(alternatives):
    """(classes, alt_lens, n_alts, optional): the C arrays as bytes"""
    parts = [split(a) for a in alternatives]
    classes = b"".join(byte_set(np.flatnonzero(row).tolist()) for t, _ in parts for row in t)
    lens = np.array([t.shape[0] for t, _ in parts], np.uint32).tobytes()
    return classes, lens, len(parts), np.concatenate([o for _, o in parts]).astype(np.uint8).tobytes()


def forms(alternatives):
    """every form of every alternative, written out as an alternative without optional items (few optional positions only)"""
    out = []
    for alt in alternatives:
        opt = [k for k, c in enumerate(alt) if isinstance(c, tuple) and len(c) == 2 and c[1] is True]
        assert len(opt) <= 10
        for keep in itertools.product((False, True), repeat=len(opt)):
            gone = {k for k, kept in zip(opt, keep) if not kept}
            form = [c[0] if k in opt else c for k, c in enumerate(alt) if k not in gone]
            if form not in out:
                out.append(form)
    return out


def invoke(lib, name, values):
    return getattr(lib, "hufgpu_" + name)(*[values[slot] for slot in SLOTS[name]])


# ---- made-up pointers --------------------------------------------------------------------------------------------------------
COLOUR = [lit(b"colour", optional=(4,)), [b"eE", b"rR", O(b"rR")]]


def call(lib, name, **kw):
    """the call with a NULL context and tests/find_args_support.py's DEFAULTS in every slot that `kw` does not name: (status,
    the message).  `quant` = a pattern as above stands for the four slots of the table (default: COLOUR); `alts` = (classes,
    alt_lens, n_alts) and `opt` set them apart; `ba` = (before, after)"""
    values = dict(DEFAULTS)
    cls, lens, n, opt = arrays(kw.pop("quant", COLOUR))
    values.update(cls=cls, lens=lens, n=n, opt=opt)
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
def quant_call(torch, codec, enc, name, alternatives, cap, delims=b"\n", max_len=0, invert=False, before=0, after=0, numbers=True,
               flags=True, counts=True, sub=None, optional="as the pattern says", fetch=True):
    """one call as tests/find_support.py's find_call makes the older ones: guarded buffers - LEAD guard words in front, `cap`
    slots, TAIL behind - for every output the call has, the 7-tuple of host arrays back.  `optional`: None or bytes in the
    place of the pattern's own flags"""
    from find_support import GUARD8, GUARD32, GUARD64, LEAD, TAIL as BEHIND

    rec = name == REC_NAME
    cls, lens, n, opt = arrays(alternatives)
    if optional != "as the pattern says":
        opt = optional
    sub = enc.sub if sub is None else sub

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
                  sub=sub.data_ptr(), raw_size=enc.raw_size, blocksize=enc.row_bs, cls=cls, lens=lens, n=n, opt=opt,
                  delims=byte_set(delims), select=1 if invert else 0, before=before, after=after, pos=ptr(pbuf), rlens=ptr(lbuf),
                  no=ptr(nbuf), sel=ptr(sbuf), cap=cap, max_len=max_len, counts=cnt.data_ptr() if counts else None,
                  totals=totals.data_ptr(), errs=errs.data_ptr(), flags=0, hip_stream=codec._stream())
    codec._check(invoke(codec.lib, name, values), "Failed to enqueue the search")

    bufs = (pbuf, lbuf, totals, errs, cnt, nbuf, sbuf)
    if not fetch:                       # the device tensors, without a wait: find_support's find_fetch brings them to the host
        return bufs
    return tuple(None if t is None else t.cpu().numpy() for t in bufs)

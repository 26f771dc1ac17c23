"""Helpers of the tests of hufgpu_find_records_terms (tests/test_find_terms_args.py, tests/test_gpu_find_terms.py): the call's
slot list next to the eleven of tests/find_calls.py, ONE caller with made-up pointers for the argument tests and ONE with
guarded device buffers for the GPU tests, both built on the older helpers.  Not a test module.

A test names its terms as a list of terms, a term a list of alternatives, an alternative what tests/find_any_model.py takes (a
`bytes` literal or a list of classes): `flat` makes the any-of table's alternatives and the counts a term of them."""
import numpy as np

from find_args_support import DEFAULTS, alts_of
from find_calls import ANY_OF, HEAD, TAIL
from libhuffman_amd.codec import GpuCodec

ALL, ORDERED = 0, 1
NAME = "find_records_terms"
WHO = NAME + ":"
# the context call's slots with (term_alts, n_terms, terms_mode) behind n_alts
SLOTS = HEAD + ("delims",) + ANY_OF + ("terms", "nt", "mode", "select", "before", "after", "pos", "rlens", "no", "sel", "cap", "max_len") + TAIL


def counts_of(*counts):
    """the host array term_alts"""
    return np.array(counts, np.uint32).tobytes()


def flat(terms):
    """(the alternatives of all terms one behind the other, each as a list of classes; the counts a term)"""
    return [[bytes([v]) for v in a] if isinstance(a, (bytes, bytearray)) else list(a) for term in terms for a in term], [len(term) for term in terms]


def invoke(lib, values):
    return lib.hufgpu_find_records_terms(*[values[slot] for slot in SLOTS])


# ---- made-up pointers --------------------------------------------------------------------------------------------------------
ONE = alts_of([b"eE", b"rR", b"rR"])
TWO = alts_of([b"eE", b"rR", b"rR"], [b"f", b"a", b"t"], [b"pP", b"i", b"g"])      # term 0: "err"; term 1: "fat" or "pig"


def call(lib, **kw):
    """the call with a NULL context and tests/find_args_support.py's DEFAULTS in every slot that `kw` does not name: (status,
    the message).  `alts` = (classes, alt_lens, n_alts) and `ta` = the counts a term stand for their slots (default: TWO as
    the terms (1, 2)); `ba` = (before, after)"""
    values = dict(DEFAULTS, mode=ALL)
    alts = kw.pop("alts", TWO)
    ta = kw.pop("ta", (1, 2) if alts is TWO else (alts[2],))
    values.update(cls=alts[0], lens=alts[1], n=alts[2], terms=None if ta is None else counts_of(*ta), nt=0 if ta is None else len(ta))
    if "ba" in kw:
        values["before"], values["after"] = kw.pop("ba")
    unknown = set(kw) - set(SLOTS)
    assert not unknown, ("the call has no", sorted(unknown))
    values.update(kw)
    rc = invoke(lib, values)
    return rc, lib.hufgpu_last_error(None).decode()


# ---- guarded device buffers --------------------------------------------------------------------------------------------------
def terms_call(torch, codec, enc, terms, mode, cap, delims=b"\n", max_len=0, invert=False, before=0, after=0, numbers=True, flags=True,
               counts=True, sub=None, fetch=True):
    """one hufgpu_find_records_terms call as tests/find_support.py's find_call makes the older ones: guarded buffers - LEAD
    guard words in front, `cap` slots, TAIL behind - for every output, the 7-tuple of host arrays back"""
    from find_support import GUARD8, GUARD32, GUARD64, LEAD, TAIL as BEHIND

    alts, per_term = flat(terms)
    classes, lens = GpuCodec.alt_classes(GpuCodec.AnyOf(*alts))
    sub = enc.sub if sub is None else sub

    def guarded(guard, dtype, wanted):
        return torch.full((LEAD + cap + BEHIND,), guard, dtype=dtype, device="cuda") if wanted else None

    def ptr(buf):
        return None if buf is None else buf[LEAD:].data_ptr()

    pbuf, lbuf = guarded(GUARD64, torch.int64, cap), guarded(GUARD32, torch.int32, cap)
    nbuf, sbuf = guarded(GUARD64, torch.int64, numbers), guarded(GUARD8, torch.uint8, flags)
    totals = torch.empty(4, dtype=torch.int64, device="cuda")
    errs = torch.empty(enc.nb, dtype=torch.int32, device="cuda")
    cnt = torch.empty(enc.nb, dtype=torch.int64, device="cuda") if counts else None
    values = dict(ctx=codec._ctx, stream=enc.stream.data_ptr(), stream_len=enc.length, index=enc.offsets.data_ptr(), nblocks=enc.nb,
                  sub=sub.data_ptr(), raw_size=enc.raw_size, blocksize=enc.row_bs, cls=classes.tobytes(), lens=lens.tobytes(), n=len(lens),
                  terms=counts_of(*per_term), nt=len(per_term), mode=mode, delims=GpuCodec.byte_set(delims), select=1 if invert else 0,
                  before=before, after=after, pos=ptr(pbuf), rlens=ptr(lbuf), no=ptr(nbuf), sel=ptr(sbuf), cap=cap, max_len=max_len,
                  counts=cnt.data_ptr() if counts else None, totals=totals.data_ptr(), errs=errs.data_ptr(), flags=0,
                  hip_stream=codec._stream())
    codec._check(invoke(codec.lib, values), "Failed to enqueue the search")

    bufs = (pbuf, lbuf, totals, errs, cnt, nbuf, sbuf)
    if not fetch:                       # the device tensors, without a wait: find_support's find_fetch brings them to the host
        return bufs
    return tuple(None if t is None else t.cpu().numpy() for t in bufs)

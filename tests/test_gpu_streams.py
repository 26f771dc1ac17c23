"""Every device call on a stream that is not the default one, and the enqueue-only calls inside a captured graph.

torch's side streams are non-blocking (asserted below through hipStreamGetFlags): nothing orders them with the null stream.
A launch that lost its stream argument, a helper that copies on the context's own stream, a blocking memset, a wait on a stale
stream - all of them are ordered for free when the caller's stream is the null stream, which is all the other test files use.

Part 1, the gate (tests/stream_gate.py).  On a side stream: a bounded spin, an event, device-to-device copies that put the real
input where a decoy stood, the call.  The decoy is a complete, valid input of the same geometry (for what decodes, the
oracle's encoding of other data whose stream is checked not to be longer; for the encoders the real bytes shuffled inside each
block), the warm-up is the same call on the decoy on the null stream, and every output starts as guard values: a misrouted
launch reads valid data and leaves an answer that the comparison rejects.  Every expected value comes from the CPU: the
oracle's stream and index, tests/sub_index_ref.py, slices of the input, the find models.  No input of a call was made by the
library under test.
  - The ENQUEUE-ONLY calls - encode and decode with sync=False, with and without the sub-index, histogram, gather, the three
    find methods and all sixteen hufgpu_find_* calls (the eleven of tests/find_calls.py and the five younger ones through
    their own helpers) - must return while the gate is closed.  A case whose gate had
    opened by then has proved nothing and FAILS; there is no skip and no second try.  The gate is the larger of 20 ms and 20
    times the host time of the warm-up call.  In front of the gate the call also runs once on the side stream itself, on the
    decoy (a stream's first launch of a kernel with scratch memory can take longer than the gate), and between the gate and
    the look at it Python's garbage collector rests.
  - The calls that WAIT inside - the sync forms of encode and decode, encode_batch, decode_batch, decode_ranges direct and by
    tiles, update_ranges, append, truncate, build_sub_index, decode_build_sub, decode_stream on a raw stream - run in the same
    set-up, but the result alone is the evidence, and it pins down only the launches in front of the call's first wait: from
    that wait on the gate is open and every stream has the real input.
  - One context across streams (a host wait between them), a fresh context whose first calls are on the side stream, a
    gather that grows its workspace with another pending in front of it, and two contexts on two streams interleaved.
Two streams on ONE context at the same time stay unsupported (include/huffman_gpu.h) and are not tested.

Part 2, capture.  While a stream captures in global mode the runtime refuses every wait and every blocking call, so an
enqueue-only call that captures has not waited.  It does NOT refuse a launch on the null stream next to a capturing stream
that is non-blocking, as torch's are: such a launch runs at once, on the decoy, and is missing from the graph.  The graph is
therefore replayed on two real inputs with two different answers, the static buffers overwritten before each replay: every
output starts as guard values inside the graph, so what was done eagerly at capture time is not there, and what the graph
carries must be the whole call.  One stream, so no parallel branches; nothing is set about queues or replay.

What this was seen to catch, once, with libraries built from a changed copy (the file then held the eleven older find calls
only): with pick_stream() returning NULL every gate case of
both kinds, the context-state, the growing-gather and the two-context cases failed on their comparisons and every capture
case failed at its first replay (the fresh-context cases passed: a first call's growth waits for the whole device, the gate
included, before anything is launched); with decode_sub_kernel alone launched on stream 0 the decode_sub gate and capture
cases failed, every output byte still the guard.  A known limit: the decoy keeps a misrouted launch to valid inputs, not to
a valid workspace - gather_place_kernel on stream 0 found the warm-up's cursors at their ends and faulted the device.
"""
import numpy as np
import pytest

import find_support as F
import sub_index_ref as R
from find_any_model import find_any_model, find_any_records_model
from find_anchor_model import find_any_anchored_model, find_records_anchored_model
from find_calls import CALLS
from find_classes_model import find_class_records_model, find_classes_model
from find_context_model import find_context_model
from find_model import find_model
from find_pattern_model import find_pattern_model
from find_records_model import find_records_model
from find_select_model import find_select_model
from find_expr_model import find_any_expr_model, find_records_expr_model
from find_expr_support import expr_call
from find_quant_model import find_quant_model, find_quant_records_model
from find_quant_support import lit, quant_call
from find_support import NL, TILE, W, find_enqueue, find_fetch
from find_terms_model import find_terms_model
from find_terms_support import terms_call
from libhuffman_amd import datagen
from stream_support import ranges_route_model
from stream_gate import GATE_FACTOR, GUARD, GUARD64, HIP_STREAM_NON_BLOCKING, MIN_GATE_MS, Gate, Input, Slots, rolled, shuffled, stream_flags

pytestmark = pytest.mark.gpu

OK = 0
G = 64                                  # guard bytes around a decoded output
BOL = 1
TERMS_ALL, TERMS_ORDERED = 0, 1
# name -> (blocksize, bytes): two tile seams a block with a short last tile, block seams and two scan lanes; more than one
# scan group of 256 blocks; blocks of 64 KiB, which alone reach decode_regs and tree_wave_kernel
SHAPES = {"5x4099": F.FOUR_SHAPES["5x4099"][:2], "300x64": F.FOUR_SHAPES["300x64"][:2], "3x65536": (65536, 2 * 65536 + 30001)}
SMALL = ("5x4099", "300x64")
P = F.pattern_below_255(6, 11)          # what the find cases look for: two literals that the data holds where they are planted
Q = F.pattern_below_255(4, 12)
CLASSES = [bytes([P[0], P[0] ^ 1])] + F.literal(P[1:])
ALTS = [P, Q]
DELIMS = bytes([NL])


# ---- the module's fixtures -----------------------------------------------------------------------------------------------------
class Env:
    def __init__(self, torch, codec, oracle):
        self.torch, self.codec, self.oracle = torch, codec, oracle
        self.gate = Gate(torch)
        self.s = torch.cuda.Stream()
        self.inputs = {}

    def ins(self, shape):
        """A and B: two real inputs of one stream length (B is A with every block rotated: the same histograms and index);
        C: other data, the second real input of what reads no stream; D: the decoy of what decodes, other and flatter data;
        S: the encoders' decoy, A shuffled inside each block"""
        if shape not in self.inputs:
            bs, n = SHAPES[shape]
            a = make_data(shape, 1)
            self.inputs[shape] = {"A": Input(self.oracle, a, bs), "B": Input(self.oracle, rolled(a, bs, bs // 4 + 1), bs),
                                  "C": Input(self.oracle, make_data(shape, 4), bs),
                                  "D": Input(self.oracle, make_data(shape, 2, flat=True), bs),
                                  "S": Input(self.oracle, shuffled(a, bs, 3), bs)}
            i = self.inputs[shape]
            assert not np.array_equal(i["A"].data, i["B"].data) and not np.array_equal(i["A"].stream, i["B"].stream)
            assert self.codec.sub_index_bytes(n, bs) == i["A"].exp.lay.size, shape
        return self.inputs[shape]


def make_data(shape, seed, flat=False):
    """zipf-like bytes with delimiters - at random, and in front of the shape's seams - and the two literals planted, P right
    behind a delimiter too; `flat`: half of the bytes are one value first, so that the encoding is shorter"""
    bs, n = SHAPES[shape]
    rng = np.random.default_rng(100 + seed)
    data = F.base_without(n, 40 + seed)
    if flat:
        data[rng.random(n) < 0.5] = 41
    at = np.unique(np.concatenate([rng.integers(0, n, n // 40), np.array(F.SEAMS.get(shape, [TILE, bs, bs + TILE]), np.int64) - 1]))
    data = F.with_delimiters(data, at)
    starts = [int(x) + 7 * seed for x in F.FOUR_SHAPES[shape][2]] if shape in F.FOUR_SHAPES else [100, bs - 3, bs + TILE - 2]
    starts += [int(x) + 1 for x in at[seed::7][:6]]
    data = F.planted(data, P, [x for x in starts if x + len(P) <= n])
    return F.planted(data, Q, [x + 20 for x in starts[::2] if x + 20 + len(Q) <= n])


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    from libhuffman_amd.codec import GpuCodec
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    codec = GpuCodec(0)
    yield Env(torch, codec, oracle)
    codec.close()


class Run:
    """one case: the static buffers, the decoy's and the real inputs' names, the call, the comparison, what clears up"""

    def __init__(self, slots, decoy, reals, enqueue, check, after=None):
        self.slots, self.decoy, self.reals, self.enqueue, self.check, self.after = slots, decoy, reals, enqueue, check, after


def full(env, n, value, dtype):
    return env.torch.full((n,), value, dtype=dtype, device="cuda")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "differ at", bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def check_sub(buf, words, inp, what):
    """a sub-index written into the front of a guard-filled buffer: the written set as the CPU reference has it, nothing else"""
    got = buf.cpu().numpy().view(np.uint8)
    fill = np.full(got.size, GUARD, np.uint8)
    assert R.mismatches(got, inp.exp) == [], (what, "(block, array, index, found, expected)")
    assert R.unwritten_changed(got, fill, inp.exp) == [], (what, "(block, array, index, found, held)")
    assert np.all(got[words * 8:] == GUARD), (what, "guard behind the sub-index")


# ---- the calls -------------------------------------------------------------------------------------------------------------
def run_encode(env, shape, sub, sync, codec=None):
    torch, codec, ins = env.torch, codec or env.codec, env.ins(shape)
    slots = Slots(torch, ins, "S", ["A", "C"], same_length=False)
    n, bs, nb = slots.n, slots.bs, slots.nb
    bound, words = codec.encode_bound(n, bs), -(-codec.sub_index_bytes(n, bs) // 8)

    def enqueue():
        out = full(env, bound + G, GUARD, torch.uint8)
        offs = full(env, nb + 3, GUARD64, torch.int64)
        subbuf = full(env, words + 8, GUARD64, torch.int64) if sub else None
        r = codec.encode(slots.data, bs, out=out[:bound], offsets=offs[:nb + 1], sync=sync, sub_index=subbuf[:words] if sub else None)
        return out, offs, subbuf, r[2]

    def check(outs, name):
        inp = ins[name]
        out, offs, subbuf, length = outs
        assert length == (inp.length if sync else None), (name, length)
        o = offs.cpu().numpy()
        same(o[:nb + 1], inp.offs, (name, "index"))
        assert np.all(o[nb + 1:] == GUARD64), (name, "guard behind the index")
        h = out.cpu().numpy()
        same(h[:inp.length], inp.stream, (name, "stream"))
        assert np.all(h[bound:] == GUARD), (name, "guard behind the stream")
        if sub:
            check_sub(subbuf, words, inp, name)

    return Run(slots, "S", ["A", "C"], enqueue, check)


def run_decode(env, shape, sub, sync, codec=None):
    torch, codec, ins = env.torch, codec or env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb

    def enqueue():
        out = full(env, n + 2 * G, GUARD, torch.uint8)
        kw = dict(sub_index=slots.sub, raw_size=n, blocksize=bs) if sub else {}
        return out, codec.decode(slots.stream, slots.length, slots.offsets, nb, out[G:G + n], sync=sync, **kw)

    def check(outs, name):
        h = outs[0].cpu().numpy()
        assert outs[1] == (n if sync else None), (name, outs[1])
        same(h[G:G + n], ins[name].data, (name, "decoded bytes"))
        assert np.all(h[:G] == GUARD) and np.all(h[G + n:] == GUARD), (name, "output guard")

    def after():
        if not sync:
            assert codec.decode_result() == n
        if sub:
            assert codec.decode_counters()[0] == 0          # its own sub-index: no block for the exact decoder

    return Run(slots, "D", ["A", "B"], enqueue, check, after)


def run_histogram(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "C"], same_length=False)
    n, bs, nb = slots.n, slots.bs, slots.nb

    def check(outs, name):
        d = ins[name].data
        want = np.stack([np.bincount(d[b * bs:(b + 1) * bs], minlength=256) for b in range(nb)]).astype(np.int32)
        same(outs[0].cpu().numpy(), want, (name, "histogram"))

    return Run(slots, "D", ["A", "C"], lambda: (codec.histogram(slots.data, bs),), check)


def records_of(shape, seed=5):
    """(positions, lengths, max_len): records across lane, tile and block seams, at 0, up to, across and behind the end"""
    bs, n = SHAPES[shape]
    max_len = 2100 if bs > TILE else 150
    rng = np.random.default_rng(seed)
    pos = [0, n - 5, n, n + 5, max(0, n - max_len)] + [max(0, x - 3) for x in F.SEAMS[shape]] + [int(x) for x in rng.integers(0, n, 40)]
    lens = [int(x) for x in rng.integers(0, max_len + 1, len(pos))]
    lens[:6] = [max_len, 30, 1, 9, max_len, 40]
    return pos, lens, max_len


def run_gather(env, shape, slots=None, seed=5, codec=None):
    torch, codec, ins = env.torch, codec or env.codec, env.ins(shape)
    slots = slots or Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb
    pos, lens, max_len = records_of(shape, seed)
    stride, lead = max_len + 5, 3
    d_pos = torch.tensor(pos, dtype=torch.int64).cuda()
    d_lens = torch.tensor(lens, dtype=torch.int32).cuda()
    torch.cuda.synchronize()

    def enqueue():
        buf = full(env, lead + len(pos) * stride + 9, GUARD, torch.uint8)
        out = buf[lead:lead + len(pos) * stride].view(len(pos), stride)
        _, errs, raws = codec.gather(slots.stream, slots.length, slots.offsets, nb, d_pos, d_lens, sub_index=slots.sub,
                                     raw_size=n, blocksize=bs, max_len=max_len, out=out)
        return buf, errs, raws

    def check(outs, name):
        d = ins[name].data
        got, errs, raws = (t.cpu().numpy() for t in outs)
        want = np.full(got.size, GUARD, np.uint8)
        cuts = [min(ln, n - p) if p < n else 0 for p, ln in zip(pos, lens)]
        for i, (p, c) in enumerate(zip(pos, cuts)):
            want[lead + i * stride:lead + i * stride + c] = d[p:p + c]
        assert not errs.any(), (name, np.flatnonzero(errs)[:8], errs[errs != 0][:8])
        same(raws, np.array(cuts, np.int32), (name, "record lengths"))
        same(got, want, (name, "records and guards"))

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_find(env, shape, name, key, model, direct, slots=None, codec=None, call=None, **kw):
    """`model(data, cap)` is the CPU model's answer; the cap holds all of A's answer and 7 more.  `call(torch, codec, slots, cap)`: the
    enqueue half of one of the younger calls' own helpers, in the place of find_enqueue"""
    torch, codec, ins = env.torch, codec or env.codec, env.ins(shape)
    slots = slots or Slots(torch, ins, "D", ["A", "B"])
    answers = {nm: F.model_parts(model(ins[nm].data, slots.n)) for nm in ("A", "B", "D")}
    cap = int(answers["A"][3][0]) + 7
    assert int(answers["A"][3][0]) >= 3 and int(answers["B"][3][0]) >= 3, (name, "the planted inputs hold too little")
    assert all(not np.array_equal(answers["A"][0], answers[nm][0]) for nm in ("B", "D")), (name, "two inputs with one answer")

    def enqueue():
        if call is not None:
            return call(torch, codec, slots, cap)
        return find_enqueue(torch, codec, slots, name, key, cap, direct=direct, **kw)

    def check(outs, nm):
        F.check(find_fetch(outs), model(ins[nm].data, cap), cap, (name, shape, nm))

    return Run(slots, "D", ["A", "B"], enqueue, check)


def bs_of(shape):
    return SHAPES[shape][0]


# the eleven C calls: name -> (what find_enqueue passes on, the model)
def c_call(name, shape):
    bs = bs_of(shape)
    rec = dict(delims=DELIMS, max_len=40)
    table = {
        "find_bytes": ([NL, P[0]], {}, lambda d, cap: find_model(d, [NL, P[0]], bs, cap)),
        "find_pattern": (P, {}, lambda d, cap: find_pattern_model(d, P, bs, cap)),
        "find_records": (P, rec, lambda d, cap: find_records_model(d, P, DELIMS, bs, cap, 40)),
        "find_classes": (CLASSES, {}, lambda d, cap: find_classes_model(d, CLASSES, bs, cap)),
        "find_records_classes": (CLASSES, rec, lambda d, cap: find_class_records_model(d, CLASSES, DELIMS, bs, cap, 40)),
        "find_any": (ALTS, {}, lambda d, cap: find_any_model(d, ALTS, bs, cap)),
        "find_records_any": (ALTS, rec, lambda d, cap: find_any_records_model(d, ALTS, DELIMS, bs, cap, 40)),
        "find_records_select": (ALTS, dict(rec, invert=True),
                                lambda d, cap: find_select_model(d, ALTS, DELIMS, bs, cap, 40, invert=True)),
        "find_records_context": (ALTS, dict(rec, before=1, after=2),
                                 lambda d, cap: find_context_model(d, ALTS, DELIMS, bs, cap, 40, before=1, after=2)),
        "find_any_anchored": (ALTS, dict(delims=DELIMS, anchors=BOL),
                              lambda d, cap: find_any_anchored_model(d, ALTS, DELIMS, W, BOL, bs, cap)),
        "find_records_anchored": (ALTS, dict(rec, anchors=BOL, before=1, after=1),
                                  lambda d, cap: find_records_anchored_model(d, ALTS, DELIMS, W, BOL, bs, cap, 40, before=1, after=1)),
    }
    return table[name]


# the five younger calls, which tests/find_calls.py does not describe: name -> (the enqueue half of the call's own helper, the model)
OPT_P = lit(P, optional=(2,))           # P with its third byte optional: both forms are planted nowhere but P's own
TERMS = [[P], [Q]]                      # P and Q in one record; Q lies 20 bytes behind every second P
EXPR_TERMS = [[lit(P)], [lit(Q, optional=(1,))]]


def younger_call(name, shape):
    bs = bs_of(shape)
    rec = dict(delims=DELIMS, max_len=40, before=1, after=1, fetch=False)
    table = {
        "find_records_terms": (lambda t, c, e, cap: terms_call(t, c, e, TERMS, TERMS_ALL, cap, **rec),
                               lambda d, cap: find_terms_model(d, TERMS, DELIMS, bs, cap, 40, before=1, after=1, mode=TERMS_ALL)),
        "find_any_quant": (lambda t, c, e, cap: quant_call(t, c, e, "find_any_quant", [OPT_P, lit(Q)], cap, fetch=False),
                           lambda d, cap: find_quant_model(d, [OPT_P, lit(Q)], bs, cap)),
        "find_records_quant": (lambda t, c, e, cap: quant_call(t, c, e, "find_records_quant", [OPT_P, lit(Q)], cap, **rec),
                               lambda d, cap: find_quant_records_model(d, [OPT_P, lit(Q)], DELIMS, bs, cap, 40, before=1, after=1)),
        "find_any_expr": (lambda t, c, e, cap: expr_call(t, c, e, "find_any_expr", [[OPT_P, lit(Q)]], cap, anchors=BOL, delims=DELIMS,
                                                      fetch=False),
                          lambda d, cap: find_any_expr_model(d, [OPT_P, lit(Q)], DELIMS, W, BOL, bs, cap)),
        "find_records_expr": (lambda t, c, e, cap: expr_call(t, c, e, "find_records_expr", EXPR_TERMS, cap, mode=TERMS_ORDERED, **rec),
                              lambda d, cap: find_records_expr_model(d, EXPR_TERMS, DELIMS, W, 0, TERMS_ORDERED, bs, cap, 40, before=1,
                                                                     after=1)),
    }
    return table[name]


YOUNGER = ("find_records_terms", "find_any_quant", "find_records_quant", "find_any_expr", "find_records_expr")


def run_c_call(env, shape, name, **more):
    if name in YOUNGER:
        call, model = younger_call(name, shape)
        return run_find(env, shape, name, None, model, True, call=call, **more)
    key, kw, model = c_call(name, shape)
    return run_find(env, shape, name, key, model, True, **kw, **more)


def run_method(env, shape, name, **more):
    bs = bs_of(shape)
    if name == "find_bytes":
        return run_find(env, shape, name, [NL, Q[0]], lambda d, cap: find_model(d, [NL, Q[0]], bs, cap), False, **more)
    if name == "find_pattern":
        return run_find(env, shape, name, Q, lambda d, cap: find_pattern_model(d, Q, bs, cap), False, **more)
    return run_find(env, shape, name, Q, lambda d, cap: find_records_model(d, Q, DELIMS, bs, cap, 0), False, delims=DELIMS, **more)


# (id, the method or C call it stands for, the builder)
ENQUEUE_ONLY = (
    [(f"encode-{s}", "encode", lambda e, s=s: run_encode(e, s, False, False)) for s in SHAPES] +
    [(f"encode_sub-{s}", "encode+sub_index", lambda e, s=s: run_encode(e, s, True, False)) for s in SHAPES] +
    [(f"decode-{s}", "decode", lambda e, s=s: run_decode(e, s, False, False)) for s in SHAPES] +
    [(f"decode_sub-{s}", "decode+sub_index", lambda e, s=s: run_decode(e, s, True, False)) for s in SHAPES] +
    [(f"histogram-{s}", "histogram", lambda e, s=s: run_histogram(e, s)) for s in SHAPES] +
    [(f"gather-{s}", "gather", lambda e, s=s: run_gather(e, s)) for s in SMALL] +
    [(f"{m}-{s}", "method " + m, lambda e, s=s, m=m: run_method(e, s, m)) for m in F.METHODS for s in SMALL] +
    [(f"hufgpu_{c}-{s}", c, lambda e, s=s, c=c: run_c_call(e, s, c)) for c in tuple(CALLS) + YOUNGER for s in SMALL])
ENQUEUE_ONLY_COVERS = ["encode", "encode+sub_index", "decode", "decode+sub_index", "histogram", "gather"] + \
                      ["method " + m for m in ("find_bytes", "find_pattern", "find_records")]


@pytest.fixture(scope="module")
def side_stream_is_non_blocking(env):
    assert stream_flags(env.s) & HIP_STREAM_NON_BLOCKING, "torch's side stream is ordered with the null stream: the gate shows nothing"
    assert env.s.cuda_stream != 0 and env.torch.cuda.current_stream().cuda_stream != env.s.cuda_stream


def test_the_side_stream_is_non_blocking(env, side_stream_is_non_blocking):
    pass


def test_every_call_has_a_case():
    """every C call of the search family and every listed method stands in Part 1 and in Part 2 (they share ENQUEUE_ONLY), and
    every call that waits inside stands in Part 1: a twelfth search call needs a stream case"""
    from libhuffman_amd import _native
    declared = {sym[len("hufgpu_"):] for sym in _native.GPU_SYMBOLS if sym.startswith("hufgpu_find_")}
    assert set(CALLS) <= declared and set(CALLS) | set(YOUNGER) == declared, declared ^ (set(CALLS) | set(YOUNGER))
    covered = {c for _, c, _ in ENQUEUE_ONLY}
    assert covered == declared | set(ENQUEUE_ONLY_COVERS), (declared | set(ENQUEUE_ONLY_COVERS)) ^ covered
    assert {c for _, c, _ in WAITS_INSIDE} == set(WAITS_INSIDE_COVERS)


# ---- Part 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ENQUEUE_ONLY, ids=[c[0] for c in ENQUEUE_ONLY])
def test_gate_enqueue_only(env, side_stream_is_non_blocking, case):
    run = case[2](env)
    env.gate.run(case[0], env.s, run.slots, run.decoy, run.reals[0], run.enqueue, run.check, True)
    if run.after:
        run.after()


def run_encode_batch(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "S", ["A", "C"], same_length=False)
    n, bs = slots.n, slots.bs
    item_lens = [2 * bs + 5, 0, bs - 7, n - 3 * bs + 2]

    def check(batch, name):
        d, at, want, offs = ins[name].data, 0, [], [0]
        for ln in item_lens:
            if ln:
                want.append(env.oracle.encode(d[at:at + ln], bs))
            offs.append(offs[-1] + (want[-1].size if ln else 0))
            at += ln
        assert batch.item_offsets == offs, (name, batch.item_offsets, offs)
        same(batch.stream.cpu().numpy(), np.concatenate(want), (name, "the batch's stream"))
        assert batch.sub_index is not None and batch.item_blocks[-1] == sum(codec.block_count(ln, bs) for ln in item_lens)

    return Run(slots, "S", ["A", "C"], lambda: codec.encode_batch(slots.data, item_lens, bs, sub_index=True), check)


def run_decode_batch(env, shape):
    from libhuffman_amd.codec import EncodedBatch
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb
    blocks = [0, 2, nb]                                     # two items of whole blocks of the one stream
    lens = [2 * bs, n - 2 * bs]
    batch = EncodedBatch(slots.stream, slots.offsets, blocks, [0, 0, slots.length], lens, bs, 0)

    def enqueue():
        out = full(env, n + G, GUARD, torch.uint8)
        return (out,) + tuple(codec.decode_batch(batch, out=out)[1:])

    def check(outs, name):
        h = outs[0].cpu().numpy()
        assert outs[1] == [0, 0] and outs[2] == lens, (name, outs[1:])
        same(h[:n], ins[name].data, (name, "decoded items"))
        assert np.all(h[n:] == GUARD), name

    return Run(slots, "D", ["A", "B"], enqueue, check)


def ranges_of(shape):
    bs, n = SHAPES[shape]
    return [(0, 9), (bs - 3, bs + 20), (bs + bs // 2, 2 * bs + 5), (3 * bs + 1, 3 * bs + 2), (n - 17, n)]


def run_decode_ranges(env, shape, tiles, slots=None):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = slots or Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb
    ranges = ranges_of(shape)
    total = sum(hi - lo for lo, hi in ranges)

    def enqueue():
        out = full(env, total + G, GUARD, torch.uint8)
        return codec.decode_ranges(slots.stream, slots.length, slots.offsets, nb, ranges, out=out, sub_index=slots.sub, raw_size=n,
                                   blocksize=bs, tiles=tiles)

    def check(outs, name):
        d = ins[name].data
        h = outs[0].cpu().numpy()
        assert outs[1] == [0] * len(ranges) and outs[2] == [hi - lo for lo, hi in ranges], (name, outs[1:])
        same(h[:total], np.concatenate([d[lo:hi] for lo, hi in ranges]), (name, "ranges"))
        assert np.all(h[total:] == GUARD), name

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_update_ranges(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb
    ranges = ranges_of(shape)[:4]
    patch = datagen.zipf255(sum(hi - lo for lo, hi in ranges), seed=9)
    d_patch = torch.from_numpy(patch).cuda()
    torch.cuda.synchronize()

    def enqueue():
        return codec.update_ranges(slots.stream, slots.length, slots.offsets, nb, ranges, d_patch, sub_index=slots.sub, raw_size=n,
                                   blocksize=bs, want_sub_index=True)

    def check(outs, name):
        new, at = ins[name].data.copy(), 0
        for lo, hi in ranges:
            new[lo:hi] = patch[at:at + hi - lo]
            at += hi - lo
        want = Input(env.oracle, new, bs)
        stream, length, offs, sub, count = outs
        assert length == want.length, (name, length, want.length)
        same(stream.cpu().numpy(), want.stream, (name, "new stream"))
        same(offs.cpu().numpy(), want.offs, (name, "new index"))
        assert R.mismatches(sub.cpu().numpy().view(np.uint8), want.exp) == [], name
        assert count == len({b for lo, hi in ranges for b in range(lo // bs, (hi - 1) // bs + 1)}), (name, count)

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_append(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    bs, n = SHAPES[shape]
    more = datagen.zipf255(bs + 77, seed=10)
    tail = n % bs
    extra_blocks = codec.block_count(n + more.size, bs) - codec.block_count(n, bs)
    slots = Slots(torch, ins, "D", ["A", "B"], extra_stream=codec.encode_bound(tail + more.size, bs), extra_blocks=extra_blocks)
    d_more = torch.from_numpy(more).cuda()
    torch.cuda.synchronize()

    def enqueue():
        r = codec.append(slots.stream, slots.length, slots.offsets, n, bs, d_more, sub_index=slots.sub, new_sub_index=True)
        assert r[0] is slots.stream and r[1] is slots.offsets        # in place
        return r

    def check(outs, name):
        want = Input(env.oracle, np.concatenate([ins[name].data, more]), bs)
        assert outs[2:4] == (want.length, n + more.size), (name, outs[2:4])
        same(outs[0][:want.length].cpu().numpy(), want.stream, (name, "stream"))
        same(outs[1].cpu().numpy(), want.offs, (name, "index"))
        assert R.mismatches(outs[4].cpu().numpy().view(np.uint8), want.exp) == [], name

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_truncate(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs = slots.n, slots.bs
    keep = 2 * bs + bs // 3

    def enqueue():
        return codec.truncate(slots.stream, slots.length, slots.offsets, n, bs, keep, sub_index=slots.sub, new_sub_index=True)

    def check(outs, name):
        want = Input(env.oracle, ins[name].data[:keep], bs)
        assert outs[2:4] == (want.length, keep), (name, outs[2:4])
        same(outs[0][:want.length].cpu().numpy(), want.stream, (name, "stream"))
        same(outs[1][:want.nb + 1].cpu().numpy(), want.offs, (name, "index"))
        assert R.mismatches(outs[4].cpu().numpy().view(np.uint8), want.exp) == [], name

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_build_sub_index(env, shape, with_decode):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs = slots.n, slots.bs
    words = -(-codec.sub_index_bytes(n, bs) // 8)

    def enqueue():
        buf = full(env, words + 8, GUARD64, torch.int64)
        if with_decode:
            out = full(env, n + G, GUARD, torch.uint8)
            raw, _, unbuilt = codec.decode_build_sub(slots.stream, slots.length, slots.offsets, out[:n], n, bs, sub_index=buf[:words])
            return buf, unbuilt, out, raw
        return buf, codec.build_sub_index(slots.stream, slots.length, slots.offsets, n, bs, sub_index=buf[:words])[1]

    def check(outs, name):
        assert outs[1] == 0, (name, "blocks without rows", outs[1])
        check_sub(outs[0], words, ins[name], name)
        if with_decode:
            h = outs[2].cpu().numpy()
            assert outs[3] == n, (name, outs[3])
            same(h[:n], ins[name].data, (name, "decoded bytes"))
            assert np.all(h[n:] == GUARD), name

    return Run(slots, "D", ["A", "B"], enqueue, check)


def run_decode_stream(env, shape):
    torch, codec, ins = env.torch, env.codec, env.ins(shape)
    slots = Slots(torch, ins, "S", ["A", "B"])              # a raw stream has no index to bound a read: a decoy of A's length
    n = slots.n

    def enqueue():
        out = full(env, n + G, GUARD, torch.uint8)
        return (out,) + codec.decode_stream(slots.stream, slots.length, slots.length, out[:n])

    def check(outs, name):
        h = outs[0].cpu().numpy()
        assert outs[1:] == (OK, n, slots.length), (name, outs[1:])
        same(h[:n], ins[name].data, (name, "decoded bytes"))
        assert np.all(h[n:] == GUARD), name

    return Run(slots, "S", ["A", "B"], enqueue, check)


WAITS_INSIDE = (
    [(f"encode_sync-{s}", "encode sync", lambda e, s=s: run_encode(e, s, s != "300x64", True)) for s in SHAPES] +
    [(f"decode_sync-{s}", "decode sync", lambda e, s=s: run_decode(e, s, s != "300x64", True)) for s in SHAPES] +
    [("encode_batch-5x4099", "encode_batch", lambda e: run_encode_batch(e, "5x4099")),
     ("decode_batch-5x4099", "decode_batch", lambda e: run_decode_batch(e, "5x4099"))] +
    [(f"decode_ranges-{s}", "decode_ranges", lambda e, s=s: run_decode_ranges(e, s, False)) for s in SMALL] +
    [(f"decode_ranges_tiles-{s}", "decode_ranges tiles", lambda e, s=s: run_decode_ranges(e, s, True)) for s in SMALL] +
    [(f"update_ranges-{s}", "update_ranges", lambda e, s=s: run_update_ranges(e, s)) for s in SMALL] +
    [(f"append-{s}", "append", lambda e, s=s: run_append(e, s)) for s in SMALL] +
    [(f"truncate-{s}", "truncate", lambda e, s=s: run_truncate(e, s)) for s in SMALL] +
    [(f"build_sub_index-{s}", "build_sub_index", lambda e, s=s: run_build_sub_index(e, s, False)) for s in SHAPES] +
    [(f"decode_build_sub-{s}", "decode_build_sub", lambda e, s=s: run_build_sub_index(e, s, True)) for s in SHAPES] +
    [(f"decode_stream-{s}", "decode_stream", lambda e, s=s: run_decode_stream(e, s)) for s in ("5x4099", "3x65536")])
WAITS_INSIDE_COVERS = ["encode sync", "decode sync", "encode_batch", "decode_batch", "decode_ranges", "decode_ranges tiles",
                       "update_ranges", "append", "truncate", "build_sub_index", "decode_build_sub", "decode_stream"]


@pytest.mark.parametrize("case", WAITS_INSIDE, ids=[c[0] for c in WAITS_INSIDE])
def test_gate_calls_that_wait_inside(env, side_stream_is_non_blocking, case):
    run = case[2](env)
    env.gate.run(case[0], env.s, run.slots, run.decoy, run.reals[0], run.enqueue, run.check, False)
    if run.after:
        run.after()


# ---- one context across streams --------------------------------------------------------------------------------------------
def blocks_with_stale_rows(own, other):
    """the blocks whose tile or group entries differ between two sub-indexes of one layout.  decode_sub_kernel starts a
    group where the entries in front of it sum to, and accepts a block only when every group takes the bits its entry claims
    and every tile starts where its entry says: up to the first wrong entry the walk is the true one, so that entry is seen.
    Each such block goes to the exact decoder, and no other does (SubCase.fix of tests/sub_index_ref.py is 0 for these
    trees)."""
    lay = own.lay
    return sum(1 for b in range(lay.nb)
               if not np.array_equal(own.tiles[b * lay.tpb:(b + 1) * lay.tpb], other.tiles[b * lay.tpb:(b + 1) * lay.tpb]) or
               not np.array_equal(own.groups[b * lay.gpb:(b + 1) * lay.gpb], other.groups[b * lay.gpb:(b + 1) * lay.gpb]))


def test_decode_result_and_counters_wait_for_the_call_s_stream(env, side_stream_is_non_blocking):
    """decode(sync=False) on s1 behind a gate with a STALE sub-index - B's, for A's stream: the same trees and index, other
    bit positions.  decode_result() and decode_counters() are then called with the default stream current: both must wait
    for s1 and report THIS call's bytes and THIS call's blocks for the exact decoder.  The warm-up - the decoy with its own
    sub-index - left 0 such blocks behind.  Then the same context serves the default stream and a second side stream, the
    host having waited in between."""
    torch, codec, gate = env.torch, env.codec, env.gate
    ins = env.ins("5x4099")
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, bs, nb = slots.n, slots.bs, slots.nb
    stale = torch.from_numpy(ins["B"].sub.view(np.int64)).cuda()
    torch.cuda.synchronize()
    want_fix = blocks_with_stale_rows(ins["A"].exp, ins["B"].exp)
    assert want_fix == nb, (want_fix, nb)
    outs = []

    def enqueue(sub):
        outs.append(full(env, n + 2 * G, GUARD, torch.uint8))
        codec.decode(slots.stream, slots.length, slots.offsets, nb, outs[-1][G:G + n], sync=False, sub_index=sub, raw_size=n, blocksize=bs)

    def decoded(name, what):
        h = outs[-1].cpu().numpy()
        same(h[G:G + n], ins[name].data, what)
        assert np.all(h[:G] == GUARD) and np.all(h[G + n:] == GUARD), what

    _, gate_ms = gate.warm_up(slots, "D", lambda: enqueue(slots.sub))
    assert codec.decode_result() == n and codec.decode_counters()[0] == 0
    s1, s2 = env.s, torch.cuda.Stream()
    gate.prime(s1, slots, "D", lambda: enqueue(slots.sub))
    assert codec.decode_result() == n and codec.decode_counters()[0] == 0
    with gate.quiet(), torch.cuda.stream(s1):
        opened = gate.close(s1, gate_ms)
        slots.load("A")
        enqueue(stale)
        closed = not opened.query()
    assert torch.cuda.current_stream().cuda_stream != s1.cuda_stream
    raw = codec.decode_result()                             # the default stream is current: this waits for s1
    assert opened.query(), "decode_result returned before the call's stream had run"
    fixed = codec.decode_counters()[0]
    assert closed, ("the gate had opened before decode returned: this run has proved nothing", gate_ms)
    assert (raw, fixed) == (n, want_fix), (raw, fixed)
    with torch.cuda.stream(s1):
        decoded("A", "decoded with a stale sub-index on s1")
    # the default stream: B's stream with B's sub-index, no block for the exact decoder
    slots.load("B")
    enqueue(stale)
    assert (codec.decode_result(), codec.decode_counters()[0]) == (n, 0)
    decoded("B", "on the default stream")
    torch.cuda.synchronize()
    # a second side stream: the stale sub-index again, pending behind a gate while the counters are asked for.  s2 is NOT
    # primed: the context's last stream is the default one until this call, so a decode that forgot to note its stream would
    # leave the two calls below waiting for the wrong one (no gate is looked at here, so a slow first launch does no harm)
    opened = gate.close(s2, gate_ms)
    with torch.cuda.stream(s2):
        slots.load("A")
        enqueue(stale)
    assert codec.decode_counters()[0] == want_fix and opened.query()
    assert codec.decode_result() == n
    with torch.cuda.stream(s2):
        decoded("A", "on the second side stream")


def test_ranges_counters_from_the_default_stream(env, side_stream_is_non_blocking):
    """decode_ranges by tiles on s1, then ranges_counters() with the default stream current: this call's routing, as the rule
    of include/huffman_gpu.h gives it (the model of tests/stream_support.py), not what the warm-up without the flag left"""
    import types
    shape = "5x4099"
    bs, n = SHAPES[shape]
    run = run_decode_ranges(env, shape, True)
    direct = run_decode_ranges(env, shape, False, slots=run.slots)
    ranges = ranges_of(shape)
    oo = np.concatenate([[0], np.cumsum([hi - lo for lo, hi in ranges])]).tolist()
    nb = run.slots.nb
    lay = types.SimpleNamespace(nb=nb, n=n, bs=bs, P=np.minimum(np.arange(nb + 1) * bs, n), elig=np.full(nb, True),
                                block_lens=np.diff(np.minimum(np.arange(nb + 1) * bs, n)))
    want = ranges_route_model(lay, ranges, oo)
    assert want[2] >= 2 and want[3] > want[2], want          # blocks served by tiles, and more (range, tile) items than blocks
    run.slots.load("D")
    direct.enqueue()
    assert env.codec.ranges_counters()[2:5] == (0, 0, 0)
    env.gate.run("ranges_counters", env.s, run.slots, "D", "A", run.enqueue, run.check, False)
    assert env.codec.ranges_counters() == want + (0, 0, 0, 0)


# ---- a fresh context on a side stream ----------------------------------------------------------------------------------------
def first_calls_ms(env, build):
    """the host time of a new context's first calls, growth included, on the decoy on the null stream: a throw-away context"""
    import time

    from libhuffman_amd.codec import GpuCodec
    codec = GpuCodec(0)
    try:
        runs = build(codec)
        for run in runs:
            run.slots.load(run.decoy)
        env.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for run in runs:
            run.enqueue()
        ms = (time.perf_counter() - t0) * 1e3
        env.torch.cuda.synchronize()
        return ms
    finally:
        codec.close()


def fresh(env, build):
    """A new context whose very first calls are enqueued on the side stream behind a gate: every workspace grows inside the
    calls, so each growth waits for the device - and with it for the gate.  The context under test has no warm-up; the gate
    is sized as everywhere, by the same first calls of a throw-away context.  The static buffers hold the decoy until the
    gated copies."""
    from libhuffman_amd.codec import GpuCodec
    torch, gate = env.torch, env.gate
    host_ms = first_calls_ms(env, build)
    gate_ms = max(MIN_GATE_MS, GATE_FACTOR * host_ms)
    print(f"[gate] a fresh context: first calls {host_ms:.3f} ms, gate {gate_ms:.1f} ms")
    codec = GpuCodec(0)
    try:
        runs = build(codec)
        for run in runs:
            run.slots.load(run.decoy)
        torch.cuda.synchronize()
        gate.close(env.s, gate_ms)
        with torch.cuda.stream(env.s):
            outs = []
            for run in runs:
                run.slots.load(run.reals[0])
                outs.append(run.enqueue())
            env.s.synchronize()
            for run, o in zip(runs, outs):
                run.check(o, run.reals[0])
    finally:
        codec.close()


def test_a_fresh_context_encodes_and_decodes_on_a_side_stream(env, side_stream_is_non_blocking):
    fresh(env, lambda codec: [run_encode(env, "5x4099", True, False, codec=codec), run_decode(env, "5x4099", True, False, codec=codec)])


def test_a_fresh_context_gathers_on_a_side_stream(env, side_stream_is_non_blocking):
    fresh(env, lambda codec: [run_gather(env, "300x64", codec=codec)])


def test_a_fresh_context_finds_records_on_a_side_stream(env, side_stream_is_non_blocking):
    fresh(env, lambda codec: [run_method(env, "300x64", "find_records", codec=codec)])


def test_a_gather_that_grows_the_workspace_behind_a_pending_one(env, side_stream_is_non_blocking):
    """a context that has gathered from 5 blocks only; a gather of that size pending behind the gate, then on the same stream
    one over 300 blocks, which makes the gather groups grow while the first has not run: both right"""
    from libhuffman_amd.codec import GpuCodec
    torch, gate = env.torch, env.gate
    codec = GpuCodec(0)
    try:
        small, large = run_gather(env, "5x4099", codec=codec), run_gather(env, "300x64", codec=codec, seed=6)
        # host/workspace.hpp, WS_DOUBLE: the first call leaves room for max(need, 2 x 0) + 16 blocks
        assert large.slots.nb > small.slots.nb + 16, "the second gather would not grow the gather groups"
        _, gate_ms = gate.warm_up(small.slots, "D", small.enqueue)
        gate.prime(env.s, small.slots, "D", small.enqueue)
        large.slots.load("D")
        torch.cuda.synchronize()
        with gate.quiet(), torch.cuda.stream(env.s):
            opened = gate.close(env.s, gate_ms)
            small.slots.load("A")
            large.slots.load("A")
            first = small.enqueue()
            closed = not opened.query()
        with torch.cuda.stream(env.s):
            second = large.enqueue()
            grew = opened.query()       # a growth waits for the device, the gate included: an enqueue-only call would not
            env.s.synchronize()
            small.check(first, "A")
            large.check(second, "A")
        assert closed, "the gate had opened before the first gather returned: the second found nothing pending"
        assert grew, "the second gather returned with the gate closed: it has not grown a workspace"
    finally:
        codec.close()


# ---- two contexts, two streams -----------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved(env, side_stream_is_non_blocking):
    """the module's codec encodes and decodes on s1, a second codec finds and gathers on s2, each behind a gate of its own, the
    enqueues interleaved from one thread: the one place where device state that all contexts share would show"""
    from libhuffman_amd.codec import GpuCodec
    torch, gate = env.torch, env.gate
    other = GpuCodec(0)
    try:
        s1, s2 = env.s, torch.cuda.Stream()
        on1 = [run_encode(env, "5x4099", True, False), run_decode(env, "5x4099", True, False)]
        on2 = [run_method(env, "5x4099", "find_records", codec=other), run_gather(env, "5x4099", codec=other)]
        ms = 2 * max(gate.warm_up(run.slots, run.decoy, run.enqueue)[1] for run in on1 + on2)     # the warm-ups, on the null stream
        for stream, runs in ((s1, on1), (s2, on2)):
            for run in runs:
                gate.prime(stream, run.slots, run.decoy, run.enqueue)
        assert env.codec.decode_result() == on1[1].slots.n
        outs = []
        with gate.quiet():
            opened1, opened2 = gate.close(s1, ms), gate.close(s2, ms)
            for r1, r2 in zip(on1, on2):
                with torch.cuda.stream(s1):
                    r1.slots.load("A")
                    outs.append(r1.enqueue())
                with torch.cuda.stream(s2):
                    r2.slots.load("A")
                    outs.append(r2.enqueue())
            closed = not opened1.query() and not opened2.query()
        s1.synchronize()
        s2.synchronize()
        assert closed, ("a gate had opened before the last call returned: this run has proved nothing", ms)
        for k, run in enumerate([on1[0], on2[0], on1[1], on2[1]]):
            with torch.cuda.stream(s2 if k % 2 else s1):
                run.check(outs[k], "A")
        assert env.codec.decode_result() == on1[1].slots.n
    finally:
        other.close()


# ---- Part 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ENQUEUE_ONLY, ids=[c[0] for c in ENQUEUE_ONLY])
def test_capture_and_replay_twice(env, side_stream_is_non_blocking, case):
    run = case[2](env)
    env.gate.capture(case[0], env.s, run.slots, run.decoy, run.reals, run.enqueue, run.check)
    env.codec.decode_result()                               # (a captured decode left the context "pending")


def test_capture_find_records_then_gather(env, side_stream_is_non_blocking):
    """the pipeline the enqueue-only calls were built for, as one graph: find_records' positions and lengths go to gather on
    the device; rows behind the written records are given length 0 by a device op, as GpuCodec.grep does"""
    torch, codec = env.torch, env.codec
    shape = "5x4099"
    ins, bs = env.ins(shape), bs_of(shape)
    slots = Slots(torch, ins, "D", ["A", "B"])
    n, nb, max_len = slots.n, slots.nb, 40
    model = lambda d, cap: find_records_model(d, P, DELIMS, bs, cap, max_len)
    cap = int(model(ins["A"].data, n)[3][0]) + 7
    stride, lead = max_len + 5, 3

    def enqueue():
        found = find_enqueue(torch, codec, slots, "find_records", P, cap, delims=DELIMS, max_len=max_len)
        pos, lens, totals = found[0][F.LEAD:F.LEAD + cap], found[1][F.LEAD:F.LEAD + cap], found[2]
        written = torch.arange(cap, device="cuda") < totals[1]
        buf = full(env, lead + cap * stride + 9, GUARD, torch.uint8)
        _, errs, raws = codec.gather(slots.stream, slots.length, slots.offsets, nb, torch.where(written, pos, n),
                                     torch.where(written, lens, 0), sub_index=slots.sub, raw_size=n, blocksize=bs, max_len=max_len,
                                     out=buf[lead:lead + cap * stride].view(cap, stride))
        return found, buf, errs, raws

    def check(outs, name):
        d = ins[name].data
        want = model(d, cap)
        F.check(find_fetch(outs[0]), want, cap, ("pipeline", name))
        got, errs, raws = (t.cpu().numpy() for t in outs[1:])
        starts, lens = want[0], np.minimum(want[1].astype(np.int64), max_len)
        rows = np.full(got.size, GUARD, np.uint8)
        for i, (p, ln) in enumerate(zip(starts.tolist(), lens.tolist())):
            rows[lead + i * stride:lead + i * stride + ln] = d[p:p + ln]
        assert not errs.any(), (name, errs)
        same(raws, np.concatenate([lens, np.zeros(cap - lens.size, np.int64)]).astype(np.int32), (name, "row lengths"))
        same(got, rows, (name, "rows and guards"))

    env.gate.capture("find_records -> gather", env.s, slots, "D", ["A", "B"], enqueue, check)

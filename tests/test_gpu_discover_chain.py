"""The raw-stream block discovery (libhuffman_amd/csrc/kernels/discover.hpp) against its CPU restatement
(tests/chain_model.py) on streams that put headers where the kernels' geometry changes (tests/chain_streams.py).

A discovery that loses a candidate, places one out of order or cannot resolve a link still decodes every stream right:
the validated prefix ends early and the in-order decoder takes the rest.  So bytes, error and consumed count - all that
the older raw-stream tests look at - cannot see it.  Here hufgpu_block_index must return the model's chain word by word,
and hufgpu_stream_counters must report the model's candidate count, the chain's block count and, for a plain chain, that
the walk's shortcut and the probes' in-place output were taken.

One departure from the issue that asked for this file: it wants the whole triple (err, raw, used) of
hufgpu_decode_stream compared.  The consumed count is compared where the oracle returns no error, as everywhere in this
suite (tests/test_gpu_parity.py): behind an error the reference's reader position says how far it had buffered, not
where the stream broke.

Word [3] of the read-out, the candidates that went to the exact probe, follows from probe_kernel's own rule: when the
candidates' claimed lengths together do not fit the output (always for hufgpu_block_index, which has none) every
candidate goes there; otherwise at least those with a tree of fewer than nine entries, and none of an intact stream of
the encoder's blocks, which are what the lean probe is for."""
import ctypes as C

import numpy as np
import pytest

import chain_model as cm
import chain_streams as cs
from test_gpu_decode_edges import Guarded

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
RELAXED = 1
OFF = 13                                   # the output's odd byte offset in its guarded buffer


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    yield c
    c.close()


_MODEL = {}


def model(oracle, key, st, avail, length):
    """(candidates, chain, the oracle's decode) of stream[:avail] with `length`, computed once"""
    if key not in _MODEL:
        cands = cm.candidates(st, avail, min(length, avail), cs.MAX_TREE)
        chain = cm.chain(oracle, st, avail, length, cs.MAX_TREE)
        want = oracle.decode(st[:avail], 8 * avail + 64, cs.MAX_TREE, length=length)
        _MODEL[key] = (cands, chain, want)
    return _MODEL[key]


def on_device(torch, st, avail, lead=0):
    """stream[:avail] at byte `lead` of a 16-byte aligned buffer, bytes that are no part of it behind"""
    buf = torch.full((lead + avail + 64,), 0xee, dtype=torch.uint8, device="cuda")
    buf[lead:lead + avail] = torch.from_numpy(st[:avail].copy()).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf[lead:lead + avail + 64]


def block_index(torch, codec, d, avail, length):
    d_index, cnt, used = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
    rc = codec.lib.hufgpu_block_index(codec._ctx, C.c_void_p(d.data_ptr()), C.c_uint64(avail), C.c_uint64(length), C.c_uint32(RELAXED),
                                      C.byref(d_index), C.byref(cnt), C.byref(used), None)
    index = []
    if rc == 0 and cnt.value:
        found = torch.empty(cnt.value + 1, dtype=torch.int64, device="cuda")
        assert codec.lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(found.data_ptr()), d_index, C.c_uint64(8 * (cnt.value + 1))) == 0
        index = found.cpu().numpy().tolist()
    return rc, int(cnt.value), int(used.value), index


def check_index(torch, codec, oracle, name, st, avail, length, d=None):
    """hufgpu_block_index and the read-out against the model; returns the read-out"""
    cands, (index, nblocks, consumed, _), _ = model(oracle, (name, avail, length), st, avail, length)
    d = on_device(torch, st, avail) if d is None else d
    rc, n, used, got = block_index(torch, codec, d, avail, length)
    c = codec.stream_counters()
    print(name, "block_index", (rc, n, used), c, "model", (nblocks, consumed, len(cands)))
    assert (rc, n, used) == (0, nblocks, consumed), (name, (rc, n, used), (nblocks, consumed))
    wrong = [(i, a, b) for i, (a, b) in enumerate(zip(got, index)) if a != b]
    assert len(got) == len(index) and not wrong, (name, len(got), len(index), wrong[:4])
    assert c[0] == 1 and c[1] == len(cands), (name, "candidates found", c[1], "the model's", len(cands))
    assert c[5] == nblocks and c[2] == c[1] and c[6] == NONE and c[7] in (1, 2), (name, c)
    assert c[3] == c[1], (name, "count-only: every candidate takes the exact probe", c)
    return c


def check_decode(torch, codec, oracle, name, st, avail, length, d=None, discovers=True, encoder_only=False):
    """hufgpu_decode_stream, discovering and in order, into a guarded output at an odd offset; returns the read-out of the
    discovering call"""
    cands, (index, nblocks, consumed, complete), (oerr, oout, oused) = model(oracle, (name, avail, length), st, avail, length)
    d = on_device(torch, st, avail) if d is None else d
    plain = complete and cands == index[:-1]
    false_below = any(p < consumed and p not in set(index) for p in cands)
    cap = oout.size + 64
    fields = [(int.from_bytes(st[p:p + 8].tobytes(), "little"), int.from_bytes(st[p + 8:p + 10].tobytes(), "little")) for p in cands]
    store = sum(bl for bl, _ in fields) <= cap               # probe_kernel: the candidates' claimed lengths fit the output
    short_tree = sum(1 for _, tl in fields if tl < 9)
    first = None
    for sequential in (False, True):
        tag = (name, "sequential" if sequential else "parallel")
        g = Guarded(torch, cap, OFF)
        err, raw, used = codec.decode_stream(d, avail, length, g.view, relaxed=True, sequential=sequential)
        c = codec.stream_counters()
        print(*tag, (err, raw, used), c, "oracle", (oerr, oout.size, oused), "plain" if plain else "", "false" if false_below else "")
        assert (err, raw) == (oerr, oout.size), tag + ((err, raw, used), (oerr, oout.size, oused))
        if oerr == 0:
            assert used == oused, tag + (used, oused)
        g.check(raw, oout, tag, touched=cap)
        if sequential or not discovers:
            assert c == (0,) * 8, tag + (c,)
            continue
        first = c
        assert c[0] == 1 and c[1] == len(cands) and c[2] == c[1] and c[5] == nblocks and c[7] in (1, 2), tag + (c, len(cands), nblocks)
        if store:
            assert short_tree <= c[3] <= c[1], tag + ("exact probes", c[3], "trees below nine entries", short_tree)
            assert c[3] == 0 or not encoder_only, tag + ("the lean probe handed on an intact block of the encoder's", c)
        else:
            assert c[3] == c[1], tag + ("count-only: every candidate takes the exact probe", c)
        if nblocks == 0:
            assert c[6] == NONE, tag + (c,)
        if plain:                    # the walk's shortcut, and every byte where the probes left it
            assert c[4] == 0 and c[6] == raw == oout.size, tag + (c,)
        if false_below:
            assert c[4] > 0, tag + (c,)
    return first


ENCODER_ONLY = ("few", "thresholds", "cut-edge", "cut-header", "cut-payload")      # intact streams of the encoder's blocks alone


def check(torch, codec, oracle, name):
    case = cs.get(oracle, name)
    d = on_device(torch, case.stream, case.avail)
    a = check_index(torch, codec, oracle, name, case.stream, case.avail, case.length, d)
    b = check_decode(torch, codec, oracle, name, case.stream, case.avail, case.length, d, encoder_only=name in ENCODER_ONLY)
    return a, b


# ---- a. header positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tree7", "tree67", "planted"])
@pytest.mark.parametrize("edge", ["wave", "row", "workgroup"])
def test_a_headers_around_an_edge(torch_mod, codec, oracle, edge, kind):
    """a header - of a 2-leaf block (exact probe), of a block with 67 tree entries (two steps of the grammar check, lean
    probe), or twelve planted bytes - at every offset of [E - 24, E + 16) around a wave's, a row's and a workgroup's edge E"""
    _, c = check(torch_mod, codec, oracle, f"sweep-{edge}-{kind}")
    if kind == "tree7":
        assert c[3] >= len(cs.DELTAS), c                     # every probed header's block took the exact probe
    if kind == "tree67":
        assert c[3] <= c[1] - len(cs.DELTAS), c              # ... and here the lean one


# ---- b. the stream's last wave ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(cs.CASES) if n.startswith(("last-wave-", "one-lane-"))])
def test_b_header_in_the_last_partial_wave(torch_mod, codec, oracle, name):
    check(torch_mod, codec, oracle, name)


@pytest.mark.parametrize("name", [n for n in sorted(cs.CASES) if n.startswith(("cut-", "garbage-"))])
def test_b_length_cuts_and_trailing_garbage(torch_mod, codec, oracle, name):
    check(torch_mod, codec, oracle, name)


# ---- c. candidates per workgroup and their order ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["per-workgroup", "order-in-workgroup"])
def test_c_candidates_per_workgroup(torch_mod, codec, oracle, name):
    check(torch_mod, codec, oracle, name)


# ---- d. the walk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["long-jump-0", "long-jump-8190", "not-at-zero", "chain-ends-bad", "chain-ends-notfound"])
def test_d_walk(torch_mod, codec, oracle, name):
    a, b = check(torch_mod, codec, oracle, name)
    assert a[4] > 0 and b[4] > 0, (name, a, b)               # none of these chains is the plain one


# ---- e. capacity and scan groups --------------------------------------------------------------------------------------
def test_e_capacity(torch_mod, oracle):
    """A context's first raw stream finds no candidate arrays: discover_chain waits for the count, makes room and goes on IN
    THE SAME pass of its loop (host/stream.hpp), so the read-out says one pass, as it does for the same stream again.  A
    stream with more candidates than the arrays then hold takes the second pass.  Results are the model's every time."""
    from libhuffman_amd.codec import GpuCodec
    fresh = GpuCodec(0)
    try:
        few, many = cs.get(oracle, "few"), cs.get(oracle, "long-jump-0")
        assert len(many.cands) > 2 * len(few.cands) + 64             # (the arrays grow by an eighth and sixteen)
        d = on_device(torch_mod, few.stream, few.avail)
        for turn in range(2):
            c = check_index(torch_mod, fresh, oracle, "few", few.stream, few.avail, few.length, d)
            assert c[7] == 1 and c[2] == c[1] == len(few.cands), (turn, c)
        a, b = check(torch_mod, fresh, oracle, "long-jump-0")
        assert a[7] == 2 and a[2] == a[1] == len(many.cands), a
        assert b[7] == 1, b                                         # (the arrays have room by now)
        c = check_decode(torch_mod, fresh, oracle, "few", few.stream, few.avail, few.length, d, encoder_only=True)
        assert c[7] == 1, c
    finally:
        fresh.close()


def test_e_no_candidate_at_all(torch_mod, codec):
    """bytes without a zero among them hold no candidate: a context's first call returns from the count, a later one goes
    through the walk; the read-out is the same"""
    from libhuffman_amd.codec import GpuCodec
    n = cm.PARALLEL_MIN + 4096
    st = (1 + np.arange(n) % 255).astype(np.uint8)
    d = on_device(torch_mod, st, n)
    fresh = GpuCodec(0)
    try:
        for c in (fresh, fresh, codec):
            assert block_index(torch_mod, c, d, n, n) == (0, 0, 0, [])
            assert c.stream_counters() == (1, 0, 0, 0, 0, 0, NONE, 1)
    finally:
        fresh.close()


def test_e_two_scan_groups(torch_mod, codec, oracle):
    check(torch_mod, codec, oracle, "two-scan-groups")


# ---- f. thresholds ----------------------------------------------------------------------------------------------------
def test_f_block_index_threshold(torch_mod, codec, oracle):
    case = cs.get(oracle, "thresholds")
    d = on_device(torch_mod, case.stream, case.avail)
    rc, n, used, got = block_index(torch_mod, codec, d, case.avail, cm.INDEX_MIN - 1)
    assert (rc, n, used, got) == (0, 0, 0, []) and codec.stream_counters() == (0,) * 8
    c = check_index(torch_mod, codec, oracle, "thresholds", case.stream, case.avail, cm.INDEX_MIN, d)
    assert c[5] >= 2, c
    rc, n, used, got = block_index(torch_mod, codec, d, case.avail, cm.INDEX_MIN - 1)       # ... and zeros again behind a call that ran
    assert (rc, n, used, got) == (0, 0, 0, []) and codec.stream_counters() == (0,) * 8


@pytest.mark.parametrize("lead", [0, 1])
def test_f_decode_stream_threshold(torch_mod, codec, oracle, lead):
    """at PARALLEL_MIN - 1 and PARALLEL_MIN, on a 16-byte aligned stream and on one that is not (it never discovers)"""
    case = cs.get(oracle, "thresholds")
    d = on_device(torch_mod, case.stream, case.avail, lead)
    assert d.data_ptr() % 16 == lead
    for length in (cm.PARALLEL_MIN - 1, cm.PARALLEL_MIN):
        c = check_decode(torch_mod, codec, oracle, "thresholds", case.stream, case.avail, length, d,
                         discovers=lead == 0 and length >= cm.PARALLEL_MIN, encoder_only=True)
        assert (c is not None) == (lead == 0 and length == cm.PARALLEL_MIN)

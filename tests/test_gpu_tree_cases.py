"""Every case of tests/tree_cases.py - histograms on the branches of tree_fast_wave (kernels/tree.hpp) - through every
encode route that builds a tree: the stream and the block index are the oracle's byte for byte, and the indexed decode
gives the data back.  A tie broken the wrong way still round-trips through our own decoder, so a difference is reported as
what it is: the first differing entry of the serialised tree.  Then the debug build's counters (-DTREE_DEBUG) say that the
kernel took, block by block, the path the model of tests/tree_rounds_ref.py takes through its source."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tree_cases
import tree_rounds_ref as M
from tree_cases import FUSED_BELOW, fused_bs, lanes_bs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def table():
    return [(c, c.data()) for c in tree_cases.cases()]


@pytest.fixture(scope="module")
def reference(oracle):
    """the oracle's (stream, offsets) of a case as one block, computed once per (case, blocksize)"""
    cache = {}

    def get(case, data, bs):
        if (case.name, bs) not in cache:
            cache[case.name, bs] = oracle.encode(data, bs, with_offsets=True)
        return cache[case.name, bs]
    return get


def block_tree(block: np.ndarray):
    """(tree_len, entries) from a block's header"""
    tl = int(np.frombuffer(block[8:10].tobytes(), dtype="<i2")[0])
    return tl, np.frombuffer(block[10:10 + 2 * max(tl, 0)].tobytes(), dtype="<i2").tolist()


def explain(name, route, got: np.ndarray, want: np.ndarray) -> str:
    """a mismatch as what it is: both tree lengths and the first differing tree entry in front of the first differing byte"""
    gl, gt = block_tree(got)
    wl, wt = block_tree(want)
    msg = f"{name} on {route}: tree_len {gl} (ours) / {wl} (oracle)"
    d = next((i for i in range(min(len(gt), len(wt))) if gt[i] != wt[i]), None)
    if d is not None:
        msg += f"; first differing tree entry {d}: {gt[d]} (ours) / {wt[d]} (oracle) - a tie broken the other way reads like this"
    m = min(got.size, want.size)
    b = np.flatnonzero(got[:m] != want[:m])
    msg += f"; first differing byte {int(b[0]) if b.size else m} of {got.size} / {want.size}"
    return msg


def check_stream(name, route, got, got_offs, want, want_offs):
    if not (got.size == want.size and np.array_equal(got, want)):
        pytest.fail(explain(name, route, got, want))
    assert np.array_equal(np.asarray(got_offs, dtype=np.uint64), np.asarray(want_offs, dtype=np.uint64)), (name, route, "block index")


def encode_one(torch, codec, reference, case, data, bs, route):
    d = torch.from_numpy(data).cuda()
    stream, offs, length = codec.encode(d, bs)
    want, want_offs = reference(case, data, bs)
    check_stream(case.name, route, stream.cpu().numpy(), offs.cpu().numpy(), want, want_offs)
    out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    assert codec.decode(stream, length, offs, 1, out, relaxed=True) == data.size, (case.name, route)
    assert torch.equal(out, d), (case.name, route, "round trip")


ROUTES = {
    # route: (cases it holds, blocksize of a case)
    "fused hist_tree_kernel": (lambda c: not c.large and fused_bs(c.n) < FUSED_BELOW, lambda c: fused_bs(c.n)),
    "hist_lanes_kernel + tree_wave_kernel": (lambda c: not c.large, lambda c: lanes_bs(c.n)),
    "chunk counts + block_hist32_kernel + tree_wave_kernel": (lambda c: not c.large, lambda c: 1 << 21),
    "tree_kernel<uint64_t, uint64_t>": (lambda c: True, lambda c: 1 << 22),
    "blocksize 0 (the large cases)": (lambda c: c.large, lambda c: 0),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_case_is_the_oracles_stream(torch_mod, codec, reference, table, route):
    holds, bs_of = ROUTES[route]
    ran = 0
    for case, data in table:
        if holds(case):
            encode_one(torch_mod, codec, reference, case, data, bs_of(case), route)
            ran += 1
    assert ran >= (6 if "large" in route else 50), ran


@pytest.mark.parametrize("below", [FUSED_BELOW, tree_cases.LARGE_FROM])
def test_every_case_as_an_item_of_one_batch(torch_mod, codec, reference, table, below):
    """blocksize 0: an item is one block and the longest item picks the kernels - hist_tree_batch_kernel below 32 KiB,
    the batch's lane-private counts and tree_wave_kernel from there on"""
    torch = torch_mod
    items = [(c, d) for c, d in table if c.n < below]
    assert len(items) >= 50 and (below == FUSED_BELOW) == (max(c.n for c, _ in items) < FUSED_BELOW)
    batch = codec.encode_batch(torch.from_numpy(np.concatenate([d for _, d in items])).cuda(), [c.n for c, _ in items], 0)
    st = batch.stream.cpu().numpy()
    offs = batch.offsets.cpu().numpy().astype(np.int64)
    route = "encode_batch, items below %d bytes" % below
    pos = 0
    for i, (case, data) in enumerate(items):
        want, want_offs = reference(case, data, 0)
        got = st[int(offs[i]):int(offs[i + 1])]
        check_stream(case.name, route, got, [0, got.size], want, want_offs)
        assert int(offs[i]) == pos == batch.item_offsets[i], (case.name, route, "block index")
        pos += want.size
    assert batch.stream_len == pos
    out, errs, raws = codec.decode_batch(batch, relaxed=True)
    assert not any(errs) and raws == [c.n for c, _ in items]
    assert np.array_equal(out.cpu().numpy(), np.concatenate([d for _, d in items]))


def update_picks(table, count=12):
    """the cases with the most distinct sets of events (the model's), among those a block of the fused route holds: first
    the ones that add the most events not seen yet, then other sets of their own"""
    cand = [(c, d, frozenset(e for e, v in M.tree(c.hist)[2].items() if v)) for c, d in table if fused_bs(c.n) < FUSED_BELOW]
    picks, seen, sets = [], set(), set()
    while len(picks) < count:
        rest = [x for x in cand if x[2] not in sets]
        if not rest:
            break
        best = max(rest, key=lambda x: (len(x[2] - seen), len(x[2])))
        picks.append(best)
        seen |= best[2]
        sets.add(best[2])
    return picks


def test_a_case_written_over_a_block_of_a_stream(torch_mod, codec, oracle, table):
    """update_ranges (the row kernels of update.hpp): the last block of a small stream of ordinary blocks replaced by a
    case's bytes is what encoding the new data from scratch gives"""
    from libhuffman_amd import datagen
    torch = torch_mod
    picks = update_picks(table)
    assert len(picks) == 12 and len({s for _, _, s in picks}) == 12
    for case, data, _ in picks:
        n, bs = case.n, fused_bs(case.n)
        old = np.concatenate([datagen.zipf255(2 * bs, seed=5), datagen.uniform256(n, seed=6)])
        stream, offs, length = codec.encode(torch.from_numpy(old).cuda(), bs)
        st, ln, new_offs, _, count = codec.update_ranges(stream, length, offs, 3, [(2 * bs, 2 * bs + n)],
                                                         torch.from_numpy(data).cuda(), blocksize=bs, relaxed=True)
        assert count == 1, case.name
        new = np.concatenate([old[:2 * bs], data])
        want, want_offs = oracle.encode(new, bs, with_offsets=True)
        got = st.cpu().numpy()
        b = int(want_offs[2])
        if not (got.size == want.size and np.array_equal(got, want)):
            assert np.array_equal(got[:b], want[:b]), (case.name, "the blocks in front")
            pytest.fail(explain(case.name, "update_ranges", got[b:], want[b:]))
        assert np.array_equal(new_offs.cpu().numpy().astype(np.uint64), want_offs), (case.name, "block index")
        out = torch.empty(new.size, dtype=torch.uint8, device="cuda")
        assert codec.decode(st, ln, new_offs, 3, out, relaxed=True) == new.size, case.name
        assert np.array_equal(out.cpu().numpy(), new), case.name


def test_the_kernel_takes_the_models_path_in_the_debug_build(torch_mod):
    """tests/tree_cases_debug_child.py under the -DTREE_DEBUG build: per case and route the stream is the oracle's and the
    counters are the model's event counts exactly; over the table every reachable event is reached, the others never"""
    from test_gpu_pack_builds import build_variant
    lib = build_variant("tree_debug", "-DTREE_DEBUG")
    env = dict(os.environ, HUF_LIB_PATH=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tree_cases_debug_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    cases = tree_cases.cases()
    assert [x["case"] for x in rows] == [c.name for c in cases], r.stdout[-3000:]
    print("\n".join(json.dumps(x) for x in rows))
    total = dict.fromkeys(M.EVENTS, 0)
    wrong = []
    for row, c in zip(rows, cases):
        assert row["equal"], row
        want = M.tree(c.hist)[2]
        assert "tree_wave" in row["counters"] and ("fused" in row["counters"]) == (fused_bs(c.n) < FUSED_BELOW), row
        for route, cnt in row["counters"].items():
            got = dict(zip(M.EVENTS, cnt))
            assert len(cnt) == len(M.EVENTS)
            if got != want:
                wrong.append((c.name, route, {e: (got[e], want[e]) for e in M.EVENTS if got[e] != want[e]}))
            for e, v in got.items():
                total[e] += v
    assert not wrong, "counters (kernel, model): " + "\n".join(map(str, wrong))
    assert all(total[e] == 0 for e in M.NEVER), {e: total[e] for e in M.NEVER}
    missing = [e for e in M.EVENTS if e not in M.NEVER and total[e] == 0]
    assert not missing, missing

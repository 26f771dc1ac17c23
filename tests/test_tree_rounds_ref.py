"""The model of the round-wise tree build (tests/tree_rounds_ref.py) checked on the CPU: on every case of
tests/tree_cases.py and on 1 500 random histograms its tree and code lengths are the oracle's, over the table every event
the debug build counts occurs, and the events that must never occur do not."""
import numpy as np
import pytest

import tree_cases
import tree_rounds_ref as M


@pytest.fixture(scope="module")
def walked(oracle):
    """every case with the model's walk and the oracle's tree"""
    out = []
    for c in tree_cases.cases():
        trace = []
        tb, lens, ev, codes = M.tree(c.hist, trace)
        out.append((c, tb, lens, ev, codes, trace, M.oracle_tree(oracle, c.data())))
    return out


def test_model_is_the_oracle_on_every_case(walked):
    for c, tb, lens, ev, codes, trace, want in walked:
        assert len(tb) == len(want), (c.name, len(tb), len(want))
        diff = [i for i in range(len(tb)) if tb[i] != want[i]]
        assert not diff, (c.name, "first differing tree entry", diff[0], tb[diff[0]], want[diff[0]])
        wl, wc = M.tree_lengths_and_codes(want)
        assert lens == wl, c.name
        assert codes == {s: wc[s] & M.MASK32 for s in wc}, c.name       # the path doubling's 32 code bits are the tree's
        assert max(wl.values()) <= 32, c.name


def test_cases_are_what_they_are_named_for(walked):
    by = {c.name: (c, tb, lens, ev, trace) for c, tb, lens, ev, codes, trace, want in walked}
    names = list(by)
    assert len(names) == len(set(names))
    for count in (1, 1000):
        for k in tree_cases.EQUAL_K:
            for side in ("low", "high"):
                c = by[f"equal_{k}x{count}_{side}"][0]
                assert np.count_nonzero(c.hist) == k and c.n == k * count
                assert (c.hist[:k] if side == "low" else c.hist[256 - k:]).all()
    # sel below, at and above round_min on every register count: the first decision of the walk
    seen = set()
    for c, tb, lens, ev, trace in by.values():
        if c.first:
            R, sel, round_min = c.first
            assert trace[0] == (R, sel, round_min, "round" if sel >= round_min else "single"), (c.name, trace[0])
            seen.add((R, sel - round_min))
    assert seen == {(R, d) for R in (1, 2, 4) for d in (-1, 0, 1)}
    # a sorted round with sel exactly 16 behind seven single merges on four registers
    assert by["ties_ramp"][4][:8] == [(4, s, 16, "single") for s in (2, 4, 6, 8, 10, 12, 14)] + [(4, 16, 16, "round")]
    ev = by["pairs65_stays_R4"][3]
    assert ev["nodes_sorted2_r4"] == 1 and ev["check_pass_r4"] >= 1 and ev["round_in_order_r4"] >= 1
    assert by["R4_to_R1"][3]["r_4_1"] == 1
    assert by["one_value"][3]["one_symbol"] == 1 and by["one_value"][1] == [256, 7, -1, -1, -1]
    assert len(by["all_256_one_dominant"][1]) == 1025
    for k in (29, 30, 31):
        c, tb, lens, ev, trace = by[f"depth_fib{k}"]
        assert c.n == {29: 1346268, 30: 2178308, 31: 3524577}[k] and max(lens.values()) == k
    c, tb, lens, ev, trace = by["depth_fib31_4194303"]
    assert c.n == 4194303 and max(lens.values()) == 31
    c, tb, lens, ev, trace = by["depth_fib31_spread"]
    deepest = [s for s, ln in lens.items() if ln == 31]
    assert sorted(deepest) == [5, 232]                             # lanes 5 and 40, registers 0 and 3
    assert by["two_values_1_4194302"][0].n == 4194303
    # small blocks: only the depth cases and the largest key are large
    for c, *_ in by.values():
        assert c.large == (c.name.startswith("depth_") or c.name == "two_values_1_4194302"), c.name
        assert c.large or c.n <= 262144, c.name


def test_every_event_is_reached_and_the_forbidden_ones_never(walked):
    total = dict.fromkeys(M.EVENTS, 0)
    for c, tb, lens, ev, *_ in walked:
        assert set(ev) == set(M.EVENTS)
        for e, v in ev.items():
            total[e] += v
        general = ev["blocks_r1"] + ev["blocks_r2"] + ev["blocks_r4"]
        assert general + ev["one_symbol"] == 1, c.name
        assert ev["wrap_root"] == general == sum(ev["path_rounds_%d" % i] for i in range(1, 7)), c.name
    for e in M.NEVER:
        assert total[e] == 0, (e, [c.name for c, _, _, ev, *_ in walked if ev[e]])
    missing = [e for e in M.EVENTS if e not in M.NEVER and total[e] == 0]
    assert not missing, missing


def test_the_reported_order_failures_at_one_register(walked):
    """what a rough walk of the control flow said while the table was planned: k bytes once each, k = 5, 65, 66, 129, 130,
    fail the order check at one register, so the round behind it sorts again; k = 129 sorts its nodes in one register,
    k = 130 in two; 1 << (i % 6) sorts its nodes in one register five times"""
    by = {c.name: ev for c, _, _, ev, *_ in walked}
    for k in (5, 65, 66, 129, 130):
        for side in ("low", "high"):
            assert by[f"equal_{k}x1_{side}"]["check_fail_r1"] >= 1, k
    assert by["equal_129x1_low"]["nodes_sorted1_r2"] == 1 and by["equal_130x1_low"]["nodes_sorted2_r2"] == 1
    assert by["ties_pow2_mod6"]["nodes_sorted1_r2"] + by["ties_pow2_mod6"]["nodes_sorted1_r4"] == 5


def test_model_is_the_oracle_on_random_histograms(oracle):
    """six kinds of counts over random byte values, 1 500 trials (what tests/stress/tree_rounds_model.py ran)"""
    rng = np.random.default_rng(1)
    total = dict.fromkeys(M.EVENTS, 0)
    for trial in range(1500):
        k = int(rng.integers(1, 257))
        syms = rng.choice(256, size=k, replace=False)
        mode = trial % 6
        if mode == 0:
            w = np.ones(k, dtype=np.int64)
        elif mode == 1:
            w = rng.integers(1, 4, size=k)
        elif mode == 2:
            w = rng.integers(1, 200, size=k)
        elif mode == 3:
            w = 2 ** rng.integers(0, 6, size=k)
        elif mode == 4:
            w = np.array([1] * (k // 2) + [2] * (k - k // 2))
        else:
            f = [1, 1]
            while len(f) < k and f[-1] < 3000:
                f.append(f[-1] + f[-2])
            w = np.array((f + [1] * k)[:k])
        data = np.repeat(syms.astype(np.uint8), w)
        rng.shuffle(data)
        tb, lens, ev, codes = M.tree(np.bincount(data, minlength=256))
        want = M.oracle_tree(oracle, data)
        assert tb == want, (trial, k, mode, tb[:12], want[:12])
        assert lens == M.tree_lengths_and_codes(want)[0], (trial, k, mode)
        for e, v in ev.items():
            total[e] += v
    for e in M.NEVER:
        assert total[e] == 0, e

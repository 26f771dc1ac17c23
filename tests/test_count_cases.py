"""tests/count_cases.py on the CPU: the census of every counting body gives np.bincount on every block of the table; every
event of a body is reached and every case reaches what it claims; the histograms are the ones whose tree shows a miscount
(the share not seen is at most 1/10 and 0 on the symbols a case is about); every mutant of the census changes the tree of a
block aimed at its branch; profiles/count_cases/sensitivity.txt is what the table gives today."""
import os

import numpy as np
import pytest

import count_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    return [(c, c.data()) for c in cc.cases()]


def body_blocks(case, data, body):
    """[(bytes, address modulo 16)] `body` counts when the case is encoded: chunks on the chunked route"""
    if case.group == "chunked" and body == "hl_count":
        return cc.chunk_blocks(case, data)
    return [(blk, addr) for blk, addr, _, _ in case.block_list(data)]


@pytest.fixture(scope="module")
def walked(table):
    """{(case name, body): [(counts, events)] per block}, no mutant"""
    return {(c.name, body): [cc.census(body, blk, addr) for blk, addr in body_blocks(c, d, body)]
            for c, d in table for body in c.bodies}


@pytest.fixture(scope="module")
def unseen_of(oracle):
    """{symbol: [deltas not seen]} per histogram, computed once; the block of 4 MiB + 1 through the oracle"""
    cache = {}

    def get(name, hist):
        if name not in cache:
            cache[name] = cc.unseen(hist) if hist.sum() + 16 < cc.TREE_MAX_TOTAL else cc.unseen_oracle(oracle, hist)
        return cache[name]
    return get


def test_the_table_has_the_shapes_the_routes_need(table):
    by = {c.name: c for c, _ in table}
    assert len(by) == len(table) >= 30
    for c, d in table:
        assert d.size == c.n and d.dtype == np.uint8
        for blk, addr, hist, _ in c.block_list(d):
            assert np.array_equal(np.bincount(blk, minlength=256), hist), c.name
    fused = [c for c, _ in table if c.group == "fused"]
    assert {c.bs for c in fused} == {4097, 13009, 32767} and all(c.blocks == 17 and c.last == 21 for c in fused)
    for c in fused:                                             # block starts take all 16 alignments
        assert {(c.offset + b * c.bs) & 15 for b in range(17)} == set(range(16))
    lanes = [c for c, _ in table if c.group == "lanes"]
    assert {c.bs for c in lanes} == {32769, 60001, 65537} and all(c.blocks == 17 and c.last == 21 for c in lanes)
    assert sorted(c.args["lane"] >= 32 for c, _ in table if c.group == "lanes_big") == [False, True]
    assert by["c2097153_flat_shuffled"].n == 2 * 2097153 + 3 * 262144 + 21 and by["c4194305_skewed_shuffled"].n == 4194305 + 21
    assert {c.bs for c, _ in table if c.group == "env"} == {65537, 131072, 131073, 200001}
    # 13 009 and 60 001 lie in the windows: a wave splits
    assert 769 <= cc.geometry(13009, 0)[1] <= 1023 and 3585 <= cc.geometry(60001, 0)[1] <= 4095


def test_the_census_counts_are_bincount(table, walked):
    for c, d in table:
        for body in c.bodies:
            for (blk, addr), (counts, ev) in zip(body_blocks(c, d, body), walked[c.name, body]):
                assert np.array_equal(counts, np.bincount(blk, minlength=256)), (c.name, body, addr)
                assert set(ev) == set(cc.BODY_EVENTS[body])


def test_every_event_is_reached_and_every_claim_holds(table, walked):
    total = {body: dict.fromkeys(cc.BODY_EVENTS[body], 0) for body in cc.BODIES}
    for c, d in table:
        assert set(c.claims) <= set(c.bodies), c.name
        for body in c.bodies:
            evs = dict.fromkeys(cc.BODY_EVENTS[body], 0)
            for _, ev in walked[c.name, body]:
                for e, v in ev.items():
                    evs[e] = max(evs[e], v) if e == "max16" else evs[e] + v
            for e in c.claims.get(body, ()):
                assert evs[e] >= (cc.MAX16_AT_LEAST if e == "max16" else 1), (c.name, body, e, evs)
            for e, v in evs.items():
                total[body][e] = max(total[body][e], v) if e == "max16" else total[body][e] + v
    for body in cc.BODIES:
        missing = [e for e, v in total[body].items() if v < (cc.MAX16_AT_LEAST if e == "max16" else 1)]
        assert not missing, (body, missing, total[body])
    # the bounds: a lane's counter of hl_count and one fold target of the packed body hold half of what 16 bits can
    assert 32768 <= total["hl_count"]["max16"] < 32768 + 32 and 32768 <= total["fused_packed"]["max16"] < 32768 + 32


def test_the_tree_shows_a_miscount(table, unseen_of):
    seen_names = set()
    for c, d in table:
        kinds = {}
        for blk, addr, hist, blind in c.block_list(d):
            full = blk.size == c.bs
            own = c.own_symbols(blk, addr)
            assert not own & set(blind), (c.name, addr, "a symbol the case is about is one the tree does not show", own & set(blind))
            kinds.setdefault(full, [hist, blind, set()])[2].update(own)
        for full, (hist, blind, own) in kinds.items():
            name = c.hname if full else "last%d" % c.last
            miss = unseen_of(name, hist)
            assert tuple(sorted(miss)) == tuple(blind), (c.name, name, miss)
            u, t = cc.share(hist, miss)
            assert u * 10 <= t, (c.name, name, u, t)
            assert len(miss) * 10 <= int((hist > 0).sum()), (c.name, name, "by symbols", miss)
            seen_names.add(name)
    assert set(cc.BLIND) <= seen_names


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_a_mutant_changes_the_tree_of_a_block_aimed_at_it(table, mutant):
    caught = []
    for c, d in table:
        for body in c.bodies:
            if body not in cc.MUTANT_BODIES[mutant]:
                continue
            for blk, addr in body_blocks(c, d, body):
                counts, _ = cc.census(body, blk, addr, mutant=mutant)
                true = np.bincount(blk, minlength=256)
                if mutant in cc.EQUIVALENT:
                    assert np.array_equal(counts, true), (c.name, body)
                    continue
                if np.array_equal(counts, true) or true.sum() + 16 >= cc.TREE_MAX_TOTAL or counts.sum() == 0:
                    continue
                if cc.tree_of(counts) != cc.tree_of(true):
                    caught.append((c.name, body, addr))
                    break
    if mutant in cc.EQUIVALENT:
        # the branch is walked (folds whose first active lane is odd), and the mistake cannot reach a count
        assert any(ev.get("fold_first_odd") for c, d in table if "fused_packed" in c.bodies
                   for blk, addr in body_blocks(c, d, "fused_packed") for ev in [cc.census("fused_packed", blk, addr)[1]])
        return
    print(mutant, "caught by", len(caught), "case / body pairs, first:", caught[:3])
    assert caught, mutant + ": the table is missing a case"
    assert {b for _, b, _ in caught} == {b for b in cc.MUTANT_BODIES[mutant] if any(b in c.bodies for c, _ in table)}, caught


def test_the_recorded_sensitivities_are_todays(unseen_of):
    path = os.path.join(ROOT, "profiles", "count_cases", "sensitivity.txt")
    with open(path) as f:
        text = f.read()
    want = cc.report_cases(unseen_of)
    assert text.startswith(want), "run `python tests/count_cases.py > profiles/count_cases/sensitivity.txt`"
    assert "# existing inputs" in text[len(want):]

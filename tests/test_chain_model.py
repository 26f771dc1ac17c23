"""tests/chain_model.py - the CPU restatement of the raw-stream block discovery - held to what the builders of
tests/chain_streams.py know by construction: where the blocks lie, which offsets are candidates, how far the chain goes.
And the oracle's decoder agrees with the construction on bytes and consumed count wherever the chain ends the stream.
No GPU."""
import numpy as np
import pytest

import chain_model as cm
import chain_streams as cs


def test_geometry_is_read_from_the_sources():
    assert (cm.PIECE, cm.WAVE, cm.ROW, cm.WORKGROUP) == (cm.DISC_PER, 64 * cm.DISC_PER, cm.DISC_THREADS * cm.DISC_PER,
                                                          cm.DISC_THREADS * cm.DISC_PER * cm.DISC_ITERS)
    assert cm.INDEX_MIN < cm.PARALLEL_MIN and cm.WALK_CHUNK > 0 and cm.DISC_SLOTS >= 1 and cm.DISC_SCAN_GROUP >= 2
    assert cm.WAVE < cm.ROW < cm.WORKGROUP                  # the sweeps take an edge of the next larger kind for that kind's case


def test_strict_header_field_by_field():
    good = np.frombuffer(cs.hm._handmade_block(b"\x11" * 8, 2), dtype=np.uint8)
    n = good.size
    assert cm.strict_header(good, 0, n, 1025) and cm.grammar_complete(np.array([0x101, 65, -1, -1, 66, -1, -1], np.int16))

    def changed(at, values):
        bad = good.copy()
        bad[at:at + len(values)] = values
        return bad
    assert not cm.strict_header(good, 0, 9, 1025)                               # fewer than ten bytes left
    assert not cm.strict_header(changed(0, [0]), 0, n, 1025)                    # block_len 0
    assert not cm.strict_header(changed(4, [1]), 0, n, 1025)                    # block_len 2^32 + 64
    assert not cm.strict_header(changed(8, [0]), 0, n, 1025)                    # tree_len 0
    assert not cm.strict_header(changed(8, [0xff, 0xff]), 0, n, 1025)           # tree_len -1
    assert not cm.strict_header(good, 0, n, 6) and cm.strict_header(good, 0, n, 7)      # tree_len against max_tree
    assert not cm.strict_header(good, 0, 23, 1025)                              # the header ends behind avail
    assert cm.strict_header(good, 0, 32, 1025) and not cm.strict_header(good, 0, 31, 1025)      # a bit a symbol: 64 symbols, 8 bytes
    assert not cm.strict_header(changed(8, [6]), 0, n, 1025)                    # the tree is not complete with six entries
    assert not cm.strict_header(changed(8, [8]), 0, n, 1025)                    # an entry behind the complete tree
    assert not cm.strict_header(changed(12, [0xff, 0xff]), 0, n, 1025)          # complete after three entries, four behind it


def test_two_headers_in_one_piece():
    """exactly the offsets +0 and +6 of the 24 bytes pass, given the stream behind them that the second one claims"""
    rng = np.random.default_rng(1)
    buf = rng.integers(1, 256, 4096 + cs.TWO_NEEDS, dtype=np.uint8)
    buf[4096:4096 + len(cs.TWO)] = np.frombuffer(cs.TWO, np.uint8)
    assert cm.candidates(buf, buf.size, buf.size, 1025) == [4096, 4102]
    assert cm.candidates(buf, buf.size - 1, buf.size, 1025) == [4096]
    assert cm.candidates(buf, buf.size, 4102, 1025) == [4096]                   # scan_len is exclusive


def test_sweeps_cover_every_position(oracle):
    for edge_name, edge in cs.EDGES.items():
        for kind in ("tree7", "tree67", "planted"):
            case = cs.get(oracle, f"sweep-{edge_name}-{kind}")
            near = sorted((c + 24) % edge - 24 for c in case.cands if -24 <= (c + 24) % edge - 24 < 16 and c >= edge - 24)
            assert set(cs.DELTAS) <= set(near), (case.name, sorted(set(cs.DELTAS) - set(near)))
            assert case.stream.size < 1 << 20, case.name


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_model_equals_construction(oracle, name):
    case = cs.get(oracle, name)
    st = case.stream
    assert st.size >= cm.PARALLEL_MIN and case.avail == st.size
    scan_len = min(case.length, case.avail)
    got = cm.candidates(st, case.avail, scan_len, cs.MAX_TREE)
    assert got == case.cands, (name, len(got), len(case.cands), sorted(set(got) ^ set(case.cands))[:8])
    index, nblocks, consumed, complete = cm.chain(oracle, st, case.avail, case.length, cs.MAX_TREE)
    want = case.index + [case.consumed] if case.index else []
    assert (nblocks, consumed, complete) == (len(case.index), case.consumed, case.complete), name
    assert index == want, (name, [(a, b) for a, b in zip(index, want) if a != b][:4])
    sizes = [int.from_bytes(st[p:p + 8].tobytes(), "little") for p in case.index]
    assert case.data.size == sum(sizes), name
    err, out, used = oracle.decode(st, 8 * st.size + 64, cs.MAX_TREE, length=case.length)
    assert np.array_equal(out[:case.data.size], case.data), (name, "the bytes of the chain's blocks")
    if case.complete:
        assert (err, out.size, used) == (0, case.data.size, case.consumed), name


def test_cases_reach_what_they_are_named_for(oracle):
    g = lambda name: cs.get(oracle, name)                                       # noqa: E731
    per_wg = np.bincount(np.array(g("per-workgroup").cands) // cm.WORKGROUP, minlength=15)[:15].tolist()
    s = cm.DISC_SLOTS
    assert per_wg == [1, 0, s, s + 1, s, 300, s, 0, s + 1, 1, s + 1, s + 1, 0, 300, 1]
    for lanes in (2, 33, 63):
        case = g(f"last-wave-{lanes}-2-row0")
        assert -(-(case.length % cm.WAVE) // cm.PIECE) == lanes and case.length % cm.WORKGROUP < cm.ROW
        assert case.index[-1] >= case.length - case.length % cm.WAVE           # the last header lies in the partial wave
    assert g("last-wave-63-100-row2").length % cm.WORKGROUP >= 2 * cm.ROW
    for where in ("edge", "header", "payload"):
        case = g(f"cut-{where}")
        p = case.index[-1] if where != "edge" else case.consumed            # the block that `length` touches
        header_end = p + cm.HEADER_FIXED + 2 * int.from_bytes(case.stream[p + 8:p + 10].tobytes(), "little")
        lo, hi = {"edge": (p, p + 1), "header": (p + 1, header_end), "payload": (header_end, case.consumed)}[where]
        assert lo <= case.length < hi, (where, case.length, p, header_end, case.consumed)
    one = g("one-lane-100")
    assert one.length % cm.WAVE == 1 and one.cands[-1] == one.length - 1 and one.consumed > one.length
    for small in (0, cm.WALK_CHUNK - 2):
        case = g(f"long-jump-{small}")
        assert case.index[small + 1] - case.index[small] > 12 * cm.WALK_CHUNK
        assert case.cands.index(case.index[small + 1]) // cm.WALK_CHUNK == case.cands.index(case.index[small]) // cm.WALK_CHUNK + (2 if small else 1)
    for how in ("bad", "notfound"):
        case = g(f"chain-ends-{how}")
        assert len(case.index) > cm.WALK_CHUNK and not case.complete and not case.plain
    two = g("two-scan-groups")
    wg = np.array(two.cands) // cm.WORKGROUP
    counts = [int(np.count_nonzero(wg == cm.DISC_SCAN_GROUP + i)) for i in (-2, -1, 0, 1)]
    assert counts == [s, s + 3, s + 1, 2] and two.stream.size > cm.SCAN_GROUP and two.stream.size < 17 << 20
    assert g("sweep-wave-tree7").plain and g("cut-payload").plain and g("sweep-wave-planted").false_below
    assert not g("not-at-zero").index and g("not-at-zero").cands[0] == len(cs.EMPTY)

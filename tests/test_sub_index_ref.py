"""The sub-index reference (tests/sub_index_ref.py) checked on the CPU: its layout is the library's, its entries add up on
the oracle's streams, and every case of test_gpu_sub_index_content.py keeps to the path, classes and blocks it claims."""
import dataclasses

import numpy as np
import pytest

import sub_index_ref as R
from libhuffman_amd import _native as N


@pytest.fixture(scope="module")
def L():
    from libhuffman_amd import build
    build.build()
    return N.load()


@pytest.fixture(scope="module")
def encoded(oracle):
    """every case of the table with the oracle's stream, block offsets and the expected sub-index"""
    out = []
    for c in R.cases():
        data = c.data()
        st, offs = oracle.encode(data, c.blocksize, with_offsets=True)
        out.append((c, data, st, offs, R.expected(st, offs, data, c.blocksize)))
    return out


@pytest.mark.parametrize("n,bs", [
    (1, 0), (1, 1), (1, 5000), (100, 1000), (4097, 0), (5000, 1), (5000, 31), (5000, 32), (5000, 33),
    (100000, 2047), (100000, 2048), (100000, 2049), (5 << 20, (2 << 20) - 1), (5 << 20, (2 << 20) + 1),
    ((9 << 20) + 77, (4 << 20) + 5), ((9 << 20) + 77, 0), (3, (4 << 20) + 5), (0, 0), (0, 64),
])
def test_layout_is_the_librarys(L, n, bs):
    lay = R.layout(n, bs)
    assert lay.size == L.hufgpu_sub_index_bytes(n, bs)
    if n:
        assert lay.nb == L.hufgpu_block_count(n, bs or n)
        assert lay.gpb % 8 == 0 and (lay.lens_off - lay.group_off) % 16 == 0 and lay.lens_off % 8 == 0
        assert lay.group_off == lay.nb * lay.tpb * 8


def test_reference_adds_up_on_oracle_streams(encoded):
    for c, data, st, offs, exp in encoded:
        lay = exp.lay
        for b, f in enumerate(exp.facts):
            tag = (c.name, b)
            s0, ln = exp.block_syms[b]
            ng, nt = -(-ln // R.GROUP), -(-ln // R.TILE)
            g = exp.groups[b * lay.gpb:(b + 1) * lay.gpb].astype(np.int64)
            t = exp.tiles[b * lay.tpb:(b + 1) * lay.tpb].astype(np.int64)
            lens = exp.lens[b * R.NSYM:(b + 1) * R.NSYM]
            # the groups hold the payload, less the pad bits of its last byte
            assert 0 <= f["pay_bits"] - g.sum() < 8, tag
            # a tile starts behind the groups in front of it
            cg = np.concatenate([[0], np.cumsum(g)])
            assert np.array_equal(t[:nt], cg[np.arange(nt) * (R.TILE // R.GROUP)]), tag
            assert not g[ng:].any() and not t[nt:].any(), tag
            # lens: exactly the values that occur, a complete tree under the wrapped root (Kraft, with L - 1)
            present = np.bincount(data[s0:s0 + ln], minlength=R.NSYM) > 0
            assert np.array_equal(lens > 0, present), tag
            if f["K"] >= 2:
                top = int(lens.max())
                assert sum(1 << (top - int(x) + 1) for x in lens[lens > 0]) == 1 << top, tag
            # the written set: nothing of a one-symbol block, never the padding
            written = f["tree_len"] != 5
            assert exp.w_groups[b * lay.gpb:(b + 1) * lay.gpb].sum() == (ng if written else 0), tag
            assert exp.w_tiles[b * lay.tpb:(b + 1) * lay.tpb].sum() == (nt if written else 0), tag
            assert exp.w_lens[b * R.NSYM:(b + 1) * R.NSYM].all() == written, tag
            if f["K"] == 2:                                     # two 2-bit codes: every whole group is 64 bits
                assert (g[:ln // R.GROUP] == 2 * R.GROUP).all(), tag


def test_every_case_keeps_to_its_path(encoded):
    for c, data, st, offs, exp in encoded:
        R.check_claims(c, st, offs, data)


def test_claims_are_checked_not_assumed(encoded):
    c, data, st, offs, _ = next(x for x in encoded if x[0].name == "lanes_full_1048576_gt24")
    for wrong in (dataclasses.replace(c, cls="16_24"), dataclasses.replace(c, path="lanes_short"),
                  dataclasses.replace(c, fix=1), dataclasses.replace(c, blocks=[("k2", ln) for _, ln in c.blocks])):
        with pytest.raises(AssertionError):
            R.check_claims(wrong, st, offs, data)


def test_the_matrix_reaches_every_writer_and_edge(encoded):
    writers, by_path = set(), {}
    for c, data, st, offs, exp in encoded:
        writers |= set(R.check_claims(c, st, offs, data))
        p = by_path.setdefault(c.path, {"bs": set(), "kinds": set(), "short": False, "unaligned": set(), "one": False,
                                              "k256": False})
        p["bs"].add(c.blocksize)
        p["kinds"] |= {k for k, _ in c.blocks}
        last = c.blocks[-1][1]
        p["short"] |= len(c.blocks) > 1 and last % R.GROUP != 0 and last % R.TILE != 0
        p["one"] |= last == 1
        p["k256"] |= any(f["K"] == 256 for f in exp.facts)
        if any(o % 16 for o in c.dev_offsets):
            p["unaligned"] |= set(c.dev_offsets)
    assert writers == {"pack_block_multi<3>", "pack_block_multi<2>", "pack_block<uint32_t>", "pack_block<hufcode_t>",
                       "pack_segment<0>", "pack_segment<1>", "pack_segment<2>"}
    want_bs = {"fused": {31, 32, 2047, 2048, 2049, 32767}, "lanes_short": {32768, 65536, 121392},
               "lanes_full": {121393, 1 << 20, (2 << 20) - 1}, "chunked32": {2 << 20, (2 << 20) + 1, (3 << 20) + 2049},
               "chunked64": {4 << 20, (5 << 20) + 3, 0}}
    assert {p: v["bs"] for p, v in by_path.items()} == want_bs
    for path, v in by_path.items():
        assert {"cls", "k1", "k2"} <= v["kinds"] and v["short"], path
        assert v["unaligned"] == {3, 13}, path
        assert v["k256"], path
    assert any(v["one"] for v in by_path.values())
    # every class of every path (where a full block of the path can reach it)
    got = {(c.path, c.cls) for c, *_ in encoded}
    for path, _, classes, _ in R.MATRIX:
        for cls in classes:
            assert (path, cls) in got, (path, cls)
    # codes over 32 bits are the only blocks the decoder hands on; the table has one such block
    assert sum(c.fix for c, *_ in encoded) == 1

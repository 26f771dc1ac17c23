"""The decode-edge case table (tests/decode_edge_cases.py) checked on the CPU: every case decodes, by the oracle, to the
symbols it was built from, and every property it claims for its blocks holds.  And the hand-made block builder
(tests/handmade_streams.py) still writes the bytes the older tests' seeds depend on."""
import hashlib

import numpy as np
import pytest

import decode_edge_cases as dec
import handmade_streams as hm


@pytest.fixture(scope="module")
def table(oracle):
    return dec.cases(oracle)


def test_every_case_decodes_to_its_symbols_and_keeps_its_claims(oracle, table):
    names = [c.name for c in table]
    assert len(set(names)) == len(names)
    for group in "ABCDE":
        assert any(n.startswith(group) for n in names), group
    for group in "BCD":                 # (threshold blocks as streams small enough for hufgpu_decode_small)
        assert any(n.startswith(group) and n.endswith("_alone") for n in names), group
    for c in table:
        st = c.stream
        err, out, used = oracle.decode(st, c.syms.size + 64, 1025)
        assert (err, used) == (0, st.size) and np.array_equal(out, c.syms), c.name
        dec.check_claims(c)
        assert c.flips, c.name
        for label, bad in dec.damaged(c):
            assert np.count_nonzero(bad != st) == 1, label


def test_claims_are_checked_not_assumed(oracle, table):
    """check_claims() fails a case whose claim is false"""
    c = next(x for x in table if x.name == "B_code32_K36")
    wrong = dec.Case(c.name, c.parts, c.syms, [(0, {"max_code": 33})])
    with pytest.raises(AssertionError):
        dec.check_claims(wrong)
    wrong = dec.Case(c.name, c.parts, c.syms, [(0, {"one_length_rel": 4})])
    with pytest.raises(AssertionError):
        dec.check_claims(wrong)


def test_encoder_tree_is_the_encoders_shape():
    rng = np.random.default_rng(3)
    lengths = dec.lengths_chain(3, 33, 256)
    assert len(lengths) == 256 and max(lengths) == 33 and sum(2.0 ** -(L - 1) for L in lengths) == 1.0
    vals = dec.values_for(256, rng)
    blk, syms, info = hm.encoder_block(lengths, vals, rng.integers(0, 256, 500))
    f = dec.block_facts(blk)
    assert f["encoder_shaped"] and f["tree_len"] == 4 * 256 + 1 and f["K"] == 256
    assert all(f["code_len"][v] == L for v, L in zip(vals, lengths))
    assert info["nbits"] == int(info["lens"].sum()) and f["pay_bits"] == 8 * ((info["nbits"] + 7) // 8)
    with pytest.raises(AssertionError):
        hm.encoder_tree([2, 3, 4], [1, 2, 3])                       # not Kraft-complete


def test_padding_with_zeros_ones_and_none():
    """the last byte's free bits are zeros or ones; a payload that ends on a byte boundary has none"""
    for pad_ones, n in ((False, 3), (True, 3), (True, 4)):
        blk, _, info = hm.encoder_block([2, 2], [5, 6], [1] * n, pad_ones=pad_ones)       # codes 01: n * 2 bits
        last = blk[-1]
        if n == 4:
            assert info["nbits"] == 8 and last == 0b01010101
        else:
            assert last == (0b01010111 if pad_ones else 0b01010100)


def test_handmade_block_bytes_are_unchanged():
    """block() with the seeds the older tests use writes the bytes it wrote before its payload writer was vectorised"""
    want = {0: "3f070fd26d83e8f260cb7804256d3ca20cd5272499a3e374be0788b9050f494e",
            1: "9b01b12451e1c2191dd8a3bfcdbe64b4df11a1daef64da1369c8fe8f1273daef",
            9000: "575d317fcbaa68b6faacdaeff008a37175c9b8ff55e63c5ac6e629553ad283dc",
            12000: "459efee45885fc07cd8726ba63c052eae750afc7d94d4e3555a7175fafbfe8f6"}
    for seed, digest in want.items():
        rng = np.random.default_rng(seed)
        h = hashlib.sha256()
        for _ in range(6):
            b, syms, d = hm.block(rng, int(rng.integers(2, 257)), float(rng.choice([0.0, 0.3, 0.8, 0.97])), bool(rng.integers(0, 2)),
                                  int(rng.choice([1, 7, 300, 5000])), deep_often=bool(rng.integers(0, 2)), pad_ones=bool(rng.integers(0, 2)))
            h.update(b)
            h.update(syms.tobytes())
            h.update(str(d).encode())
        assert h.hexdigest() == digest, seed


def test_payload_writer_takes_a_block_of_many_symbols(oracle):
    """2^22 symbols: more than one of the writer's chunks"""
    rng = np.random.default_rng(5)
    lengths = dec.lengths_chain(3, 20)
    pick = rng.integers(0, len(lengths), 1 << 22)
    blk, syms, info = hm.encoder_block(lengths, dec.values_for(len(lengths), rng), pick)
    assert info["nbits"] == int(np.asarray(lengths)[pick].sum())
    f = dec.block_facts(blk)
    assert f["len"] == pick.size and f["pay_bits"] == 8 * ((info["nbits"] + 7) // 8)
    err, out, _ = oracle.decode(blk, pick.size, 1025)
    assert err == 0 and np.array_equal(out, syms)

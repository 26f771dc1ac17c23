"""What the encoder writes into its sub-index (hufgpu_encode_sub), entry by entry, against the CPU reference of
tests/sub_index_ref.py - and that decoding with it hands no block to the exact decoder.

The decoder verifies the sub-index and decodes a block it cannot verify again with the exact decoder, so a wrong entry
costs time and never shows in the output: only a comparison with the expected entries and the decoder's counters see it.
The cases (sub_index_ref.cases(), their claims checked on the CPU by test_sub_index_ref.py) put every blocksize path of
encode_impl and every max_len class of pack_kernel / pack_chunk_kernel to work, with one-symbol, two-symbol, 256-symbol
and short last blocks among ordinary ones.
"""
import numpy as np
import pytest

import sub_index_ref as R

pytestmark = pytest.mark.gpu

GUARD_WORDS = 1024                      # 8 KiB behind the sub-index that no encode may touch
FILL_A = 0x5A5A5A5A5A5A5A5A
FILL_B = -1                             # all ones: what is not written stays garbage for the decoder
OUT_GUARD = 64
OUT_FILL = 0xA5

CASES = [(c, off) for c in R.cases() for off in c.dev_offsets]


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


def encode_into(torch, codec, d, bs, lay, fill):
    """encode_sub into the front of a filled int64 tensor; returns (stream, offsets, length, the sub-index slice, the whole
    buffer's bytes on the host)"""
    words = -(-lay.size // 8)
    buf = torch.full((words + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    sub = buf[:words]
    stream, offs, length = codec.encode(d, bs, sub_index=sub)
    return stream, offs, length, sub, buf.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("case,off", CASES, ids=[f"{c.name}@{off}" for c, off in CASES])
def test_encoder_sub_index_equals_the_reference(torch_mod, codec, oracle, case, off):
    torch = torch_mod
    data = case.data()
    n, bs = data.size, case.blocksize
    want, woffs = oracle.encode(data, bs, with_offsets=True)
    exp = R.expected(want, woffs, data, bs)
    lay = exp.lay
    assert codec.sub_index_bytes(n, bs) == lay.size

    inp = torch.full((n + off + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    d = inp[off:off + n]
    d.copy_(torch.from_numpy(data).cuda())

    # 1. into a buffer of one pattern: the written set as expected, nothing else touched
    stream, offs, length, _, got = encode_into(torch, codec, d, bs, lay, FILL_A)
    st = stream.cpu().numpy()
    assert st.size == want.size and np.array_equal(st, want), case.name
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), woffs), case.name
    fill_a = np.full(got.size // 8, FILL_A, dtype=np.int64).view(np.uint8)
    assert R.mismatches(got, exp) == [], (case.name, "(block, array, index, found, expected)")
    assert R.unwritten_changed(got, fill_a, exp) == [], (case.name, "(block, array, index, found, held)")
    assert np.array_equal(got[lay.size:], fill_a[lay.size:]), (case.name, "guard")

    # 2. into a buffer of another pattern: the same written set
    stream2, offs2, length2, sub2, got2 = encode_into(torch, codec, d, bs, lay, FILL_B)
    assert length2 == length and torch.equal(stream2, stream) and torch.equal(offs2, offs), case.name
    assert R.mismatches(got2, exp) == [], (case.name, "second encode")
    assert np.all(got2[lay.size:] == 0xFF), (case.name, "guard of the second encode")

    # 3. decode with the second sub-index, its unwritten entries all ones
    out_big = torch.full((n + 2 * OUT_GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    out = out_big[OUT_GUARD:OUT_GUARD + n]
    raw = codec.decode(stream2, length2, offs2, lay.nb, out, relaxed=True, sub_index=sub2, raw_size=n, blocksize=bs)
    assert raw == n, case.name
    assert torch.equal(out, d), case.name
    ob = out_big.cpu().numpy()
    assert np.all(ob[:OUT_GUARD] == OUT_FILL) and np.all(ob[OUT_GUARD + n:] == OUT_FILL), (case.name, "output guard")
    # no block goes to the exact decoder, but one with a code over 32 bits (decode_sub.hpp, dsub_fast_tables)
    assert codec.decode_counters()[0] == case.fix, case.name


def seam_hazards(stream, woffs, data, bs) -> int:
    """blocks whose last chunk (a few symbols) ends inside the 4-byte word of its first byte, that byte not the word's
    first: the chunk's first part then stores nothing"""
    exp = R.expected(stream, woffs, data, bs)
    out = 0
    for b, f in enumerate(exp.facts):
        s0, ln = exp.block_syms[b]
        if f["K"] < 2 or ln % R.CHUNK_SYMS == 0 or ln % R.CHUNK_SYMS > 8:
            continue
        c0 = ln - ln % R.CHUNK_SYMS
        pay = 8 * (int(woffs[b]) + 10 + 2 * f["tree_len"])
        P = pay + int(exp.tiles[b * exp.lay.tpb + c0 // R.TILE])
        end = pay + int(exp.groups[b * exp.lay.gpb:(b + 1) * exp.lay.gpb].astype(np.int64).sum())
        out += (P >> 3) % 4 != 0 and end >> 5 == P >> 5
    return out


@pytest.mark.parametrize("cls", ["17_24", "gt24"])
def test_a_last_chunk_of_a_few_symbols_keeps_to_its_bytes(torch_mod, codec, oracle, cls):
    """A block whose last chunk holds 1 to 3 symbols.  pack_segment places and flushes the lanes of a tile in parts when
    codes are long; a part that ended inside the word of the chunk's first byte stored nothing and moved the chunk's
    first owned byte back to that word's start, so its last flush stored zero bits over the previous chunk's last bytes
    (a race the previous chunk mostly lost).  Many such blocks, encoded into outputs of two fills."""
    torch = torch_mod
    hazards = 0
    for tail in (1, 2, 3):
        bs = 2 * R.CHUNK_SYMS * 4 + tail
        rng = np.random.default_rng(tail)
        data = np.concatenate([R.class_data(rng, cls, bs) for _ in range(4)])
        want, woffs = oracle.encode(data, bs, with_offsets=True)
        hazards += seam_hazards(want, woffs, data, bs)
        d = torch.from_numpy(data).cuda()
        for fill in (0x00, 0xFF):
            out = torch.full((codec.encode_bound(data.size, bs),), fill, dtype=torch.uint8, device="cuda")
            st, offs, length = codec.encode(d, bs, out=out)
            got = st.cpu().numpy()
            bad = np.flatnonzero(got != want) if got.size == want.size else [-1]
            assert len(bad) == 0, (cls, tail, fill, [(int(p), int(np.searchsorted(woffs, p, side="right")) - 1) for p in bad[:8]])
    assert hazards >= 2, hazards

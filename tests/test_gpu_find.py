"""GPU tests of hufgpu_find_bytes (GpuCodec.find_bytes / count_bytes): the positions of the bytes of a set of byte values,
straight from stream, block index and sub-index, enqueue-only.

Bit-exact, no tolerance.  Expected values are np.flatnonzero(np.isin(data, values)) of the input through the model of
tests/find_model.py.  The position buffer has guard words in front and behind and is filled with the guard first: the
words beyond totals[1] must still hold it.  Whatever the sub-index holds, a block is either served - status 0, its exact
count and positions - or has a non-zero status and contributes nothing.
"""
import numpy as np
import pytest

from find_model import block_lens, find_model
from find_support import GUARD64, LEAD, OK, RW, TAIL, answer_or_not_served, check, codec, damaged, encoded, find, payload_start, torch_mod
from libhuffman_amd import datagen
from stream_support import GUARD, Enc, dev, make

pytestmark = pytest.mark.gpu

CASES = [("zipf255", "bs4096"), ("zipf255", "bs4099"), ("zipf255", "bs65536"), ("zipf255", "oneblock"), ("two", "bs4099"),
         ("two", "bs65536"), ("l2", "bs4096"), ("l2", "bs65536"), ("long", "bs65536"), ("const41", "bs4096"),
         ("const41", "bs4099"), ("const41", "bs65536"), ("mix", "bs4096"), ("mix", "bs4099")]


def value_sets(data):
    """name -> values: one frequent value, the rarest present, an absent one, none, 128 values"""
    hist = np.bincount(data, minlength=256)
    present = np.flatnonzero(hist)
    absent = np.flatnonzero(hist == 0)
    sets = {"frequent": [int(hist.argmax())], "rarest": [int(present[hist[present].argmin()])], "empty": [],
            "half": [int(v) for v in np.random.default_rng(7).permutation(256)[:128]]}
    if absent.size:
        sets["absent"] = [int(absent[0])]
    return sets


def check_exact_or_not_served(enc, res, values, cap, what=""):
    """every block has status 0 and its exact count and positions, or a non-zero status and contributes nothing"""
    return answer_or_not_served(lambda cap: res, lambda cap, served: find_model(enc.data, values, enc.bs, cap, served=served), cap, what)


# ---- equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_value_sets(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    sets = value_sets(enc.data)
    if kind == "const41":
        sets = {"the value": [41], "another": [42], "empty": [], "half": sets["half"]}
    for name, values in sets.items():
        total = int(find_model(enc.data, values, enc.bs)[2][0])
        if name in ("absent", "empty", "another"):
            assert total == 0
        res = find(torch_mod, codec, enc, values, total + 9)
        assert not res[2].any(), (name, np.flatnonzero(res[2])[:8])
        check(res, find_model(enc.data, values, enc.bs, total + 9), total + 9, name)


@pytest.mark.parametrize("kind", ["zipf255", "const41", "mix"])
def test_the_full_set(torch_mod, codec, kind):
    enc = encoded(torch_mod, codec, kind, "bs4096")
    res = find(torch_mod, codec, enc, bytes(range(256)), enc.n + 2)
    assert np.array_equal(res[0][LEAD:LEAD + enc.n], np.arange(enc.n)) and res[1].tolist() == [enc.n, enc.n, 0, 0]
    check(res, find_model(enc.data, range(256), enc.bs, enc.n + 2), enc.n + 2)
    assert res[3].tolist() == block_lens(enc.n, enc.bs)


def test_uniform256_needs_the_relaxed_flag(torch_mod, codec):
    for shape in ("bs4096", "bs65536"):
        enc = encoded(torch_mod, codec, "uniform256", shape)
        bs = enc.bs
        values = value_sets(enc.data)["half"]
        total = int(find_model(enc.data, values, bs)[2][0])
        res = find(torch_mod, codec, enc, values, total, relaxed=True)
        assert not res[2].any()
        check(res, find_model(enc.data, values, bs, total), total, shape)
        # a tree of all 256 byte values has 1 025 entries and does not parse without the flag: such a block - every
        # whole block here, the short last one only if it happens to hold all values - is not served
        all_values = np.array([np.unique(enc.data[o:o + bs]).size == 256 for o in range(0, enc.n, bs)])
        assert all_values[:enc.n // bs].all()
        res = find(torch_mod, codec, enc, values, total)
        assert np.array_equal(res[2] == RW, all_values), res[2]
        check(res, find_model(enc.data, values, bs, total, served=~all_values), total, shape)


@pytest.mark.parametrize("kind,shape", [("zipf255", "bs4099"), ("zipf255", "oneblock"), ("mix", "bs4096")])
def test_caps(torch_mod, codec, kind, shape):
    enc = encoded(torch_mod, codec, kind, shape)
    values = value_sets(enc.data)["frequent"] + [41]
    total = int(find_model(enc.data, values, enc.bs)[2][0])
    assert total > 2
    for cap in (0, total, total - 1, 1, total + 100):
        res = find(torch_mod, codec, enc, values, cap)          # (cap 0: d_pos is NULL)
        assert not res[2].any() and int(res[1][0]) == total
        check(res, find_model(enc.data, values, enc.bs, cap), cap, cap)
    # without d_block_counts: the same
    res = find(torch_mod, codec, enc, values, total, counts=False)
    check(res, find_model(enc.data, values, enc.bs, total), total)
    totals, errs = codec.count_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, values)
    assert totals.cpu().tolist() == [total, 0, 0, 0] and not errs.cpu().numpy().any()


# ---- any content of the sub-index --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape", [("zipf255", "bs4096"), ("mix", "bs4096"), ("zipf255", "bs65536")])
def test_sub_index_abuse(torch_mod, codec, kind, shape):
    torch = torch_mod
    enc = encoded(torch, codec, kind, shape)
    values = value_sets(enc.data)["frequent"] + [41, 0]
    cap = int(find_model(enc.data, values, enc.bs)[2][0]) + 3
    rng = np.random.default_rng(13)
    bs = enc.bs
    one_leaf = np.array([np.unique(enc.data[o:o + bs]).size == 1 for o in range(0, enc.n, bs)])
    # a bit count of 0 or of 65 535 cannot be that of 32 codewords, a code length of 0 or 255 is not the tree's
    for name, sub in (("zeros", torch.zeros_like(enc.sub)), ("ones", torch.full_like(enc.sub, -1))):
        errs = check_exact_or_not_served(enc, find(torch, codec, enc, values, cap, sub=sub), values, cap, name)
        assert np.array_equal(errs != OK, ~one_leaf), name
    other = Enc(torch, codec, make("two", enc.n, enc.bs), enc.bs, sub=True)
    for name, sub in (("random", torch.from_numpy(rng.integers(-2**62, 2**62, enc.sub.numel())).cuda()), ("foreign", other.sub)):
        errs = check_exact_or_not_served(enc, find(torch, codec, enc, values, cap, sub=sub), values, cap, name)
        assert not errs[one_leaf].any(), name                       # (one-symbol blocks have no rows to be wrong)


# ---- damage ------------------------------------------------------------------------------------------------------------


def only_this_block(enc, res, values, cap, b):
    errs = check_exact_or_not_served(enc, res, values, cap)
    want = np.zeros(enc.nb, np.int32)
    want[b] = RW
    assert np.array_equal(errs, want), errs


def test_a_flipped_payload_bit(torch_mod, codec):
    """two byte values have the codes 00 and 01: a 1 at an even payload bit leaves the tree, whichever group it is in"""
    enc = encoded(torch_mod, codec, "two", "bs65536")
    values = [7]
    cap = int(find_model(enc.data, values, enc.bs)[2][0])
    for bit in (2 * 20000, 0, 2 * 65535):
        bad = damaged(enc, payload_start(enc, 1) + bit // 8, 0x80 >> (bit % 8))
        only_this_block(enc, find(torch_mod, codec, bad, values, cap), values, cap, 1)


def test_a_flipped_payload_bit_in_many_codes(torch_mod, codec):
    """zipf255: the damaged group may take its bits by chance - then the block is served with what decode delivers"""
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", "bs65536")
    values = value_sets(enc.data)["half"]
    cap = int(find_model(enc.data, values, enc.bs)[2][0]) + 5
    seen = []
    for at, xor in ((12345, 0x10), (777, 0x01), (40001, 0x80)):
        bad = damaged(enc, payload_start(enc, 1) + at, xor)
        res = find(torch, codec, bad, values, cap)
        if res[2][1] == OK:                             # served: the bytes are those of the exact decoder
            out = torch.empty(enc.n, dtype=torch.uint8, device="cuda")
            assert codec.decode(bad.stream, bad.length, bad.offsets, bad.nb, out) == enc.n
            now = bad.with_stream(bad.stream)
            now.data = out.cpu().numpy()
            check_exact_or_not_served(now, res, values, cap)
        else:
            only_this_block(enc, res, values, cap, 1)
        seen.append(int(res[2][1]))
    assert RW in seen, "no damage was noticed"


def test_tree_and_header_damage(torch_mod, codec):
    torch = torch_mod
    enc = encoded(torch, codec, "zipf255", "bs65536")
    values = value_sets(enc.data)["frequent"]
    cap = int(find_model(enc.data, values, enc.bs)[2][0])
    bo = int(enc.h_offs[1])
    # the root's entry overwritten with a marker; block_len changed; a tree_len that reaches past the block's record
    st = enc.stream.clone()
    st[bo + 10] = 0xFF
    st[bo + 11] = 0xFF
    only_this_block(enc, find(torch, codec, enc.with_stream(st), values, cap), values, cap, 1)
    for at, xor in ((bo, 0x01), (bo + 3, 0x01), (bo + 9, 0x40)):
        only_this_block(enc, find(torch, codec, damaged(enc, at, xor), values, cap), values, cap, 1)


def test_one_symbol_payload_damage(torch_mod, codec):
    enc = encoded(torch_mod, codec, "const41", "bs4096")
    cap = enc.n
    for sym in (100, 0, 4095):
        bad = damaged(enc, payload_start(enc, 1) + sym // 8, 0x80 >> (sym % 8))
        only_this_block(enc, find(torch_mod, codec, bad, [41], cap), [41], cap, 1)


# ---- other sub-indexes and layouts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["bs4099", "bs65536"])
def test_built_sub_index(torch_mod, codec, shape):
    enc = encoded(torch_mod, codec, "zipf255", shape)
    built, unbuilt = codec.build_sub_index(enc.stream, enc.length, enc.offsets, enc.n, enc.bs)
    assert unbuilt == 0
    values = value_sets(enc.data)["half"]
    cap = int(find_model(enc.data, values, enc.bs)[2][0])
    res = find(torch_mod, codec, enc, values, cap, sub=built)
    assert not res[2].any()
    check(res, find_model(enc.data, values, enc.bs, cap), cap)


def test_a_batch_stream(torch_mod, codec):
    """a batch's stream with (nblocks x row_blocksize, row_blocksize): full blocks are served and addressed from
    b * row_blocksize, the items' short last blocks do not have the layout's length and are reported not served"""
    torch = torch_mod
    bs = 4096
    lens = [5000, 0, 70000, 3, 12345, 4096]
    data = np.concatenate([datagen.zipf255(x, seed=50 + i) if x else np.zeros(0, np.uint8) for i, x in enumerate(lens)])
    batch = codec.encode_batch(dev(torch, data), lens, bs, sub_index=True)
    blens = [min(bs, x - o) for x in lens for o in range(0, x, bs)]
    enc = Enc(torch, codec, data, bs, stream=batch.stream, offsets=batch.offsets, block_lens=blens)
    enc.sub, enc.raw_size, enc.row_bs = batch.sub_index, batch.nblocks * batch.row_blocksize, batch.row_blocksize
    assert enc.nb == batch.nblocks and batch.row_blocksize == bs
    full = np.array([x == bs for x in blens])
    assert not full.all() and full.any()
    # the same bytes as the layout sees them: block b at b * bs, short blocks empty
    laid = np.zeros(enc.nb * bs, np.uint8)
    for b in np.flatnonzero(full):
        laid[b * bs:(b + 1) * bs] = data[int(enc.P[b]):int(enc.P[b]) + bs]
    values = [int(np.bincount(data).argmax())]
    cap = int(find_model(laid, values, bs, served=full)[2][0]) + 4
    res = find(torch, codec, enc, values, cap)
    assert np.array_equal(res[2] == OK, full), res[2]
    check(res, find_model(laid, values, bs, cap, served=full), cap)


# ---- sequencing --------------------------------------------------------------------------------------------------------
def test_two_calls_back_to_back(torch_mod, codec):
    """no synchronise between the two calls, one behind them: the buffers are made first"""
    torch = torch_mod
    jobs = []
    for kind, shape, pick in (("zipf255", "bs4096", "frequent"), ("long", "bs65536", "half")):
        enc = encoded(torch, codec, kind, shape)
        values = value_sets(enc.data)[pick]
        cap = int(find_model(enc.data, values, enc.bs)[2][0]) + 2
        jobs.append((enc, values, cap, torch.full((LEAD + cap + TAIL,), GUARD64, dtype=torch.int64, device="cuda")))
    torch.cuda.synchronize()
    res = []
    for enc, values, cap, buf in jobs:
        res.append(codec.find_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, values,
                                    max_positions=cap, block_counts=True, out=buf[LEAD:LEAD + cap]))
    torch.cuda.synchronize()
    for (enc, values, cap, buf), (_, totals, errs, cnt) in zip(jobs, res):
        check((buf.cpu().numpy(), totals.cpu().numpy(), errs.cpu().numpy(), cnt.cpu().numpy()),
              find_model(enc.data, values, enc.bs, cap), cap)


def test_between_two_decodes(torch_mod, codec):
    torch = torch_mod
    a = encoded(torch, codec, "zipf255", "bs4096")
    b = encoded(torch, codec, "zipf255", "bs65536")
    out = torch.full((b.n + 3,), GUARD, dtype=torch.uint8, device="cuda")
    assert codec.decode(b.stream, b.length, b.offsets, b.nb, out, sub_index=b.sub, raw_size=b.n, blocksize=b.bs) == b.n
    values = value_sets(a.data)["half"]
    cap = int(find_model(a.data, values, a.bs)[2][0])
    check(find(torch, codec, a, values, cap), find_model(a.data, values, a.bs, cap), cap)
    h = out.cpu().numpy()
    assert np.array_equal(h[:b.n], b.data) and np.all(h[b.n:] == GUARD)
    assert codec.decode(a.stream, a.length, a.offsets, a.nb, out[:a.n]) == a.n
    assert np.array_equal(out.cpu().numpy()[:a.n], a.data)


def test_no_blocks(torch_mod, codec):
    torch = torch_mod
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(1, dtype=torch.int64, device="cuda")
    buf = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    pos, totals, errs, cnt = codec.find_bytes(empty, 0, offsets, 0, codec.new_sub_index(0, 4096), 0, 4096, [10],
                                              max_positions=4, block_counts=True, out=buf)
    assert totals.cpu().tolist() == [0, 0, 0, 0] and errs.numel() == 0 and cnt.numel() == 0
    assert buf.cpu().tolist() == [GUARD64] * 4


# ---- the pipeline ------------------------------------------------------------------------------------------------------
def test_newlines_feed_a_gather(torch_mod, codec):
    """find_bytes({10}) -> positions + 1 by a torch op on the device -> gather(max_len=64): the 64 bytes behind each
    newline, with no host synchronisation between the two calls (the cap is host-known: a line has at least 40 bytes)"""
    torch = torch_mod
    n, bs = 1 << 20, 65536
    data = datagen.logtext(n)
    enc = Enc(torch, codec, data, bs, sub=True)
    want = np.flatnonzero(data == 10)
    cap = n // 40
    assert 0 < want.size <= cap
    pos, totals, errs, _ = codec.find_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, n, bs, b"\n", max_positions=cap)
    starts = torch.where(torch.arange(cap, device="cuda") < totals[1], pos + 1, n)      # (past the end: a record of 0 bytes)
    rows, gerrs, raws = codec.gather(enc.stream, enc.length, enc.offsets, enc.nb, starts, 64, sub_index=enc.sub, raw_size=n, blocksize=bs)
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [want.size, want.size, 0, 0] and not errs.cpu().numpy().any()
    assert np.array_equal(pos.cpu().numpy()[:want.size], want)
    rows, gerrs, raws = rows.cpu().numpy(), gerrs.cpu().numpy(), raws.cpu().numpy()
    assert not gerrs.any() and not raws[want.size:].any()
    for i, p in enumerate(want):
        c = min(64, n - (p + 1))
        assert raws[i] == c and np.array_equal(rows[i, :c], data[p + 1:p + 1 + c]), i

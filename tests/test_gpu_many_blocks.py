"""GPU tests at block counts that cross the edges of the prefix sums (kernels/offsets.hpp), for every route that places
per-block values with them.

The three edges: 256 blocks are one scan group (below that gprefix[i / SCAN_GROUP] is gprefix[0] == 0 and a consumer that
forgot the group term is right); 64 groups = 16 384 blocks or tiles are one pass of two_level_finish (beyond it the carry
and the running minimum across passes are used); 16 384 elements (4 096 in app_index_kernel) are one chunk of
chunked_excl_scan (beyond it the second chunk's carry, and with an index 8 bytes off a 16-byte boundary the word-by-word
stores).  Many blocks are not much data: S64 is at most 16 700 blocks of 64 bytes, S2049 8 200 blocks of 2 049 bytes -
two sub-index tiles, the second of one symbol, 16 400 tiles.

Bit-exact, no tolerance.  Expected values come from the input in numpy and from the oracle's encoder, never from another
GPU call; every output buffer lies between guard bytes.  The module uses ONE context from its first call to its last, and
every call is made twice in a row: tickets and `done` that are not back at zero show in the second.
"""
import ctypes as C

import numpy as np
import pytest

import sub_index_ref as sref
import test_gpu_append as ap
import test_gpu_range_tiles as rt
import test_gpu_update as upd
from find_model import find_model
from test_gpu_find import check, find, value_sets
from test_gpu_gather import check_good, check_guards, cut, gather
from test_gpu_ranges import GUARD, Enc, check_all_good, dev, slots_for

pytestmark = pytest.mark.gpu

SCAN_GROUP, PASS = 256, 64 * 256        # a group; what one pass of two_level_finish / one chunk of 1 024 threads covers
OK, MEMORY, RW, OVERFLOW = 0, 1, 3, 5
GUARD_BYTES = 80
IDX_FILL, SUB_FILL = ap.IDX_FILL, ap.SUB_FILL
S64_COUNTS = (257, 16384, 16385, 16700)
S64_POOL = 20500                        # blocks of bytes made for S64: the append test needs 16 380 + 4 100
KEYS_DAGGER = [f"s64-{nb}" for nb in S64_COUNTS]
KEYS_BOTH = ["s64-16700", "s2049"]
# whole blocks of one value (no sub-index rows, the fill paths): (first block, blocks, the value)
RUNS_64 = [(2, 3, 65), (255, 1, 66), (257, 2, 67), (16382, 2, 68), (16385, 2, 69), (16498, 5, 70), (16650, 6, 71)]
RUNS_2049 = [(2, 2, 65), (255, 1, 66), (257, 1, 67), (8191, 1, 68), (8193, 1, 69), (8197, 1, 70)]


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


# ---- inputs: made once, never changed --------------------------------------------------------------------------------
def s64_pool():
    """S64_POOL blocks of 64 bytes: per block a share p of the bytes from 4 values, the rest from 64 (p uniform, a half on
    average): the encoded sizes differ strongly from block to block; 64 bytes cannot hold all 256 values"""
    rng = np.random.default_rng(64)
    shape = (S64_POOL, 64)
    few = rng.random(shape) < rng.random(S64_POOL)[:, None]
    data = np.where(few, rng.integers(0, 4, shape), rng.integers(0, 64, shape)).astype(np.uint8).reshape(-1)
    for b0, k, v in RUNS_64:
        data[b0 * 64:(b0 + k) * 64] = v
    return data


def s2049_data():
    from libhuffman_amd import datagen
    bs = 2049
    data = datagen.zipf255(8199 * bs + 1500, seed=3).copy()
    for b0, k, v in RUNS_2049:
        data[b0 * bs:(b0 + k) * bs] = v
    return data


class Input:
    """an input, the oracle's stream and index of it, the reference's sub-index; .enc (on the device) comes later"""

    def __init__(self, oracle, data, bs):
        self.data, self.bs, self.n = data, bs, int(data.size)
        self.nb = -(-self.n // bs)
        self.want, woffs = oracle.encode(data, bs, with_offsets=True)
        self.woffs = np.asarray(woffs, dtype=np.uint64)
        self.exp = sref.expected(self.want, self.woffs, data, bs)
        self.one = np.array([f["tree_len"] == 5 for f in self.exp.facts])
        self.P = np.minimum(np.arange(self.nb + 1, dtype=np.int64) * bs, self.n)
        self.enc = None
        setup_asserts(self)


def setup_asserts(inp):
    """a wrong scan must show: sizes that differ, sums that differ with and without the group term and the carry"""
    offs = inp.woffs.astype(np.int64)
    sizes, lens = np.diff(offs), np.diff(inp.P)
    assert np.unique(sizes).size > 50 and np.unique(lens).size == 2 and lens[-1] < inp.bs
    for i in (256, 16384, 16385):
        if i <= inp.nb:
            no_group = offs[i] - offs[i // SCAN_GROUP * SCAN_GROUP]          # local[i] alone
            no_carry = offs[i] - offs[i // PASS * PASS]                      # a second pass / chunk that starts at 0
            assert no_group != offs[i], i
            if i >= PASS:
                assert no_carry != offs[i], i
    groups = set((np.flatnonzero(inp.one) // SCAN_GROUP).tolist())
    assert 0 in groups and not inp.one.all()
    if inp.nb in (16700, 8200):                         # the whole inputs (the smaller S64 are their first blocks)
        assert (inp.nb - 1) // SCAN_GROUP in groups, "one-symbol blocks in the last group"
    if inp.nb == 16700:
        assert 64 in groups and 65 in groups


_inputs = {}


def pool_bytes():
    if "pool" not in _inputs:
        _inputs["pool"] = s64_pool()
    return _inputs["pool"]


def cpu_input(oracle, key):
    if key not in _inputs:
        if key == "s2049":
            _inputs[key] = Input(oracle, s2049_data(), 2049)
        else:
            nb = int(key.split("-")[1])
            _inputs[key] = Input(oracle, pool_bytes()[:(nb - 1) * 64 + 21], 64)
    return _inputs[key]


def gpu_input(torch, codec, oracle, key):
    """the input with its encode on the device (with the sub-index), dressed for the helpers of the other test modules"""
    inp = cpu_input(oracle, key)
    if inp.enc is None:
        enc = Enc(torch, codec, inp.data, inp.bs, sub=True)
        enc.codec, enc.raw_size, enc.row_bs = codec, enc.n, enc.bs
        enc.block_lens = np.diff(enc.P)
        enc.elig = ~inp.one                              # (one-symbol blocks have no rows: never by tiles)
        assert enc.nb == inp.nb and np.array_equal(enc.P, inp.P)
        inp.enc = enc
    return inp


def twice(fn):
    """every call is made twice in a row"""
    fn()
    return fn()


def guarded(torch, n, lead=GUARD_BYTES):
    big = torch.full((n + 2 * lead,), GUARD, dtype=torch.uint8, device="cuda")
    return big, big[lead:lead + n]


def guards_intact(big, n, lead=GUARD_BYTES):
    h = big.cpu().numpy()
    return bool(np.all(h[:lead] == GUARD) and np.all(h[lead + n:] == GUARD))


def sub_buffer(torch, nbytes):
    words = max(1, -(-nbytes // 8))
    big = torch.full((words + 4,), SUB_FILL, dtype=torch.int64, device="cuda")
    return big, big[2:2 + words]


def check_sub(big, exp, what):
    """a sub-index buffer that was filled with SUB_FILL: the written set equals the reference's, nothing else changed"""
    h = big.cpu().numpy()
    assert np.all(h[:2] == SUB_FILL) and np.all(h[-2:] == SUB_FILL), (what, "guard words around the sub-index")
    got = h[2:-2].view(np.uint8)
    held = np.full(got.size // 8, SUB_FILL, dtype=np.int64).view(np.uint8)
    assert sref.mismatches(got, exp) == [], (what, "(block, array, index, found, expected)")
    assert sref.unwritten_changed(got, held, exp) == [], (what, "(block, array, index, found, held)")
    assert np.array_equal(got[exp.lay.size:], held[exp.lay.size:]), (what, "behind the sub-index")


# ---- 1. encode and the decoders ----------------------------------------------------------------------------------------
def decode_guarded(torch, codec, inp, st, length, offs, **kw):
    big, out = guarded(torch, inp.n, lead=GUARD_BYTES + 3)
    assert codec.decode(st, length, offs, inp.nb, out, **kw) == inp.n
    assert guards_intact(big, inp.n, GUARD_BYTES + 3)
    return out.cpu().numpy()


@pytest.mark.parametrize("key", KEYS_DAGGER + ["s2049"])
def test_encode_and_the_decoders(torch_mod, codec, oracle, key):
    """257: the group term; 16 384 / 16 385 / 16 700 blocks, 16 400 tiles: the second pass of two_level_finish (encode's
    sizes, the decoders' output positions, sub_build's rows) and the second chunk of cand_lens_kernel (the raw stream)"""
    torch = torch_mod
    inp = cpu_input(oracle, key)
    n, bs, nb = inp.n, inp.bs, inp.nb
    d_in = dev(torch, inp.data)
    cap = codec.encode_bound(n, bs)
    for idx_lead in (2, 1, 2):                          # the index 16-byte aligned, 8 bytes off, and aligned again
        big, out = guarded(torch, cap)
        idx_big = torch.full((nb + 1 + 4,), IDX_FILL, dtype=torch.int64, device="cuda")
        offs = idx_big[idx_lead:idx_lead + nb + 1]
        sub_big, sub = sub_buffer(torch, codec.sub_index_bytes(n, bs))
        st, _, length = codec.encode(d_in, bs, out=out, offsets=offs, sub_index=sub)
        what = (key, idx_lead)
        hi = idx_big.cpu().numpy()
        assert np.all(hi[:idx_lead] == IDX_FILL) and np.all(hi[idx_lead + nb + 1:] == IDX_FILL), what
        got_offs = hi[idx_lead:idx_lead + nb + 1].astype(np.uint64)
        bad = np.flatnonzero(got_offs != inp.woffs)
        assert bad.size == 0, (what, "index differs from the oracle's first at", bad[:4], got_offs[bad[:4]], inp.woffs[bad[:4]])
        hb = big.cpu().numpy()
        assert length == inp.want.size and np.array_equal(hb[GUARD_BYTES:GUARD_BYTES + length], inp.want), what
        assert np.all(hb[:GUARD_BYTES] == GUARD) and np.all(hb[GUARD_BYTES + length:] == GUARD), what
        check_sub(sub_big, inp.exp, what)

        # the block index alone, the sub-index, the raw stream, the index of the raw stream
        assert np.array_equal(decode_guarded(torch, codec, inp, st, length, offs), inp.data), what
        back = decode_guarded(torch, codec, inp, st, length, offs, sub_index=sub, raw_size=n, blocksize=bs)
        assert np.array_equal(back, inp.data) and codec.decode_counters()[0] == 0, what
        raw = torch.zeros(length + 64, dtype=torch.uint8, device="cuda")
        raw[:length] = st
        big, out = guarded(torch, n)
        assert codec.decode_stream(raw[:length], length, length, out) == (0, n, length), what
        assert np.array_equal(out.cpu().numpy(), inp.data) and guards_intact(big, n), what
        d_index, cnt, used = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        rc = codec.lib.hufgpu_block_index(codec._ctx, C.c_void_p(raw.data_ptr()), C.c_uint64(length), C.c_uint64(length),
                                          C.c_uint32(0), C.byref(d_index), C.byref(cnt), C.byref(used), None)
        assert (rc, cnt.value, used.value) == (0, nb, length), what
        found = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
        assert codec.lib.hufgpu_memcpy_d2d(codec._ctx, C.c_void_p(found.data_ptr()), d_index, C.c_uint64(8 * (nb + 1))) == 0
        assert np.array_equal(found.cpu().numpy().astype(np.uint64), inp.woffs), what

        # the two builders: the decode's output and the rows the encoder wrote
        built_big, built = sub_buffer(torch, codec.sub_index_bytes(n, bs))
        big, out = guarded(torch, n)
        assert codec.decode_build_sub(st, length, offs, out, n, bs, sub_index=built)[::2] == (n, 0), what
        assert np.array_equal(out.cpu().numpy(), inp.data) and guards_intact(big, n), what
        check_sub(built_big, inp.exp, what + ("decode_build_sub",))
        assert torch_mod.equal(built_big, sub_big), what
        built_big, built = sub_buffer(torch, codec.sub_index_bytes(n, bs))
        assert codec.build_sub_index(st, length, offs, n, bs, sub_index=built)[1] == 0, what
        check_sub(built_big, inp.exp, what + ("build_sub_index",))
        assert torch_mod.equal(built_big, sub_big), what


# ---- 2. decode_ranges --------------------------------------------------------------------------------------------------
def edge_blocks(inp):
    """(the blocks around the group edge, around the second-pass edge - of blocks for S64, of tiles for S2049 -, a block
    of the last groups that many ranges share)"""
    return (255, 16383, 16650 + 8) if inp.bs == 64 else (255, 8191, 8195)


def some_ranges(inp, seed, count=300):
    bs, n = inp.bs, inp.n
    g, e, shared = edge_blocks(inp)
    r = [(300 * bs + 5, 300 * bs + 40),                                      # inside block 300
         (g * bs + 7, (g + 2) * bs + bs - 5), (e * bs + 9, (e + 2) * bs + bs - 3),   # across three blocks, cut on both sides
         (g * bs + bs - 1, (g + 1) * bs + 1), ((e + 1) * bs - 2, (e + 1) * bs + 2),
         (5, 5), (n, n), (0, 0), (n - 10, n + 100), (n + 3, n + 8), (n, n + 50)]
    r += [(shared * bs + k, shared * bs + k + 1 + k % 7) for k in range(40)]  # forty ranges in one block
    rng = np.random.default_rng(seed)
    for _ in range(count):
        lo = int(rng.integers(0, n + 10))
        span = int(rng.choice([0, 1, 17, bs // 2, bs, bs + 1, 3 * bs + 5])) + int(rng.integers(0, 64))
        r.append((lo, lo + int(rng.integers(0, span + 1))))
    order = rng.permutation(len(r))
    return [r[int(j)] for j in order]


def ranges_three_ways(torch, codec, enc, ranges):
    """with the sub-index and the flag, with the sub-index, with the block index alone: slices of the input per range,
    the guards, and the counters of the routing rule"""
    oo = slots_for(ranges, enc.n)
    direct, staged, tiles, items = rt.model(enc, ranges, oo)
    for name, flag, sub in (("tiles", True, "own"), ("sub-index", False, "own"), ("block index", False, None)):
        got, errs, raws = twice(lambda: rt.call(torch, codec, enc, ranges, oo, flag, sub_index=sub))
        check_all_good(enc, ranges, got, errs, raws, oo)
        cnt = codec.ranges_counters()
        if flag:
            assert cnt == (direct, staged, tiles, items, 0, 0, 0, 0), (name, cnt, (direct, staged, tiles, items))
        else:                                            # without the flag the tile blocks are staged
            assert cnt[:3] == (direct, staged + tiles, 0), (name, cnt, (direct, staged, tiles))
    return direct, staged, tiles


@pytest.mark.parametrize("key", KEYS_BOTH)
def test_decode_ranges(torch_mod, codec, oracle, key):
    """drange_pos across groups and passes, the strided loops of mark and result over thousands of direct blocks, the
    binary searches over positions that carry a group term"""
    inp = gpu_input(torch_mod, codec, oracle, key)
    enc, n = inp.enc, inp.n
    direct, staged, tiles = ranges_three_ways(torch_mod, codec, enc, [(3, n - 5), (n, n), (n + 3, n + 8), (5, 5)])
    assert direct == inp.nb - 2 and staged + tiles == 2
    direct, staged, tiles = ranges_three_ways(torch_mod, codec, enc, [(7, 7), (0, n), (n, n + 50)])
    assert (direct, staged, tiles) == (inp.nb, 0, 0)
    direct, staged, tiles = ranges_three_ways(torch_mod, codec, enc, some_ranges(inp, 11))
    assert direct > 0 and staged > 0 and tiles > 40     # (the shared block and cut one-symbol blocks are staged)
    # a three-block call, then the many-block call again: nothing of the large call's sums leaks into the small one
    bs = inp.bs
    small = Enc(torch_mod, codec, inp.data[:2 * bs + 21], bs, sub=True)
    small.raw_size, small.row_bs, small.block_lens, small.elig = small.n, bs, np.diff(small.P), ~inp.one[:3]
    ranges_three_ways(torch_mod, codec, small, [(3, small.n - 5), (bs + 1, bs + 9), (0, small.n), (bs - 1, bs + 1)])
    ranges_three_ways(torch_mod, codec, enc, some_ranges(inp, 12, 100))


# ---- 3. gather ---------------------------------------------------------------------------------------------------------
def gather_good(torch, codec, enc, pos, lens, max_len=None, spare=5, lead=3):
    got, errs, raws, stride = twice(lambda: gather(torch, codec, enc, pos, lens, max_len=max_len, spare=spare, lead=lead))
    check_good(enc, got, errs, raws, pos, lens, stride, lead)
    return got


@pytest.mark.parametrize("key", KEYS_BOTH)
def test_gather(torch_mod, codec, oracle, key):
    """the touched blocks' list slots (gather_place_kernel) across groups and, on S64, passes; gather_serve_kernel's
    stride over more touched blocks than workgroups"""
    torch = torch_mod
    inp = gpu_input(torch, codec, oracle, key)
    enc, bs, n, nb = inp.enc, inp.bs, inp.n, inp.nb
    g, e, _ = edge_blocks(inp)
    rng = np.random.default_rng(31)
    ln = 48 if bs == 64 else 300
    # (a) records only behind the second-pass edge: every group in front is untouched
    late = [int(x) for x in rng.integers((e + 1) * bs, n - ln, 500)]
    gather_good(torch, codec, enc, late, ln)
    # (b) records that straddle the borders of the group edge and the pass edge
    borders = [(g + 1) * bs, (e + 1) * bs]
    pos = [p - k for p in borders for k in (0, 1, ln // 2, ln - 1)] + [borders[1] - bs - 3]
    gather_good(torch, codec, enc, pos, ln, spare=0, lead=1)
    # (c) one record in every block, the short last one included
    every = [b * bs + (b * 37) % (bs - 16) for b in range(nb - 1)] + [(nb - 1) * bs + 9]
    gather_good(torch, codec, enc, every, 16, spare=1, lead=7)
    # the same kind of call with three records, then the large one again
    gather_good(torch, codec, enc, [5, bs + 1, 2 * bs - 3], 16)
    gather_good(torch, codec, enc, every, 16, spare=1, lead=7)
    # (d) 5 000 records anywhere, fixed length and lengths from the device
    pos = [int(x) for x in rng.integers(0, n + 5, 5000)]
    gather_good(torch, codec, enc, pos, ln)
    lens = [int(x) for x in rng.integers(0, 101, len(pos))]
    lens[:3] = [100, 0, 1]
    gather_good(torch, codec, enc, pos, lens, max_len=100)


# ---- 4. find_bytes / count_bytes ---------------------------------------------------------------------------------------
def model_with_room(enc, values, room=9):
    """(positions, counts, totals) of the model with `room` words more than it needs, and that cap"""
    pos, counts, totals = find_model(enc.data, values, enc.bs, enc.n + room)
    return (pos, counts, totals), int(totals[0]) + room


@pytest.mark.parametrize("key", KEYS_BOTH)
def test_find_bytes(torch_mod, codec, oracle, key):
    """a block's rank = the sum over its tiles' counts: find_finish_kernel's (b + 1) * tpb across groups and, at 16 400
    and 16 700 tiles, passes; the cap cuts inside a block whose prefix carries both terms"""
    torch = torch_mod
    inp = gpu_input(torch, codec, oracle, key)
    enc = inp.enc
    sets = value_sets(enc.data)
    assert "absent" in sets
    sets["all 256"] = list(range(256))
    sets["a run's value"] = [70]
    for name, values in sets.items():
        want, cap = model_with_room(enc, values)
        if name in ("absent", "empty"):
            assert cap == 9
        if name == "all 256":
            assert np.array_equal(want[0], np.arange(enc.n)) and want[1].tolist() == np.diff(inp.P).tolist()
        res = twice(lambda: find(torch, codec, enc, values, cap))
        assert not res[2].any(), (name, np.flatnonzero(res[2])[:8])
        check(res, want, cap, name)
        totals, errs = codec.count_bytes(enc.stream, enc.length, enc.offsets, enc.nb, enc.sub, enc.n, enc.bs, values)
        assert totals.cpu().tolist() == [int(want[2][0]), 0, 0, 0] and not errs.cpu().numpy().any(), name
    # the cap cuts the list inside a block behind the second-pass edge; the words behind totals[1] keep the guard
    values = sets["frequent"] + sets["half"][:40]
    counts = find_model(enc.data, values, enc.bs)[1]
    _, e, shared = edge_blocks(inp)
    b = shared + 1 + int(np.argmax(counts[shared + 1:] >= 2))
    assert b > e + 1 and counts[b] >= 2
    cap = int(counts[:b].sum()) + int(counts[b]) // 2
    want = find_model(enc.data, values, enc.bs, cap)
    assert 0 < int(want[2][1]) == cap < int(want[2][0])
    check(twice(lambda: find(torch, codec, enc, values, cap)), want, cap, "cut")
    # three blocks, then the many again
    small = Enc(torch, codec, inp.data[:2 * inp.bs + 21], inp.bs, sub=True)
    small.raw_size, small.row_bs = small.n, small.bs
    want3, cap3 = model_with_room(small, values)
    check(find(torch, codec, small, values, cap3), want3, cap3, "three blocks")
    check(find(torch, codec, enc, values, cap), want, cap, "cut, again")


# ---- 5. update_ranges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS_DAGGER)
def test_update_ranges(torch_mod, codec, oracle, key):
    """upd_index_kernel's second chunk (16 385 and 16 700 blocks) and its word-by-word stores (idx_lead 1); the touched
    blocks' rows at both ends of the group and pass edges"""
    torch = torch_mod
    inp = gpu_input(torch, codec, oracle, key)
    enc, bs, n, nb = inp.enc, inp.bs, inp.n, inp.nb
    rng = np.random.default_rng(nb)
    blocks = [b for b in (0, 255, 256, 16383, 16384) if b < nb - 1]
    ranges = [(b * bs + 3 + k, b * bs + 13 + 2 * k) for k, b in enumerate(blocks)] + [((nb - 1) * bs + 2, (nb - 1) * bs + 12)]
    patches = [rng.integers(0, 256, hi - lo, dtype=np.uint8) for lo, hi in ranges]
    # a block of the last group becomes one value, a one-value block of it gets 64 different bytes
    free = np.ones(nb - 1, bool)
    free[blocks] = False                                # (no block is patched twice)
    plain = int(np.flatnonzero(~inp.one[:nb - 1] & free)[-1])
    run = int(np.flatnonzero(inp.one[:nb - 1] & free)[-1])
    if nb == 16700:
        assert plain // SCAN_GROUP == run // SCAN_GROUP == 65
    ranges += [(plain * bs, (plain + 1) * bs), (run * bs, (run + 1) * bs)]
    patches += [np.full(bs, 99, np.uint8), rng.permutation(bs).astype(np.uint8)]
    everything = np.roll(inp.data, 5 * bs + 1)
    for what, rr, pp in (("patches", ranges, patches), ("everything", [(0, n)], [everything]),
                         ("three blocks", None, None), ("patches again", ranges, patches)):
        for idx_lead in (2, 1):
            e = enc
            if rr is None:                                  # a small call of the same kind between the large ones
                e = Enc(torch, codec, inp.data[:2 * bs + 21], bs, sub=True)
                rr_, pp_ = [(bs - 2, bs + 9)], [rng.integers(0, 256, 11, dtype=np.uint8)]
            else:
                rr_, pp_ = rr, pp
            r = twice(lambda: upd.update(torch, codec, e, rr_, pp_, old_sub=e.sub, want_sub=True, idx_lead=idx_lead,
                                         scatter_seed=idx_lead if rr_ is ranges else None))
            tag = (key, what, idx_lead)
            new, want, woffs = upd.check_equals_encode(torch, codec, oracle, e, rr_, pp_, r, tag)
            got = r.sub.cpu().numpy().view(np.uint8)
            exp = sref.expected(want, woffs, new, bs)
            assert sref.mismatches(got, exp) == [], tag + ("(block, array, index, found, expected)",)
            held = np.full(got.size // 8, 0x7B7B7B7B7B7B7B7B, dtype=np.int64).view(np.uint8)
            assert sref.unwritten_changed(got, held, exp) == [], tag + ("(block, array, index, found, held)",)


# ---- 6. append / truncate ----------------------------------------------------------------------------------------------
def test_append_and_truncate(torch_mod, codec, oracle):
    """4 100 new rows: app_index_kernel's second chunk of 4 096; the result has 20 480 blocks - the packer's prefix of the
    new rows crosses a pass; truncate cuts in the group behind the pass edge and back to the first group's edge"""
    torch = torch_mod
    bs = 64
    pool = pool_bytes()
    raw = 16379 * bs + 21                                # 16 380 blocks, the last one short: it is encoded again
    la = 4100 * bs
    assert raw + la <= pool.size
    for rep in range(2):
        buf = ap.Buf(torch, codec, pool[:raw], bs, entries=ap.nblocks(raw + la, bs) + 1, room=ap.bound(21 + la, bs), sub=True)
        r = ap.append(torch, codec, buf, pool[raw:raw + la], src_off=1, old_sub=buf.sub, want_sub=True)
        want, woffs = ap.check_equals_encode(torch, codec, oracle, pool[:raw + la], bs, r, ("append", rep))
        ap.check_sub_index(torch, codec, r, buf.stream, buf.index, pool[:raw + la], want, woffs, bs)
        buf.raw, buf.length = raw + la, r.length
        cut1 = 16383 * bs + 5
        r1 = ap.truncate(torch, codec, buf, cut1, old_sub=r.sub, want_sub=True)
        want, woffs = ap.check_equals_encode(torch, codec, oracle, pool[:cut1], bs, r1, ("truncate", rep))
        ap.check_sub_index(torch, codec, r1, buf.stream, buf.index, pool[:cut1], want, woffs, bs)
        buf.raw, buf.length = cut1, r1.length
        r2 = ap.truncate(torch, codec, buf, 255 * bs, old_sub=r1.sub, want_sub=True)
        want, woffs = ap.check_equals_encode(torch, codec, oracle, pool[:255 * bs], bs, r2, ("truncate to 255", rep))
        ap.check_sub_index(torch, codec, r2, buf.stream, buf.index, pool[:255 * bs], want, woffs, bs)
        # a three-block stream gets a few bytes, between the two large rounds
        small = ap.Buf(torch, codec, pool[:2 * bs + 21], bs, entries=5, room=ap.bound(21 + 70, bs), sub=True)
        r3 = ap.append(torch, codec, small, pool[2 * bs + 21:2 * bs + 91], old_sub=small.sub, want_sub=True)
        ap.check_equals_encode(torch, codec, oracle, pool[:2 * bs + 91], bs, r3, ("small append", rep))


# ---- 7. batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [False, True], ids=["index", "sub_index"])
def test_batch_items_across_group_edges(torch_mod, codec, oracle, sub):
    """70 items of 240 blocks: item i starts at block 240 i, inside one group, and ends in the next: dbatch_rebase_kernel's
    g - g0; 16 800 blocks: the batch's sums cross a pass"""
    torch = torch_mod
    bs, per, nitems = 64, 240 * 64, 70
    pool = pool_bytes()
    data = pool[:nitems * per]
    lens = [per] * nitems
    want, woffs = oracle.encode(data, bs, with_offsets=True)             # whole blocks: the items' streams back to back
    for rep in range(2):
        batch = codec.encode_batch(dev(torch, data), lens, bs, sub_index=sub)
        assert batch.nblocks == 240 * nitems and batch.stream_len == want.size
        assert np.array_equal(batch.stream.cpu().numpy(), want)
        assert np.array_equal(batch.offsets.cpu().numpy().astype(np.uint64), np.asarray(woffs, dtype=np.uint64))
        assert batch.item_offsets == [int(woffs[240 * i]) for i in range(nitems + 1)]
        short = 37
        oo = [5]
        for i in range(nitems):
            oo.append(oo[-1] + per + (13 if i != short else -1))
        out = torch.full((oo[-1] + 7,), GUARD, dtype=torch.uint8, device="cuda")
        _, errs, raws = codec.decode_batch(batch, out=out, out_offsets=oo)
        got = out.cpu().numpy()
        full = np.full(got.size, GUARD, np.uint8)
        for i in range(nitems):
            if i == short:                               # one byte short: this item alone fails, inside its slot
                assert errs[i] == MEMORY and raws[i] <= per - 1, (i, errs[i], raws[i])
                assert np.array_equal(got[oo[i]:oo[i] + raws[i]], data[i * per:i * per + raws[i]])
                full[oo[i]:oo[i + 1]] = got[oo[i]:oo[i + 1]]
                continue
            assert (errs[i], raws[i]) == (OK, per), (i, errs[i], raws[i])
            full[oo[i]:oo[i] + per] = data[i * per:(i + 1) * per]
        bad = np.flatnonzero(got != full)
        assert bad.size == 0, ("bytes differ at", bad[:8], "slots of", per + 13)
        # three items of three blocks, between the two
        tiny = codec.encode_batch(dev(torch, data[:9 * bs]), [3 * bs] * 3, bs, sub_index=sub)
        out3, errs3, raws3 = codec.decode_batch(tiny)
        assert errs3 == [0] * 3 and raws3 == [3 * bs] * 3 and np.array_equal(out3.cpu().numpy(), data[:9 * bs])


# ---- 8. damage, located late -------------------------------------------------------------------------------------------
def damaged_streams(inp):
    """name -> (stream, the blocks whose header is overwritten, (block, symbol) of a flipped payload bit or None)"""
    enc = inp.enc
    offs = inp.woffs.astype(np.int64)

    def tree_len_1025(st, b):
        st[int(offs[b]) + 8] = 1025 & 0xFF
        st[int(offs[b]) + 9] = 1025 >> 8

    out = {}
    for name, heads, flip in (("16390", [16390], None), ("700 and 16390", [700, 16390], None),
                              ("16390 and a bit of 16500", [16390], (16500, 17))):
        st = enc.stream.clone()
        for b in heads:
            assert not inp.one[b]
            tree_len_1025(st, b)
        if flip:
            b, sym = flip
            assert inp.one[b]                           # a one-symbol block: its payload bits must be 0
            st[int(offs[b]) + 20 + sym // 8] ^= 0x80 >> (sym % 8)
        out[name] = (st, heads, flip)
    return out


@pytest.mark.parametrize("name", ["16390", "700 and 16390", "16390 and a bit of 16500"])
def test_damage_behind_the_pass_edge(torch_mod, codec, oracle, name):
    """the first block whose header does not parse is a minimum over the groups (gmin): with the only bad block in group
    64 it comes from the second pass, with one in group 2 as well it must survive the second pass"""
    torch = torch_mod
    from libhuffman_amd.codec import HuffmanGpuError
    inp = gpu_input(torch, codec, oracle, "s64-16700")
    enc, bs, n, nb = inp.enc, inp.bs, inp.n, inp.nb
    st, heads, flip = damaged_streams(inp)[name]
    bad = enc.with_stream(st)
    first = min(heads)
    p = first * bs
    # the oracle, in order, on the same bytes
    oerr, oout, _ = oracle.decode(st.cpu().numpy(), n)
    assert oerr == OVERFLOW and oout.size == p and np.array_equal(oout, inp.data[:p])
    for kw in ({}, bad.sub_args()):
        for sync in (True, False, True):
            big, out = guarded(torch, n)
            with pytest.raises(HuffmanGpuError) as ei:
                codec.decode(bad.stream, bad.length, bad.offsets, nb, out, sync=sync, **kw)
                if not sync:
                    codec.decode_result()
            assert (ei.value.err, ei.value.raw) == (oerr, p), (name, sync, ei.value.err, ei.value.raw)
            assert np.array_equal(out[:p].cpu().numpy(), oout) and guards_intact(big, n), (name, sync)

    # decode_ranges: a range that ends in front of the first bad header is served, every other one fails with its error
    ranges = [(0, p), (p - 10, p), (5, 2 * bs + 3), (p, p), (p, p + 1), (p - 100, p + 100), (p + bs, p + 2 * bs), (0, n),
              (16390 * bs - 5, 16390 * bs), (16391 * bs, 16392 * bs), (n - 5, n), (16384 * bs - 3, 16384 * bs + 3)]
    oo = slots_for(ranges, n)
    for flag, sub in ((False, None), (False, "own"), (True, "own")):
        got, errs, raws = twice(lambda: rt.call(torch, codec, bad, ranges, oo, flag, sub_index=sub))
        fine = [i for i, (lo, hi) in enumerate(ranges) if min(hi, n) <= p]
        assert 3 in fine and len(fine) >= 4
        check_all_good(bad, ranges, got, errs, raws, oo, only=fine)
        for i, (lo, hi) in enumerate(ranges):
            if i in fine:
                continue
            delivered = max(0, p - lo)
            assert (errs[i], raws[i]) == (OVERFLOW, delivered), (name, flag, sub, i, ranges[i], errs[i], raws[i])
            assert np.array_equal(got[oo[i]:oo[i] + delivered], inp.data[lo:lo + delivered])
            assert np.all(got[oo[i] + delivered:oo[i + 1]] == GUARD), f"range {i}: bytes behind the delivered ones written"

    # gather: every record off the damage is served, a record on a damaged block or on the flipped bit is not
    ln = 16
    pos = [b * bs + (b * 37) % (bs - ln) for b in range(nb - 1)]
    hit = set(heads)
    if flip:
        pos[flip[0]] = flip[0] * bs + flip[1] - 3          # this record holds the damaged symbol
        pos[flip[0] + 1] = flip[0] * bs + flip[1] + 1      # this one starts behind it, in the same block
        hit.add(flip[0])
    got, errs, raws, stride = twice(lambda: gather(torch, codec, bad, pos, ln))
    check_guards(bad, got, pos, ln, stride)
    want = np.zeros(len(pos), np.int32)
    want[sorted(hit)] = RW
    assert np.array_equal(errs, want), (name, np.flatnonzero(errs != want)[:8])
    assert all(raws[i] == cut(bad, q, ln) for i, q in enumerate(pos))
    check_good(bad, got, errs, raws, pos, ln, stride, only=set(range(len(pos))) - hit)

    # find_bytes: the damaged blocks are not served and add nothing, every other block has its exact count and positions
    values = value_sets(inp.data)["half"] + [70]
    served = np.ones(nb, bool)
    served[sorted(hit)] = False
    m = find_model(inp.data, values, bs, n, served=served)
    cap = int(m[2][0]) + 9
    res = twice(lambda: find(torch, codec, bad, values, cap))
    assert np.array_equal(res[2] != OK, ~served), (name, np.flatnonzero((res[2] != OK) != ~served)[:8])
    assert set(res[2].tolist()) == {OK, RW}
    check(res, find_model(inp.data, values, bs, cap, served=served), cap, name)
    # and the context serves the good stream afterwards
    big, out = guarded(torch, n)
    assert codec.decode(enc.stream, enc.length, enc.offsets, nb, out, **enc.sub_args()) == n
    assert np.array_equal(out.cpu().numpy(), inp.data) and guards_intact(big, n)


# ---- 9. one long-lived context -----------------------------------------------------------------------------------------
def test_large_small_large_encode_and_decode(torch_mod, codec, oracle):
    """the encoder's and the decoders' sums after a call with 3 blocks between two with 16 700: entries of gprefix and
    local beyond the small call's are stale and must not be read (the other kinds of call: in their own tests above)"""
    torch = torch_mod
    big_in = cpu_input(oracle, "s64-16700")
    data3 = big_in.data[:2 * 64 + 21]
    want3, woffs3 = oracle.encode(data3, 64, with_offsets=True)
    for inp_data, want, woffs in ((big_in.data, big_in.want, big_in.woffs), (data3, want3, np.asarray(woffs3, dtype=np.uint64)),
                                  (big_in.data, big_in.want, big_in.woffs)):
        n = int(inp_data.size)
        nb = -(-n // 64)
        sub = codec.new_sub_index(n, 64)
        st, offs, length = codec.encode(dev(torch, inp_data), 64, sub_index=sub)
        assert length == want.size and np.array_equal(st.cpu().numpy(), want)
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), woffs)
        for kw in ({}, dict(sub_index=sub, raw_size=n, blocksize=64)):
            big, out = guarded(torch, n)
            assert codec.decode(st, length, offs, nb, out, **kw) == n
            assert np.array_equal(out.cpu().numpy(), inp_data) and guards_intact(big, n)
        big, out = guarded(torch, n)
        assert codec.decode_stream(st, length, length, out) == (0, n, length)
        assert np.array_equal(out.cpu().numpy(), inp_data) and guards_intact(big, n)

"""Every case of tests/decode_edge_cases.py - blocks on the thresholds of decode_regs.hpp and the raw-stream probe - through
every decode entry point, into outputs at odd byte offsets of a larger buffer filled with a pattern: what the oracle
delivers, and not a byte outside it touched.  Then the debug build's counters (-DDFAST_DEBUG) say that each case reached
the branch it is named for."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_edge_cases as dec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSETS = (0, 1, 3, 7, 13)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def codec(torch_mod):
    from libhuffman_amd.codec import GpuCodec
    c = GpuCodec(0)
    vp, u64 = C.c_void_p, C.c_uint64
    c.lib.hufgpu_decode_small.argtypes = [vp, vp, u64, u64, C.c_uint32, vp, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(oracle):
    return dec.cases(oracle)


def pattern(n: int) -> np.ndarray:
    return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)     # (not zeros: zeros are valid output)


class Guarded:
    """an output view at byte `off` of a larger buffer that holds a seeded pattern"""

    def __init__(self, torch, cap: int, off: int):
        self.off, self.cap = off, cap
        self.pat = pattern(cap + off + 67)
        self.big = torch.from_numpy(self.pat.copy()).cuda()
        self.view = self.big[off:off + cap]

    def check(self, got: int, want: np.ndarray | None, tag, touched: int | None = None):
        """the first `got` bytes of the view are `want`; nothing outside [off, off + touched) changed (touched = got)"""
        host = self.big.cpu().numpy()
        t = got if touched is None else touched
        if want is not None:
            assert np.array_equal(host[self.off:self.off + got], want), tag + ("bytes",)
        outside = np.concatenate([host[:self.off] != self.pat[:self.off], host[self.off + t:] != self.pat[self.off + t:]])
        assert not outside.any(), tag + ("guard bytes changed", int(np.count_nonzero(outside)))


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def small_decode(torch, codec, stream: np.ndarray, g: Guarded):
    h_in = torch.from_numpy(stream.copy()).pin_memory()
    d_in = torch.empty(stream.size, dtype=torch.uint8, device="cuda")
    h_out = torch.zeros(((g.cap + 7) & ~7) + 64, dtype=torch.uint8).pin_memory()
    raw, used = C.c_uint64(), C.c_uint64()
    err = codec.lib.hufgpu_decode_small(codec._ctx, h_in.data_ptr(), stream.size, stream.size, 1, d_in.data_ptr(), g.view.data_ptr(),
                                        g.cap, h_out.data_ptr(), h_out.numel(), C.byref(raw), C.byref(used))
    torch.cuda.synchronize()
    return err, int(raw.value), int(used.value), h_out[:raw.value].numpy().copy()


def intact(torch, codec, oracle, case, off):
    from libhuffman_amd.codec import HuffmanGpuError
    st, n = case.stream, case.syms.size
    s = dev(torch, st)
    offs = dev(torch, case.offsets.astype(np.int64))
    nb = len(case.parts)
    tag = (case.name, off)
    g = Guarded(torch, n, off)
    assert codec.decode(s, st.size, offs, nb, g.view, relaxed=True) == n, tag
    g.check(n, case.syms, tag + ("indexed",))
    assert codec.decode_counters()[0] == 0, tag + ("blocks the exact decoder took", codec.decode_counters())
    for sequential in (False, True):
        g = Guarded(torch, n, off)
        assert codec.decode_stream(s, st.size, st.size, g.view, relaxed=True, sequential=sequential) == (0, n, st.size), tag + (sequential,)
        g.check(n, case.syms, tag + ("raw", sequential))
    if st.size <= dec.SMALL_MAX:
        g = Guarded(torch, n, off)
        err, raw, used, host = small_decode(torch, codec, st, g)
        assert (err, raw, used) == (0, n, st.size) and np.array_equal(host, case.syms), tag + ("small",)
        g.check(n, case.syms, tag + ("small",))
    if case.encoded is not None:
        data, bs = case.encoded
        sub = codec.new_sub_index(n, bs)
        stream2, offs2, length2 = codec.encode(dev(torch, data), bs, sub_index=sub)
        assert np.array_equal(stream2.cpu().numpy(), st), tag + ("the encoder's stream",)
        g = Guarded(torch, n, off)
        assert codec.decode(stream2, length2, offs2, nb, g.view, sub_index=sub, raw_size=n, blocksize=bs) == n, tag
        g.check(n, case.syms, tag + ("sub",))
    # an output one byte short: the oracle's error and bytes, nothing written behind the output's end
    if off == 1:
        oerr, oout, _ = oracle.decode(st, n - 1, 1025)
        g = Guarded(torch, n - 1, off)
        err, raw, used = codec.decode_stream(s, st.size, st.size, g.view, relaxed=True)
        assert (err, raw) == (oerr, oout.size) == (1, oout.size), tag + ("short", err, raw, oerr, oout.size)
        g.check(raw, oout, tag + ("short",), touched=n - 1)
        g = Guarded(torch, n - 1, off)
        with pytest.raises(HuffmanGpuError) as ei:
            codec.decode(s, st.size, offs, nb, g.view, relaxed=True)
        assert ei.value.err == 1, tag
        g.check(0, None, tag + ("short indexed",), touched=n - 1)


def test_cases_through_every_entry_point_at_every_offset(torch_mod, codec, oracle, table):
    for case in table:
        for off in OFFSETS:
            intact(torch_mod, codec, oracle, case, off)


def indexed_want(oracle, case, bad):
    """(err, delivered, bytes): the block index fixes where every block lies, so each record decodes by itself; the first that
    fails ends the call after the symbols in front of it and the ones it delivered (test_gpu_subindex.py)"""
    offs = case.offsets
    got = []
    for i in range(len(case.parts)):
        rec = bad[int(offs[i]):int(offs[i + 1])]
        bl = int.from_bytes(rec[:8].tobytes(), "little")
        err, out, _ = oracle.decode(rec, bl + 64, 1025, length=1)
        got.append(out)
        if err:
            return err, np.concatenate(got)
    return 0, np.concatenate(got)


def test_damaged_cases_match_the_oracle_at_every_offset(torch_mod, codec, oracle, table):
    from libhuffman_amd.codec import HuffmanGpuError
    torch = torch_mod
    seen = set()
    for case in table:
        n = case.syms.size
        offs = dev(torch, case.offsets.astype(np.int64))
        for label, bad in dec.damaged(case):
            s = dev(torch, bad)
            oerr, oout, oused = oracle.decode(bad, n, 1025)
            ierr, iout = indexed_want(oracle, case, bad)
            seen.add(oerr)
            for off in OFFSETS:
                tag = (label, off)
                for sequential in (False, True):
                    g = Guarded(torch, n, off)
                    err, raw, used = codec.decode_stream(s, bad.size, bad.size, g.view, relaxed=True, sequential=sequential)
                    assert (err, raw) == (oerr, oout.size), tag + (sequential, (err, raw, used), (oerr, oout.size, oused))
                    if oerr == 0:
                        assert used == oused, tag + (sequential,)
                    g.check(raw, oout, tag + ("raw", sequential), touched=n if err else None)
                if bad.size <= dec.SMALL_MAX:
                    g = Guarded(torch, n, off)
                    err, raw, used, host = small_decode(torch, codec, bad, g)
                    assert (err, raw) == (oerr, oout.size) and np.array_equal(host, oout), tag + ("small", err, raw)
                    if oerr == 0:
                        assert used == oused, tag + ("small",)
                    g.check(raw, oout, tag + ("small",), touched=n if err else None)
                g = Guarded(torch, n, off)
                if ierr == 0:
                    assert codec.decode(s, bad.size, offs, len(case.parts), g.view, relaxed=True) == iout.size == n, tag
                    g.check(n, iout, tag + ("indexed",))
                else:
                    with pytest.raises(HuffmanGpuError) as ei:
                        codec.decode(s, bad.size, offs, len(case.parts), g.view, relaxed=True)
                    assert (ei.value.err, ei.value.raw) == (ierr, iout.size), tag + ("indexed", ei.value.err, ei.value.raw)
                    g.check(iout.size, iout, tag + ("indexed",), touched=n)
    assert 0 in seen and len(seen) >= 2, seen


@pytest.mark.parametrize("extra", [0, 1])
def test_blocks_at_dreg_max_block(torch_mod, codec, oracle, extra):
    """F: one block of 2^26 (+ 1) zipf symbols, the oracle's stream: the largest block decode_regs takes and the smallest it
    does not, with the block index alone, as a raw stream in parallel and in order"""
    from libhuffman_amd import datagen
    torch = torch_mod
    n = dec.DREG_MAX_BLOCK + extra
    data = datagen.zipf255(n, seed=26)
    st, o = oracle.encode(data, 0, with_offsets=True)
    assert o.size == 2 and dec.block_facts(st[:64 + 2 * 1025])["len"] == n
    s = dev(torch, st)
    offs = dev(torch, o.astype(np.int64))
    want = torch.from_numpy(data).cuda()
    for off in OFFSETS:
        pat = pattern(n + off + 67)
        big = torch.from_numpy(pat).cuda()
        pat_d = big.clone()
        view = big[off:off + n]
        entries = [("indexed", lambda: codec.decode(s, st.size, offs, 1, view, relaxed=True) == n),
                   ("raw", lambda: codec.decode_stream(s, st.size, st.size, view, relaxed=True) == (0, n, st.size))]
        if off in (0, 13):
            entries.append(("sequential", lambda: codec.decode_stream(s, st.size, st.size, view, relaxed=True, sequential=True) == (0, n, st.size)))
        for name, run in entries:
            big.copy_(pat_d)
            assert run(), (n, off, name)
            assert torch.equal(view, want), (n, off, name)
            assert torch.equal(big[:off], pat_d[:off]) and torch.equal(big[off + n:], pat_d[off + n:]), (n, off, name, "guard")


@pytest.mark.parametrize("kind", ["uniform256", "zipf255"])
def test_G_beyond_4_gib_of_64k_blocks(torch_mod, codec, oracle, kind):
    """G: streams of more than 4 GiB in 64 KiB blocks.  decode_regs.hpp takes such blocks with the block index alone and in the
    raw-stream probe, and clamps what it may read behind a payload (`readable`, the buffer resource's record count) to
    0xfffffe00 bytes: the first blocks here have more than that behind them.  A full round trip through both entry points,
    into an output at an odd offset of a buffer of random bytes, and a sample of blocks against the oracle's encoder."""
    torch = torch_mod
    bs = 65536
    n = (4 << 30) + (1 << 28) if kind == "uniform256" else (4 << 30) + (3 << 28)       # streams of about 4.9 and 4.5 GiB
    nb = n // bs
    data = torch.empty(n, dtype=torch.uint8, device="cuda")
    codec.fill(data, kind)
    stream, offs, length = codec.encode(data, bs)
    offs_h = offs.cpu().numpy().astype(np.uint64)
    assert length > (1 << 32) + (1 << 28) and length - int(offs_h[1]) > 0xfffffe00, length
    b4 = int(np.searchsorted(offs_h, 1 << 32))                      # the block that holds the stream's byte 2^32
    for b in (0, 1, 2, nb // 2, b4 - 1, b4, nb - 1):
        block = data[b * bs:(b + 1) * bs].cpu().numpy()
        got = stream[int(offs_h[b]):int(offs_h[b + 1])].cpu().numpy()
        assert np.array_equal(got, oracle.encode(block, bs)), (kind, b)
    off = 3
    big = torch.empty(n + off + 61, dtype=torch.uint8, device="cuda")
    view = big[off:off + n]
    for entry in ("indexed", "raw"):
        big.random_(0, 256)
        edges = (big[:off].clone(), big[off + n:].clone())
        if entry == "indexed":
            assert codec.decode(stream, length, offs, nb, view, relaxed=True) == n, kind
            assert codec.decode_counters()[0] == 0, (kind, codec.decode_counters())
        else:
            assert codec.decode_stream(stream, length, length, view, relaxed=True) == (0, n, length), kind
        assert torch.equal(view, data), (kind, entry)
        assert torch.equal(big[:off], edges[0]) and torch.equal(big[off + n:], edges[1]), (kind, entry, "guard bytes")
    del big, view, stream, data
    torch.cuda.empty_cache()


# ---- the branches, counted by the debug build -------------------------------------------------------------------------
CALLER = {"indexed": 0, "probe": 1, "chain": 2}


def branch_holds(want: str, c: list, caller: int) -> bool:
    """c = the debug counters 16..31 (decode_fast.hpp, DFAST_DBG_REGS_*)"""
    no_tables, ok, failed, long_ = c[4 * caller:4 * caller + 4]
    shrink, one_length = c[12:15], c[15]
    if isinstance(want, list):            # the outcomes exactly
        return c[4 * caller:4 * caller + 4] == want
    if want == "declined":
        return ok == 0 and failed == 0 and long_ == 0
    if failed or not ok:
        return False
    return {"taken": True, "table": long_ == 0, "long": long_ >= 1, "one_length": one_length >= 1,
            "shrink1": shrink[0] >= 1 and shrink[1] == 0 and shrink[2] == 0,
            "shrink2": shrink[1] >= 1 and shrink[2] == 0}[want]


def test_each_case_reaches_its_branch_in_the_debug_build(torch_mod):
    from test_gpu_pack_builds import build_variant
    lib = build_variant("dfast_debug", "-DDFAST_DEBUG")
    env = dict(os.environ, HUF_LIB_PATH=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "decode_edges_debug_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(rows) >= 30, r.stdout[-3000:]
    wrong = []
    for row in rows:
        assert row["equal"], row
        if not branch_holds(row["want"], row["counters"], CALLER[row["entry"]]):
            wrong.append(row)
    print("\n".join(json.dumps(x) for x in rows))
    assert not wrong, "\n".join(json.dumps(x) for x in wrong)
    names = {(x["case"], x["entry"]) for x in rows}
    for must in (("E_small_multi[1:]", "chain"), ("E_small_multi[3:]", "chain"), ("A_block_8191", "indexed"), ("A_block_8192", "indexed"), ("B_code33_K37", "indexed"), ("B_code32_K36", "indexed"),
                 ("C_burst_once", "indexed"), ("C_burst_twice", "indexed"), ("D_impostor_3_plus5", "probe"),
                 ("E_bar_3_9", "probe"), ("E_bar_4_1", "probe"), ("E_small_multi", "chain"), ("F_2^26", "indexed"), ("F_2^26+1", "indexed")):
        assert must in names, must

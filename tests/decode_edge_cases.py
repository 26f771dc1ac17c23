"""Named streams built to sit on the thresholds of the index-only and raw-stream decoders (kernels/decode_regs.hpp, and
decode_fast.hpp for what decode_regs declines).  Each case says what it claims about its blocks - block lengths, longest
code, bits a symbol, the one-length relation, where the bursts of short codes lie - and test_decode_edge_cases.py checks
every claim and the symbols against the oracle on the CPU; test_gpu_decode_edges.py runs the cases through every decode
entry point.  Test infrastructure (CPU, numpy).

Thresholds (decode_regs.hpp unless said otherwise):
  A  block_len >= DREG_MIN_BLOCK = 8 192 (decode_fast.hpp), outputs of blocks that start at odd offsets;
  B  codes of 13 to 32 bits through the LONG retry (binary search over K <= 256 leaves), 33 declined;
  C  a share of more than 64 codewords: the segment again with half the bits (shrink), once and twice;
  D  one-length mode: pay_bits - L * block_len < 8, true ones and impostors of mixed lengths;
  E  the raw-stream probe's bar of 192 bits a share (4 bits a symbol), and the small call's hint that overstates;
  F  DREG_MAX_BLOCK = 2^26 symbols (built by the oracle; test_gpu_decode_edges.py);
  H  A..E with one bit flipped in a long code, a burst or the last byte.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import handmade_streams as hm
from libhuffman_amd import datagen

DREG_MIN_BLOCK = 8192
DREG_MAX_BLOCK = 1 << 26
SMALL_MAX = 32768                       # streams hufgpu_decode_small is meant for (include/huffman_gpu.h)
RAW_PARALLEL_MIN = 65536                # a raw stream shorter than this goes to the in-order chain (decode_stream_general)


@dataclasses.dataclass
class Case:
    name: str
    parts: list                         # the blocks' bytes, in stream order
    syms: np.ndarray                    # what the stream decodes to
    claims: list                        # [(block number, {property: value})]: checked by block_facts()
    encoded: tuple | None = None        # (data, blocksize) when the stream is the encoder's (decode_sub applies)
    flips: list = dataclasses.field(default_factory=list)       # [(label, stream bit)] for the damaged copies (H)
    probe: tuple | None = None          # (blocks, {entry: expected branch}) for the debug build's child
    more_probes: list = dataclasses.field(default_factory=list)     # [(label, blocks, {entry: expected branch})] besides
    alone: int | None = None            # a block to be a case of its own as well: a stream small enough for hufgpu_decode_small

    @property
    def stream(self) -> np.ndarray:
        return np.concatenate([np.frombuffer(bytes(p), dtype=np.uint8) for p in self.parts])

    @property
    def offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum([len(p) for p in self.parts])]).astype(np.uint64)


# ---- facts of a block, read from its bytes alone -----------------------------------------------------------------------
def tree_code_lengths(ent: list) -> dict:
    """byte value -> code length for a serialised tree (preorder, -1 for a missing child; src/tree.c:138-227)"""
    out, i = {}, 0

    def rec(depth):
        nonlocal i
        v = ent[i]
        i += 1
        if v < 0:
            return
        if v < 256:
            out[v] = depth
            i += 2                      # its two -1
            return
        rec(depth + 1)
        rec(depth + 1)
    rec(0)
    return out


def block_facts(part) -> dict:
    b = bytes(part)
    n = int.from_bytes(b[:8], "little")
    tl = int.from_bytes(b[8:10], "little", signed=True)
    ent = list(np.frombuffer(b[10:10 + 2 * tl], dtype="<i2").astype(int))
    lens = tree_code_lengths(ent)
    pay_bits = 8 * (len(b) - 10 - 2 * tl)
    bps = pay_bits / n if n else 0.0
    L = int(bps + 0.001)
    return {"len": n, "tree_len": tl, "K": len(lens), "max_code": max(lens.values()), "code_len": lens,
            "encoder_shaped": ent[0] >= 256 and ent[-1] == -1 and min(lens.values()) >= 2,
            "pay_bits": pay_bits, "bps": bps, "one_length_rel": L if (2 <= L <= 12 and pay_bits - L * n < 8) else 0,
            "true_one_length": len(set(lens.values())) == 1}


# ---- builders -----------------------------------------------------------------------------------------------------------
def zipf_parts(oracle, n: int, bs: int, seed: int):
    """(blocks, data): ordinary zipf bytes as the encoder writes them"""
    data = datagen.zipf255(n, seed=seed)
    st, offs = oracle.encode(data, bs, with_offsets=True)
    return [st[int(offs[i]):int(offs[i + 1])] for i in range(offs.size - 1)], data


def filler(oracle, seed: int):
    """blocks below DREG_MIN_BLOCK (decode_fast.hpp's, never decode_regs'): enough of them that a raw stream is long enough
    for the parallel path, none of them near a threshold"""
    return zipf_parts(oracle, 24 * 3000, 3000, seed)


def lengths_chain(base_depth: int, lmax: int, K: int | None = None) -> list:
    """Code lengths (root bit included): a complete tree of 2^base_depth leaves under the root, one of which is replaced by a
    chain down to lmax (two leaves of lmax at its end); then, while fewer than K leaves, the deepest leaf shorter than lmax - 1
    is split in two."""
    L = [base_depth + 1] * (2 ** base_depth - 1) + list(range(base_depth + 2, lmax)) + [lmax, lmax]
    while K is not None and len(L) < K:
        cand = [x for x in L if x < lmax - 1]
        d = max(cand)
        L.remove(d)
        L += [d + 1, d + 1]
    return sorted(L)


def values_for(K: int, rng) -> list:
    return [int(v) for v in rng.permutation(256)[:K]]


def picks_geometric(rng, lengths, n: int, clip: int = 14) -> np.ndarray:
    p = np.array([2.0 ** -min(L, clip) for L in lengths])
    return rng.choice(len(lengths), size=n, p=p / p.sum())


def place(pick, at, leaf):
    for i in at:
        pick[i] = leaf
    return pick


def join(*pieces):
    """pieces: (blocks, symbols[, flips in block-relative terms]) -> (parts, syms, the first block number of every piece)"""
    parts, syms, firsts = [], [], []
    for pc in pieces:
        firsts.append(len(parts))
        parts += list(pc[0])
        syms.append(np.asarray(pc[1], dtype=np.uint8))
    return parts, np.concatenate(syms), firsts


def bit_of(parts, block: int, payload_bit: int, pay_at: int) -> int:
    return 8 * (sum(len(p) for p in parts[:block]) + pay_at) + payload_bit


# ---- the table ----------------------------------------------------------------------------------------------------------
def cases(oracle) -> list:
    out = []
    rng = np.random.default_rng(20261015)
    fz, fd = filler(oracle, 41)

    # A. block lengths at DREG_MIN_BLOCK, the encoder's blocks, blocksizes that are not multiples of 4 (odd output starts)
    for bs in (8191, 8192, 8193):
        n = 10 * bs + 1000                                           # ten blocks of bs (a raw stream for the parallel path) and a short one
        blocks, data = zipf_parts(oracle, n, bs, seed=bs)
        one, _ = zipf_parts(oracle, bs, bs, seed=bs)
        out.append(Case(f"A_block_{bs}", blocks, data, [(0, {"len": bs}), (10, {"len": 1000})], encoded=(data, bs),
                        flips=[("last_byte", 8 * sum(len(p) for p in blocks) - 8)],
                        probe=(one + fz, {"indexed": "declined" if bs < DREG_MIN_BLOCK else "taken"})))
    for bs in (65537, 98305):
        n = 3 * bs + 4099
        blocks, data = zipf_parts(oracle, n, bs, seed=bs)
        out.append(Case(f"A_encoder_bs{bs}", blocks, data, [(1, {"len": bs}), (3, {"len": 4099})], encoded=(data, bs),
                        flips=[("last_byte", 8 * sum(len(p) for p in blocks) - 8)]))

    # B. the longest code: 12 (table), 13 (LONG), 31, 32 (LONG), 33 (declined); K = 33..40 and K = 256
    for lmax, K in ((12, None), (13, None), (31, 36), (32, 36), (32, 40), (33, 37), (32, 256), (33, 256)):
        lengths = lengths_chain(3, lmax, K)
        vals = values_for(len(lengths), rng)
        n = 20000
        pick = picks_geometric(rng, lengths, n)
        deep = len(lengths) - 1                                      # a leaf of lmax bits
        pick = place(pick, [0, n - 1] + list(range(5, n - 5, 61)), deep)
        blk, syms, info = hm.encoder_block(lengths, vals, pick, pad_ones=bool(lmax & 1))
        parts, allsyms, firsts = join(([blk], syms), (fz, fd))
        at = info["starts"][n - 1] + info["lens"][n - 1] // 2        # inside the last long code
        flips = [("long_code", bit_of(parts, 0, int(at), info["pay_at"])), ("last_byte", 8 * len(blk) - 8)]
        branch = "long" if 12 < lmax <= 32 else "table" if lmax <= 12 else "declined"
        out.append(Case(f"B_code{lmax}_K{len(lengths)}", parts, allsyms,
                        [(0, {"max_code": lmax, "K": len(lengths), "len": n, "first_last_max": True, "bps_ge": 4.0})],
                        flips=flips, probe=([blk] + fz, {"indexed": branch, "probe": branch}), alone=0))

    # C. share overflow: codes of 10 and 11 bits with bursts of 2-bit codewords (a block of 24 000 such symbols: under 32 KiB)
    lengths = [2, 3, 4, 5, 6, 7] + [10] * 4 + [11] * 8              # (the short ones but 2 bits are not used)
    assert sum(2.0 ** -(L - 1) for L in lengths) == 1.0, lengths
    vals = values_for(len(lengths), rng)
    short = lengths.index(2)
    mids = [k for k, L in enumerate(lengths) if 10 <= L <= 11]
    for name, shape in (("C_burst_once", "mixed"), ("C_burst_twice", "pure"), ("C_burst_at_end", "end")):
        n = 24000
        pick = rng.choice(mids, size=n)
        if shape == "mixed":                                         # 5 two-bit codewords a 10-11-bit one, 3.4 bits a codeword: more than 64
            a, cnt = 7001, 400                                       # in the block's shares of 246 bits, at most 64 in 192
            pick[a:a + cnt] = short
            pick[a + 5:a + cnt:6] = rng.choice(mids, size=len(range(a + 5, a + cnt, 6)))
            claim = {"burst": (a, cnt, "mixed")}
        elif shape == "pure":                                        # 300 two-bit codewords in a row (600 bits), twice
            a, cnt = 9000, 300
            pick[a:a + cnt] = short
            pick[17000:17000 + cnt] = short
            claim = {"burst": (a, cnt, "pure")}
        else:
            a, cnt = n - 260, 260
            pick[a:] = short
            claim = {"burst": (a, cnt, "pure")}
        blk, syms, info = hm.encoder_block(lengths, vals, pick)
        parts, allsyms, _ = join(([blk], syms), (fz, fd))
        flips = [("burst", bit_of(parts, 0, int(info["starts"][a + cnt // 2]), info["pay_at"])), ("last_byte", 8 * len(blk) - 8)]
        want = {"mixed": "shrink1", "pure": "shrink2", "end": "shrink2"}[shape]
        out.append(Case(name, parts, allsyms, [(0, dict(claim, len=n, max_code=11))], flips=flips,
                        probe=([blk] + fz, {"indexed": want}), alone=0))

    # D. one length: true ones (every code L bits: 2^(L-1) leaves, so L <= 9 with 256 byte values) ...
    for L in range(2, 10):
        K = 2 ** (L - 1)
        lengths = [L] * K
        vals = values_for(K, rng)
        n = 12000 + int(rng.integers(0, 8))
        pick = rng.integers(0, K, size=n)
        blk, syms, info = hm.encoder_block(lengths, vals, pick, pad_ones=bool(L & 1))
        parts, allsyms, _ = join((fz[:12], fd[:12 * 3000]), ([blk], syms), (fz[12:], fd[12 * 3000:]))
        b = 12
        flips = [("last_byte", bit_of(parts, b, info["nbits"] - 1, info["pay_at"]))]
        out.append(Case(f"D_one_length_{L}", parts, allsyms, [(b, {"true_one_length": True, "one_length_rel": L, "len": n})],
                        flips=flips, probe=([blk] + fz, {"indexed": "one_length", "probe": "one_length"}), alone=b))
    # ... and impostors: mixed lengths whose padded payload is L * block_len + 0..7 bits
    for L, extra in ((2, 6), (2, 1), (3, 0), (3, 5), (9, 0), (9, 7), (12, 3)):
        if L == 2:
            lengths = [2, 3, 3]                                      # all 2-bit codes but `extra` 3-bit ones
        elif L == 12:
            lengths = list(range(2, 11)) + [11, 12, 13, 13]         # (the short ones but 11 bits are not used)
        else:
            lengths = [L - 1] + [L] * (2 ** (L - 1) - 3) + [L + 1] * 2
        assert sum(2.0 ** -(x - 1) for x in lengths) == 1.0, (L, lengths)
        vals = values_for(len(lengths), rng)
        at_L = [k for k, x in enumerate(lengths) if x == L]
        lo_k = [k for k, x in enumerate(lengths) if x == L - 1]
        hi_k = [k for k, x in enumerate(lengths) if x == L + 1]
        for n in range(12000, 12016):                                # (L * n) mod 8 + extra <= 8: the padding keeps it under L*n + 8
            if (L * n) % 8 == 0 and extra == 0 or (L * n) % 8 != 0 and (L * n) % 8 + extra <= 8:
                break
        pick = rng.choice(at_L, size=n)
        pairs = 0 if L == 2 else 600                                 # a shorter and a longer codeword: 2L bits in two
        slots = rng.permutation(n)
        if pairs:
            pick[slots[:pairs]] = rng.choice(lo_k, size=pairs)
            pick[slots[pairs:2 * pairs]] = rng.choice(hi_k, size=pairs)
        pick[slots[2 * pairs:2 * pairs + extra]] = rng.choice(hi_k, size=extra)      # one bit more each
        blk, syms, info = hm.encoder_block(lengths, vals, pick, pad_ones=True)
        assert info["nbits"] == L * n + extra
        parts, allsyms, _ = join(([blk], syms), (fz, fd))
        long_at = int(np.nonzero(info["lens"] > L)[0][-1])
        flips = [("long_code", bit_of(parts, 0, int(info["starts"][long_at]), info["pay_at"])), ("last_byte", 8 * len(blk) - 8)]
        out.append(Case(f"D_impostor_{L}_plus{extra}", parts, allsyms,
                        [(0, {"true_one_length": False, "one_length_rel": L, "len": n, "nbits": L * n + extra})],
                        flips=flips, probe=([blk] + fz, {"indexed": "one_length", "probe": "one_length"}), alone=0))

    # E. the probe's bar (4 bits a symbol) in a raw stream, and a small stream of several blocks through hufgpu_decode_small
    lengths = [3, 4, 4, 4, 4, 4, 5, 5]
    vals = values_for(8, rng)
    for name, p3, p5, want in (("E_bar_3_9", 0.2, 0.1, "declined"), ("E_bar_4_1", 0.1, 0.2, "taken")):
        n = 30000
        pk = rng.choice(8, size=n, p=[p3] + [(1 - p3 - p5) / 5] * 5 + [p5 / 2] * 2)
        blk, syms, info = hm.encoder_block(lengths, vals, pk)
        parts, allsyms, _ = join(([blk], syms), (fz, fd))
        bps = info["nbits"] / n
        out.append(Case(name, parts, allsyms, [(0, {"bps_lt" if want == "declined" else "bps_ge": 4.0, "len": n,
                                                    "one_length_rel": 0})],
                        flips=[("last_byte", 8 * len(blk) - 8)], probe=([blk] + fz, {"probe": want, "indexed": "taken"}), alone=0))
        assert 3.85 < bps < 4.15, bps
    # a small stream: three blocks of 2-3 bits a symbol, then one of 9 bits (its hint, "the rest of the stream", overstates
    # every payload but the last)
    pieces = []
    for i, (ls, n) in enumerate((([2, 3, 4, 4], 8192), ([2, 3, 4, 5, 5], 9000), ([3, 3, 3, 3], 8300))):
        v = values_for(len(ls), rng)
        pk = picks_geometric(rng, ls, n)
        blk, syms, _ = hm.encoder_block(ls, v, pk, pad_ones=bool(i & 1))
        pieces.append(([blk], syms))
    blk9, syms9, info9 = hm.encoder_block([9] * 256, values_for(256, rng), rng.integers(0, 256, size=8200))
    pieces.append(([blk9], syms9))
    parts, allsyms, _ = join(*pieces)
    out.append(Case("E_small_multi", parts, allsyms,
                    [(0, {"len": 8192, "bps_lt": 3.0}), (1, {"len": 9000, "bps_lt": 3.0}), (2, {"true_one_length": True, "one_length_rel": 3}),
                     (3, {"true_one_length": True, "one_length_rel": 9}), (-1, {"stream_le": SMALL_MAX})],
                    flips=[("last_byte", 8 * sum(len(p) for p in parts) - 1), ("payload", bit_of(parts, 1, 100, 10 + 2 * 21))],
                    probe=(parts, {"chain": SMALL_MULTI_CHAIN[0]}),
                    more_probes=[(f"E_small_multi[{i}:]", parts[i:], {"chain": SMALL_MULTI_CHAIN[i]}) for i in range(1, 4)]))
    return out + [alone_copy(c) for c in out if c.alone is not None]


# E_small_multi through hufgpu_decode_small, the stream from block i on: decode_regs' outcomes in the in-order chain
# (DREG_NO_TABLES, DREG_OK, DREG_FAILED, LONG retried) - the difference of two rows is block i's.  As the kernels stand,
# block 1 (9 000 symbols of 2 to 5 bits, its hint "the rest of the stream" six times its payload) is not vouched for by
# decode_regs - its round loop gives up after DREG_MAX_ROUNDS (debug counter 1) - and goes on to the exact decoder
# (decode_chain_lean_kernel: what it delivers is checked elsewhere); blocks 0,
# 2 (one length, not recognised as such under the overstated hint) and 3 (one length, the stream's last: its hint is exact)
# are taken.  A change in any of these outcomes is a change of the path, to be looked at.
SMALL_MULTI_CHAIN = {0: [0, 3, 1, 0], 1: [0, 2, 1, 0], 2: [0, 2, 0, 0], 3: [0, 1, 0, 0]}


def alone_copy(case: Case) -> Case:
    """the case's block `alone` as a stream of its own, with its claims and the flips that lie in it"""
    b = case.alone
    at = sum(len(p) for p in case.parts[:b])
    first = sum(block_facts(p)["len"] for p in case.parts[:b])
    n = block_facts(case.parts[b])["len"]
    flips = [(label, bit - 8 * at) for label, bit in case.flips if 0 <= bit - 8 * at < 8 * len(case.parts[b])]
    claims = [(0, cl) for blk, cl in case.claims if blk == b] + [(-1, {"stream_le": SMALL_MAX})]
    return Case(case.name + "_alone", [case.parts[b]], case.syms[first:first + n], claims, flips=flips)


def damaged(case: Case) -> list:
    """(label, stream) with one bit flipped, for every flip the case names"""
    res = []
    for label, bit in case.flips:
        s = case.stream.copy()
        s[bit >> 3] ^= 0x80 >> (bit & 7)
        res.append((f"{case.name}/{label}", s))
    return res


def check_claims(case: Case):
    """every claim of the case holds for the bytes of its blocks"""
    for b, claim in case.claims:
        if b == -1:
            if "stream_le" in claim:
                assert case.stream.size <= claim["stream_le"], (case.name, case.stream.size)
            continue
        f = block_facts(case.parts[b])
        start = sum(block_facts(p)["len"] for p in case.parts[:b])
        syms = case.syms[start:start + f["len"]]
        for key, want in claim.items():
            tag = (case.name, b, key, want)
            if key in ("len", "max_code", "K", "true_one_length", "one_length_rel"):
                assert f[key] == want, tag + (f[key],)
            elif key == "bps_ge":
                assert f["bps"] >= want, tag + (f["bps"],)
            elif key == "bps_lt":
                assert f["bps"] < want, tag + (f["bps"],)
            elif key == "nbits":
                assert f["pay_bits"] - 8 < want <= f["pay_bits"], tag + (f["pay_bits"],)
            elif key == "first_last_max":
                cl = f["code_len"]
                assert cl[int(syms[0])] == cl[int(syms[-1])] == f["max_code"], tag
            elif key == "burst":
                a, cnt, shape = want
                cl = np.array([f["code_len"].get(v, 0) for v in range(256)])[syms[a:a + cnt]]
                if shape == "pure":
                    assert (cl == 2).all(), tag
                else:
                    assert (cl == 2).sum() >= 4 * cnt // 5 and (cl >= 10).sum() >= cnt // 6 - 1, tag
            else:
                raise AssertionError(("unknown claim", key))

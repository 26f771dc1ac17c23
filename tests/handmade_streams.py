"""Blocks no encoder wrote: random trees (any shape src/tree.c:138-227 deserializes, with or without the encoder's root
that has a left child only), random symbols coded with them.  The reference's decoder (src/decoder.c:34-96) walks whatever
tree a stream brings, so its restatement in oracle/ says what every such stream decodes to; the tests compare the HIP
decoders with it.  Test infrastructure (CPU, numpy)."""
from __future__ import annotations

import struct

import numpy as np


def random_tree(rng, leaves: int, skew: float):
    """nested tuples: a leaf is its byte value, a node (left, right); skew = how often a node keeps ONE leaf on a side"""
    syms = [int(x) for x in rng.choice(256, size=leaves, replace=False)]

    def build(items):
        if len(items) == 1:
            return items[0]
        if rng.random() < skew:
            k = 1 if rng.random() < 0.5 else len(items) - 1
        else:
            k = int(rng.integers(1, len(items)))
        return (build(items[:k]), build(items[k:]))
    return build(syms)


def serialize(tree, wrap: bool) -> list:
    """preorder entries as src/tree.c writes them: an index per node (>= 256 for inner nodes), -1 where a child is missing"""
    out, counter = [], [256]

    def rec(t):
        if isinstance(t, int):
            out.extend([t, -1, -1])
        else:
            out.append(counter[0])
            counter[0] += 1
            rec(t[0])
            rec(t[1])
    if wrap:
        out.append(counter[0])
        counter[0] += 1
        rec(tree)
        out.append(-1)
    else:
        rec(tree)
    return out


def codes(tree, wrap: bool) -> dict:
    """byte value -> list of bits"""
    table = {}

    def rec(t, prefix):
        if isinstance(t, int):
            table[t] = prefix
        else:
            rec(t[0], prefix + [0])
            rec(t[1], prefix + [1])
    rec(tree, [0] if wrap else [])
    return table


def block(rng, leaves: int, skew: float, wrap: bool, nsym: int, deep_often: bool = False, pad_ones: bool = False):
    """(bytes of the block, its symbols).  deep_often: every leaf equally likely (long codes all the time) instead of
    likely in proportion to 2^-depth."""
    tree = random_tree(rng, leaves, skew)
    table = codes(tree, wrap)
    keys = sorted(table)
    if deep_often:
        p = np.full(len(keys), 1.0 / len(keys))
    else:
        p = np.array([2.0 ** -min(len(table[k]), 40) for k in keys])
        p /= p.sum()
    pick = rng.choice(len(keys), size=nsym, p=p)
    syms = np.array(keys, dtype=np.uint8)[pick]
    payload = pack_payload([table[k] for k in keys], pick, pad_ones)[0]
    return header(nsym, serialize(tree, wrap)) + payload, syms, max(len(v) for v in table.values())


def header(nsym: int, ent: list) -> bytes:
    """block_len, tree_len and the tree's entries as src/encoder.c writes them"""
    return struct.pack("<Qh", nsym, len(ent)) + np.asarray(ent, dtype="<i2").tobytes()


def _handmade_block(payload: bytes, leaves: int) -> bytes:
    """A block whose tree is complete with 2 or 4 leaves ('A' = 0, 'B' = 1 / 'A'..'D' = 00..11): its payload is ANY byte
    string, one symbol a bit or two (src/decoder.c:34-96 walks whatever tree the stream brings)."""
    tree = [0x0101, 0x41, -1, -1, 0x42, -1, -1] if leaves == 2 else \
           [0x0103, 0x0101, 0x41, -1, -1, 0x42, -1, -1, 0x0102, 0x43, -1, -1, 0x44, -1, -1]
    per_byte = 8 if leaves == 2 else 4
    return struct.pack("<Qh", per_byte * len(payload), len(tree)) + b"".join(struct.pack("<h", v) for v in tree) + payload


def pack_payload(leaf_bits: list, pick: np.ndarray, pad_ones: bool = False, chunk: int = 1 << 20):
    """(payload bytes, bit count before padding): the codewords leaf_bits[pick[0]], leaf_bits[pick[1]] ... back to back,
    most significant bit first, the last byte filled with zeros or ones.  Codes of any length; numpy, a chunk of symbols at
    a time (a gather from the leaves' bits laid end to end)."""
    lens = np.array([len(b) for b in leaf_bits], dtype=np.int64)
    flat = np.array([x for b in leaf_bits for x in b], dtype=np.uint8)
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pick = np.asarray(pick, dtype=np.int64)
    parts = []
    for c0 in range(0, pick.size, chunk):
        k = pick[c0:c0 + chunk]
        L = lens[k]
        ends = np.cumsum(L)
        src = np.repeat(at[k] - (ends - L), L) + np.arange(int(ends[-1]) if ends.size else 0, dtype=np.int64)
        parts.append(flat[src])
    bits = np.concatenate(parts) if parts else np.empty(0, np.uint8)
    nbits = bits.size
    pad = (-nbits) % 8
    if pad:
        bits = np.concatenate([bits, np.full(pad, 1 if pad_ones else 0, dtype=np.uint8)])
    return np.packbits(bits).tobytes(), nbits


def encoder_tree(lengths, values):
    """The tree the encoder writes (a root with a left child only, above a full binary tree) whose leaf k has the code length
    lengths[k] - the root's 0 included, so 2 and more - and the byte values[k].  The lengths are a Kraft-complete multiset of the
    full tree below the root: sum 2^-(length - 1) == 1.  Codes are canonical: shorter first, ties in the order given."""
    lengths = [int(x) for x in lengths]
    assert len(lengths) == len(values) >= 2 and min(lengths) >= 2 and len(set(int(v) for v in values)) == len(values)
    assert sum(2.0 ** -(L - 1) for L in lengths) == 1.0, "not Kraft-complete"
    order = sorted(range(len(lengths)), key=lambda k: (lengths[k], k))
    trie: dict = {}
    code, prev = 0, lengths[order[0]] - 1
    for k in order:
        d = lengths[k] - 1
        code <<= d - prev
        prev = d
        node = trie
        for i in range(d - 1, 0, -1):
            node = node.setdefault((code >> i) & 1, {})
        node[code & 1] = int(values[k])
        code += 1

    def tup(t):
        return t if isinstance(t, int) else (tup(t[0]), tup(t[1]))
    return tup(trie)


def encoder_block(lengths, values, pick, pad_ones: bool = False):
    """(bytes of the block, its symbols, info) for the encoder-shaped tree of encoder_tree(lengths, values) and the symbol
    sequence of leaves `pick` (indices into lengths).  info: pay_at = the payload's first byte in the block, starts / lens =
    each symbol's first payload bit and code length, nbits = payload bits before the padding."""
    tree = encoder_tree(lengths, values)
    table = codes(tree, True)
    leaf_bits = [table[int(v)] for v in values]
    assert [len(b) for b in leaf_bits] == [int(x) for x in lengths]
    pick = np.asarray(pick, dtype=np.int64)
    payload, nbits = pack_payload(leaf_bits, pick, pad_ones)
    hdr = header(pick.size, serialize(tree, True))
    lens = np.asarray(lengths, dtype=np.int64)[pick]
    info = {"pay_at": len(hdr), "starts": np.cumsum(lens) - lens, "lens": lens, "nbits": nbits}
    return hdr + payload, np.asarray(values, dtype=np.uint8)[pick], info

"""Helpers that the GPU tests of the indexed routes share (tests/test_gpu_ranges.py, tests/test_gpu_range_tiles.py and, through
tests/find_support.py, the tests of the search family): the guard byte, an encoded input with what the tests know about it,
and the inputs whose trees reach each look-up path of the decoder.  Not a test module."""
import numpy as np

from libhuffman_amd import datagen

GUARD = 0xA5


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


class Enc:
    """an encoded input and what the tests know about it: P = where each block's bytes start in the raw data"""

    def __init__(self, torch, codec, data, bs, sub=False, stream=None, offsets=None, block_lens=None):
        self.data, self.bs, self.n = data, bs, int(data.size)
        self.sub = None
        if stream is None:
            self.sub = codec.new_sub_index(self.n, bs) if sub else None
            stream, offsets, _ = codec.encode(dev(torch, data), bs, sub_index=self.sub)
            nb = codec.block_count(self.n, bs)
            block_lens = [min(bs or self.n, self.n - b * (bs or self.n)) for b in range(nb)]
        self.stream, self.offsets = stream, offsets
        self.length = int(stream.numel())
        self.nb = len(block_lens)
        self.P = np.concatenate([[0], np.cumsum(block_lens)]).astype(np.int64)
        self.h_offs = offsets.cpu().numpy().astype(np.int64)

    def with_stream(self, stream):
        other = object.__new__(Enc)
        other.__dict__.update(self.__dict__)
        other.stream = stream
        return other

    def sub_args(self):
        return {} if self.sub is None else dict(sub_index=self.sub, raw_size=self.n, blocksize=self.bs)


# ---- ranges ----------------------------------------------------------------------------------------------------------------
TILE = 2048


def touched(enc, lo, hi):
    """first and last block of the cut range, None when it is empty"""
    lo_c, hi_c = min(lo, enc.n), min(hi, enc.n)
    if lo_c >= hi_c:
        return None
    fb = int(np.searchsorted(enc.P, lo_c, side="right")) - 1
    lb = int(np.searchsorted(enc.P, hi_c, side="left")) - 1
    return fb, lb


def ranges_route_model(enc, ranges, oo):
    """(direct, staged, tiles, items) the rule of include/huffman_gpu.h gives"""
    cover, pairs, whole = np.zeros(enc.nb, int), np.zeros(enc.nb, int), np.zeros(enc.nb, int)
    for i, (lo, hi) in enumerate(ranges):
        t = touched(enc, lo, hi)
        lo_c, hi_c = min(lo, enc.n), min(hi, enc.n)
        if t is None or oo[i + 1] - oo[i] < hi_c - lo_c:
            continue
        for b in range(t[0], t[1] + 1):
            p0, p1 = int(enc.P[b]), int(enc.P[b + 1])
            c0, c1 = max(lo_c, p0) - p0, min(hi_c, p1) - p0
            if c0 >= c1:
                continue
            cover[b] += 1
            pairs[b] += (c1 - 1) // TILE - c0 // TILE + 1
            whole[b] += c0 == 0 and c1 == p1 - p0
    direct = (cover == 1) & (whole == 1)
    rest = (cover > 0) & ~direct
    tiles = rest & enc.elig & (pairs <= (enc.block_lens + TILE - 1) // TILE)
    return int(direct.sum()), int((rest & ~tiles).sum()), int(tiles.sum()), int(pairs[tiles].sum())


# ---- inputs ------------------------------------------------------------------------------------------------------------
def by_counts(n, bs, counts, seed):
    """every block a permutation of the same multiset: value v counts[v] times (cut for a short last block)"""
    rng = np.random.default_rng(seed)
    block = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
    assert block.size == (bs or n), (block.size, bs, n)
    parts = [rng.permutation(block) for _ in range(0, n, block.size)]
    return np.concatenate(parts)[:n]


def halving(size):
    """counts size/2, size/4, ..., 1, 1: code lengths 2 .. log2(size) + 1 (the root's bit included)"""
    c = [size >> (k + 1) for k in range(size.bit_length() - 1)]
    return c + [1]


def fibonacci(size):
    """Fibonacci counts (the deepest trees a block of `size` bytes can have), the most frequent value takes the rest"""
    f = [1, 1]
    while sum(f) + f[-1] + f[-2] <= size // 2:
        f.append(f[-1] + f[-2])
    return f + [size - sum(f)]


def halving_for(n):
    """halving counts for a block of any size: powers of two from 2^14 down, the most frequent value takes the rest"""
    c = [1 << k for k in range(14, -1, -1)]
    return [n - sum(c)] + c


def make(kind, n, bs):
    if kind == "zipf255":
        return datagen.zipf255(n, seed=3)
    if kind == "two":                                   # two byte values: about one bit a symbol
        return (np.random.default_rng(5).integers(0, 2, n) * 200 + 7).astype(np.uint8)
    if kind == "l2":                                    # codes of 13 bits and more: the second-level table
        return by_counts(n, bs, halving(bs) if bs else halving_for(n), 7)
    if kind == "long":                                  # codes beyond 18 bits: the binary search over the leaves
        return by_counts(n, bs, fibonacci(bs) if bs else fibonacci(n), 8)
    if kind == "uniform256":
        return datagen.uniform256(n, seed=1)
    if kind == "const41":
        return datagen.const_bytes(n)
    raise ValueError(kind)


def max_code_len(enc):
    """the longest claimed code length of the sub-index (its last nblocks x 256 bytes are the lengths by byte value)"""
    b = enc.sub.cpu().numpy().view(np.uint8)
    nbytes = enc.codec.sub_index_bytes(enc.n, enc.bs)
    return int(b[nbytes - 256 * enc.nb:nbytes].max())

"""The CPU model of hufgpu_scatter (include/huffman_gpu.h): the records applied to a copy of the data, then the oracle's
encode of the result, its block index and the CPU reference's sub-index - the way tests/test_gpu_update.py gets its
expectation.  Not a test module.

A record is (position, length); len_i > max_len is the call's argument error and is refused here.  With `fill` the result
is defined whatever overlaps.  In source mode a byte that several records cover receives the byte of one of them, so the
model asserts that all records that cover a byte carry the same value for it - the only inputs with one right answer -
and then applies them in order.
"""
import numpy as np

import sub_index_ref as sref


def cut(pos, length, n):
    """the record cut at the end of the data: (start, bytes), bytes = 0 when nothing of it is written"""
    pos, length = int(pos), int(length)
    if pos >= n or length <= 0:
        return pos, 0
    return pos, min(length, n - pos)


def apply(data, positions, lengths, max_len, fill=None, slots=None):
    """D': `lengths` is None (every record max_len long), an int or a sequence; `slots` a [nrecords, >= max_len] array whose
    row i holds record i's new bytes"""
    assert (fill is None) != (slots is None), "exactly one of fill and slots"
    n = int(data.size)
    out = bytearray(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
    nrec = len(positions)
    if lengths is None or np.isscalar(lengths):
        lengths = [max_len if lengths is None else int(lengths)] * nrec
    assert len(lengths) == nrec
    written = np.zeros(n, bool)
    for i, (p, ln) in enumerate(zip(positions, lengths)):
        assert 0 <= int(ln) <= max_len, ("record longer than max_len", i, ln, max_len)
        p, k = cut(p, ln, n)
        if k == 0:
            continue
        if fill is not None:
            out[p:p + k] = bytes([fill]) * k
            continue
        new = np.asarray(slots[i][:k], np.uint8)
        seen = written[p:p + k]
        if seen.any():
            old = np.frombuffer(bytes(out[p:p + k]), np.uint8)
            assert np.array_equal(old[seen], new[seen]), ("overlapping records disagree", i)
        out[p:p + k] = new.tobytes()
        written[p:p + k] = True
    return np.frombuffer(bytes(out), np.uint8).copy()


def touched_blocks(n, bs, positions, lengths, max_len):
    """the distinct blocks of the layout that a record has bytes in (records longer than max_len write nothing)"""
    bs = bs or n
    nrec = len(positions)
    if lengths is None or np.isscalar(lengths):
        lengths = [max_len if lengths is None else int(lengths)] * nrec
    hit = set()
    for p, ln in zip(positions, lengths):
        if int(ln) > max_len:
            continue
        p, k = cut(p, ln, n)
        if k:
            hit.update(range(p // bs, (p + k - 1) // bs + 1))
    return sorted(hit)


def touched_bound(nblocks, bs, nrecords, max_len):
    """hufgpu_scatter_touched_bound's formula"""
    if nblocks == 0 or nrecords == 0:
        return 0
    if bs == 0:
        return 1
    per = (max_len + bs - 2) // bs + 1 if max_len else 1
    return min(nblocks, nrecords * per)


class Expected:
    """the oracle's encode of D' in blocks of bs, its index, and the sub-index entries the encoder writes"""

    def __init__(self, oracle, new, bs):
        self.new, self.bs = new, bs
        stream, offs = oracle.encode(new, bs, with_offsets=True)
        self.stream, self.offs = np.asarray(stream, np.uint8), np.asarray(offs).astype(np.uint64)
        self.length = int(self.stream.size)

    def sub(self):
        return sref.expected(self.stream, self.offs, self.new, self.bs or int(self.new.size))

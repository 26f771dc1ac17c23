"""The block discovery of a raw stream (libhuffman_amd/csrc/kernels/discover.hpp) restated on the CPU: which offsets
discover_kernel takes for candidate headers, and the chain of blocks that walk_kernel validates from offset 0.  numpy and
the oracle, no GPU.  Test infrastructure.

The strict test is the KERNEL's, not the reference decoder's: src/decoder.c also takes a block_len of 2^32 and more, a
tree_len of 0, and entries behind a complete tree; discover_kernel rejects all three on purpose (such a header ends the
validated prefix, and the in-order decoder takes over there), and so does this model.

The geometry is read out of the sources, so that a change of it moves the tests' positions with it."""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libhuffman_amd", "csrc")


def _text(*path) -> str:
    with open(os.path.join(CSRC, *path)) as f:
        return f.read()


def _define(text: str, name: str) -> int:
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)u?\b", text, re.M)
    assert m, name + " is no longer a plain #define"
    return int(m.group(1))


def _threshold(text: str, pattern: str) -> int:
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


_DISCOVER, _STREAM = _text("kernels", "discover.hpp"), _text("host", "stream.hpp")
DISC_THREADS = _define(_DISCOVER, "DISC_THREADS")
DISC_PER = _define(_DISCOVER, "DISC_PER")
DISC_ITERS = _define(_DISCOVER, "DISC_ITERS")
DISC_SLOTS = _define(_DISCOVER, "DISC_SLOTS")
DISC_SCAN_GROUP = _define(_DISCOVER, "DISC_SCAN_GROUP")
WALK_CHUNK = _define(_DISCOVER, "WALK_CHUNK")
INDEX_MIN = _threshold(_STREAM, r"if \(scan_len < (\d+)\) return HUFE_OK;")          # hufgpu_block_index: below it nothing is looked for
PARALLEL_MIN = _threshold(_STREAM, r"scan_len >= (\d+) && !\(flags & HUFGPU_SEQUENTIAL\)")   # hufgpu_decode_stream: the discovery from here on

PIECE = DISC_PER                         # bytes a thread owns of a row
WAVE = 64 * DISC_PER                     # bytes a wavefront owns of a row; its lane 63 alone loads the piece behind its own
ROW = DISC_THREADS * DISC_PER            # bytes of a row
WORKGROUP = ROW * DISC_ITERS             # bytes a workgroup scans
SCAN_GROUP = WORKGROUP * DISC_SCAN_GROUP   # bytes whose workgroups' counts one workgroup of scan_counts_kernel sums
HEADER_FIXED = 10                        # block_len (8) and tree_len (2)


def grammar_complete(entries: np.ndarray) -> bool:
    """tree_grammar_complete: the int16 entries are a preorder tree that ends with the last of them - every entry but -1
    opens a child slot more than it fills, -1 fills one, and no entry stands behind a complete tree"""
    d = np.where(entries != -1, 1, -1).astype(np.int64)
    before = 1 + np.cumsum(d) - d
    return bool((before > 0).all() and 1 + int(d.sum()) == 0)


def strict_header(stream: np.ndarray, p: int, avail: int, max_tree: int) -> bool:
    """discover_kernel's test of offset p"""
    if avail - p < HEADER_FIXED:
        return False
    block_len = int.from_bytes(stream[p:p + 8].tobytes(), "little")
    tree_len = int.from_bytes(stream[p + 8:p + 10].tobytes(), "little", signed=True)
    if not 0 < block_len < 1 << 32 or not 1 <= tree_len <= max_tree:
        return False
    header_end = p + HEADER_FIXED + 2 * tree_len
    if header_end > avail or block_len > 8 * (avail - header_end):
        return False
    return grammar_complete(np.frombuffer(stream[p + HEADER_FIXED:header_end].tobytes(), "<i2"))


def candidates(stream: np.ndarray, avail: int, scan_len: int, max_tree: int) -> list:
    """every offset below scan_len that passes the strict test, ascending"""
    n = min(scan_len, avail - HEADER_FIXED + 1)
    if n <= 0:
        return []
    zero = stream[:avail] == 0
    maybe = zero[4:n + 4] & zero[5:n + 5] & zero[6:n + 6] & zero[7:n + 7]          # the upper half of block_len
    maybe &= ~(zero[0:n] & zero[1:n + 1] & zero[2:n + 2] & zero[3:n + 3])           # block_len != 0
    return [int(p) for p in np.flatnonzero(maybe) if strict_header(stream, int(p), avail, max_tree)]


def chain(oracle, stream: np.ndarray, avail: int, length: int, max_tree: int):
    """(index, nblocks, consumed, complete) as walk_kernel defines them and hufgpu_block_index returns them: index = the
    header offsets of the blocks validated from offset 0 on and the offset behind them (empty when there is none)"""
    scan_len = min(length, avail)
    index, p, complete = [], 0, False
    while p < scan_len and strict_header(stream, p, avail, max_tree):
        block_len = int.from_bytes(stream[p:p + 8].tobytes(), "little")
        err, _, used = oracle.decode(stream[p:avail], block_len + 64, max_tree, length=1)
        if err:
            break                                    # LINK_BAD: the walk stops in front of the block
        index.append(p)
        p += used
        if p >= length:                              # LINK_TERMINAL, src/decoder.c:218
            complete = True
            break
    if not index:
        return [], 0, 0, False
    return index + [p], len(index), p, complete

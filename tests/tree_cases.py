"""Named histograms built to sit on the branches of the encoder's round-wise tree build (csrc/kernels/tree.hpp,
tree_fast_wave): equal counts at every register layout, tied node sums, `sel` below, at and above the threshold of a
sorted round for every register count, a round of more than 64 pairs that stays on four registers, the degenerate blocks
and the deepest trees a block below 4 MiB can have.  A case is a name plus a 256-entry histogram; its block is np.repeat of
the histogram, shuffled with a seed fixed per case.  tests/tree_rounds_ref.py walks the kernel on the histogram,
test_tree_rounds_ref.py checks that walk against the oracle on the CPU, test_gpu_tree_cases.py runs the blocks through every
encode route that builds a tree.  Test infrastructure (CPU, numpy)."""
from __future__ import annotations

import dataclasses
import zlib

import numpy as np

EQUAL_K = (2, 3, 4, 5, 63, 64, 65, 66, 127, 128, 129, 130, 200, 255, 256)
LARGE_FROM = 1 << 20                    # blocks from here on are the "large" cases: encoded with blocksize 0 and 1 << 22 only
FUSED_BELOW = 32768                     # HL_MIN_BLOCK: shorter blocks take the fused hist_tree_kernel


def fused_bs(n: int) -> int:
    """the blocksize of the fused route for a block of n bytes: 4096, or the block's length rounded up when larger
    (the route holds the block when this is below FUSED_BELOW)"""
    return max(4096, -(-n // 4096) * 4096)


def lanes_bs(n: int) -> int:
    """... of the route with lane-private counts and tree_wave_kernel"""
    return 65536 if n <= 65536 else 262144


@dataclasses.dataclass
class Case:
    name: str
    hist: np.ndarray                    # 256 counts
    first: tuple | None = None          # (R on entry, sel, round_min) of the first decision, where the case is built for one

    @property
    def n(self) -> int:
        return int(self.hist.sum())

    @property
    def large(self) -> bool:
        return self.n >= LARGE_FROM

    def data(self) -> np.ndarray:
        d = np.repeat(np.arange(256, dtype=np.uint8), self.hist)
        np.random.default_rng(zlib.crc32(self.name.encode())).shuffle(d)
        return d


def _hist(counts, values=None) -> np.ndarray:
    """counts[i] for byte value values[i] (default: byte i)"""
    h = np.zeros(256, dtype=np.int64)
    counts = [int(c) for c in counts]
    values = range(len(counts)) if values is None else values
    for v, c in zip(values, counts):
        assert 0 <= v < 256 and h[v] == 0 and c > 0
        h[v] = c
    return h


def fib(k: int) -> list:
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def cases() -> list:
    out = []

    def add(name, h, first=None):
        assert len(h) == 256 and not any(c.name == name for c in out)
        out.append(Case(name, np.asarray(h, dtype=np.int64), first))

    # equal counts: every key ties with every other; low byte values and high ones (slot -> lane / register and the
    # compaction's ballots differ), single occurrences and a thousand each
    for count in (1, 1000):
        for k in EQUAL_K:
            add(f"equal_{k}x{count}_low", _hist([count] * k))
            add(f"equal_{k}x{count}_high", _hist([count] * k, [255 - i for i in range(k)]))

    # tied node sums
    add("ties_half_ones_half_twos", _hist([1] * 128 + [2] * 128))
    add("ties_pow2_mod6", _hist([1 << (i % 6) for i in range(256)]))
    add("ties_mod3", _hist([1 + i % 3 for i in range(256)]))
    add("ties_staircase", _hist([1 + i // 2 for i in range(256)]))
    add("ties_ramp", _hist([1 + i for i in range(256)]))
    add("ties_ramp_reversed", _hist([256 - i for i in range(256)]))
    head = fib(18)                                              # 1 .. 2584
    add("ties_fib_head_100_ones", _hist(head + [1] * 100))
    add("ties_fib_head_232_ones", _hist(head + [1] * 232))
    rng = np.random.default_rng(150)
    add("ties_random_1to4_150", _hist(rng.integers(1, 5, 150), rng.choice(256, 150, replace=False)))

    # sel below, at and above round_min: m ones (a + b = 2, so sel = m exactly) and a rest that rises from 2
    for R, live, ms in ((1, 9, (3, 4, 5)), (2, 80, (7, 8, 9)), (4, 200, (15, 16, 17))):
        for m in ms:
            add(f"sel_R{R}_m{m}", _hist([1] * m + [2 + i for i in range(live - m)]), first=(R, m, 4 * R))

    # more than 64 pairs in a round that leaves more than 128 keys: the nodes sorted in two registers, then the merge on four
    add("pairs65_stays_R4", _hist([1] * 130 + [260 + i for i in range(126)]))
    # four registers on entry, single merges down to 128 keys or fewer, then a round that leaves 64: 4 -> 1
    add("R4_to_R1", _hist([1, 2, 3] + [100] * 126))

    # degenerate
    add("one_value", _hist([100], [7]))
    add("two_values_1_1", _hist([1, 1], [3, 200]))
    add("two_values_1_4194302", _hist([1, 4194302], [250, 9]))          # the largest key the 32-bit tree sees
    add("all_256_one_dominant", _hist([1000] + [1] * 255))              # tree_len 1025

    # depth: Fibonacci counts, depth k with the wrap root
    for k in (29, 30, 31):
        add(f"depth_fib{k}", _hist(fib(k)))
    f31 = fib(31)
    add("depth_fib31_4194303", _hist(f31[:-1] + [f31[-1] + 4194303 - sum(f31)]))
    # ... the deepest leaves in different lanes, registers j = 0 and 3 (byte = lane + 64 j)
    spread = [5, 232] + [v for v in ((i * 37 + 11) % 256 for i in range(256)) if v not in (5, 232)][:29]
    assert spread[0] % 64 != spread[1] % 64 and spread[0] // 64 == 0 and spread[1] // 64 == 3
    add("depth_fib31_spread", _hist(f31, spread))
    return out

"""Raw streams that put headers - real ones and bytes that only look like one - where the geometry of the block discovery
(libhuffman_amd/csrc/kernels/discover.hpp, read through chain_model.py) changes: the piece of a thread, the piece of
lane 63, the row, the workgroup, the scan group, the stream's last wave, the walk's chunk.  Every case knows by
construction where its blocks lie, which candidates the discovery must find and how far the chain goes; tests/
test_chain_model.py holds the CPU model to that, tests/test_gpu_discover_chain.py the kernels to the model.

A block of handmade_streams._handmade_block has a 24-byte header (2 leaves) and ANY payload, so a block that starts at s
with a payload of P - 24 - s bytes puts the next header at exactly P.  Payload bytes are drawn from 1..255: four zero
bytes in a row - what every candidate needs - then stand only where a case puts them.  Test infrastructure (CPU)."""
from __future__ import annotations

import bisect
import struct

import numpy as np

import chain_model as cm
import handmade_streams as hm
from libhuffman_amd import datagen

MAX_TREE = 1025
HEADER2 = 24                                         # the header of a 2-leaf block
BIG_BLOCK = 1 << 22                                  # symbols from which hufgpu_decode_stream takes a LEADING block another way


def planted(block_len: int) -> bytes:
    """twelve bytes that pass the strict test: block_len, a tree of one entry, the marker -1 (no tree: its probe fails)"""
    return struct.pack("<Qh", block_len, 1) + b"\xff\xff"


FAKE = planted(1)
# two strict headers in one 16-byte piece, at +0 (block_len 1, seven entries) and at +6 (block_len 0x70000, one entry)
TWO = bytes([1, 0, 0, 0, 0, 0, 0, 0, 7, 0, 0, 0, 0, 0, 1, 0]) + b"\xff" * 8
TWO_NEEDS = 16 + 2 + 0x70000 // 8                    # bytes of stream from the first of them on
# a block the strict test takes and no decoder: the root's right child is missing, and the payload's first bit asks for it
DAMAGED = hm.header(64, [0x0101, 0x41, -1, -1, -1]) + b"\xff" * 8
EMPTY = struct.pack("<Qh", 0, 0)                     # a block of no symbols: the reference takes it, the strict test does not


class Case:
    """stream[:avail] is readable, `length` drives the block loop; cands = the offsets the discovery must find, index /
    consumed / complete = the chain by construction, data = what its blocks decode to; plain = every candidate is a block
    of the chain and the last one ends the stream; false_below = a candidate that is no block lies below the chain's end"""

    def __init__(self, name, stream, avail, length, cands, index, consumed, complete, data):
        self.name, self.stream, self.avail, self.length = name, stream, avail, length
        self.cands, self.index, self.consumed, self.complete, self.data = cands, index, consumed, complete, data
        self.plain = complete and cands == index
        self.false_below = any(c < consumed and c not in set(index) for c in cands)


class Builder:
    def __init__(self, oracle, seed: int):
        self.oracle, self.rng, self.seed = oracle, np.random.default_rng(seed), seed
        self.buf = bytearray()
        self.real, self.false, self.payloads, self.taken = [], [], [], set()
        self.raws = {}                    # header offset -> the block's symbols, or the (lo, hi) of a 2-leaf block's payload

    @property
    def size(self) -> int:
        return len(self.buf)

    def block(self, b: bytes, raw) -> int:
        at = self.size
        self.real.append(at)
        self.raws[at] = raw
        self.buf += b
        return at

    def two_leaf(self, nbytes: int) -> int:
        """a 2-leaf block of that many payload bytes: 'A' for a 0 bit, 'B' for a 1 bit, whatever the payload holds in the end"""
        assert 0 <= nbytes < BIG_BLOCK // 8, nbytes
        span = (self.size + HEADER2, self.size + HEADER2 + nbytes)
        self.payloads.append(span)
        return self.block(hm._handmade_block(self.rng.integers(1, 256, nbytes, dtype=np.uint8).tobytes(), 2), span)

    def lead(self, to: int) -> int:
        """a 2-leaf block from here on that ends at `to`: the next header stands there"""
        return self.two_leaf(to - self.size - HEADER2)

    def tree_block(self, leaves: int, nsym: int) -> int:
        """a block with a random tree of 4 * leaves - 1 entries (no one-child root)"""
        b, syms, _ = hm.block(self.rng, leaves, 0.3, False, nsym)
        return self.block(b, syms)

    def small_blocks(self, count: int):
        for _ in range(count):
            self.two_leaf(8)

    def plant(self, at: int, what: bytes = FAKE, offs=(0,)):
        """overwrite payload bytes with bytes that look like a header"""
        lo, hi = self.payloads[bisect.bisect_right(self.payloads, (at, 1 << 62)) - 1]         # (payloads ascend)
        assert lo <= at and at + len(what) <= hi, (at, "is not inside a payload")
        assert not any(q in self.taken for q in range(at, at + len(what))), (at, "overlaps a planted header")
        self.taken.update(range(at, at + len(what)))
        self.buf[at:at + len(what)] = what
        self.false += [at + o for o in offs]

    def pad(self, nbytes: int, blocksize: int = 4096):
        """ordinary blocks, the oracle's encoder's, of at least nbytes"""
        while nbytes > 0:
            raw = max(blocksize, min(nbytes * 2, 1 << 22))
            self.seed += 1000
            data = datagen.zipf255(raw, seed=self.seed)
            st, offs = self.oracle.encode(data, blocksize, with_offsets=True)
            keep = int(np.searchsorted(offs, min(nbytes, st.size)))          # whole blocks, the first that reaches nbytes included
            for i, o in enumerate(offs[:keep]):
                self.real.append(self.size + int(o))
                self.raws[self.real[-1]] = data[i * blocksize:(i + 1) * blocksize]
            self.buf += st[:int(offs[keep])].tobytes()
            nbytes -= int(offs[keep])

    def pad_to(self, size: int, blocksize: int = 4096):
        if self.size < size:
            self.pad(size - self.size, blocksize)

    def case(self, name, length=None, avail=None, index=None, consumed=None, complete=True, extra_cands=()):
        stream = np.frombuffer(bytes(self.buf), dtype=np.uint8)
        avail = stream.size if avail is None else avail
        length = avail if length is None else length
        scan_len = min(length, avail)
        real = sorted(self.real)
        cands = [c for c in sorted(real + self.false + list(extra_cands)) if c < scan_len]
        index = real if index is None else index
        consumed = stream.size if consumed is None else consumed
        parts = [self.raws[p] for p in index]
        parts = [r if isinstance(r, np.ndarray) else 0x41 + np.unpackbits(stream[r[0]:r[1]]) for r in parts]
        data = np.concatenate(parts).astype(np.uint8) if parts else np.empty(0, np.uint8)
        return Case(name, stream, avail, length, cands, list(index), consumed, complete, data)


# ---- a. header positions ----------------------------------------------------------------------------------------------
DELTAS = tuple(range(-24, 16))            # around an edge E: the whole piece of lane 63 and a header's fields across E
EDGES = {"wave": cm.WAVE, "row": cm.ROW, "workgroup": cm.WORKGROUP}


def low_zero(delta: int) -> int:
    """A header at E - 1 / E - 2 has the lowest one / two bytes of its block_len in front of the edge and the rest behind:
    with those bytes zero the piece behind the edge alone says that block_len is not 0.  Returns the block_len's unit."""
    return {-1: 256, -2: 65536}.get(delta, 0)


def positions(b: Builder, edge: int, room: int):
    """one position E + delta per delta, every one at an edge of its own; `room`: bytes needed in front of it"""
    k = 0
    for delta in DELTAS:
        k += 1
        while edge * k + delta < b.size + room or (edge < cm.WORKGROUP and edge * k % (4 * edge) == 0):
            k += 1                        # (an edge of the next larger kind is that kind's case)
        yield delta, edge * k + delta


def sweep(oracle, edge_name: str, kind: str) -> Case:
    """kind tree7: the header of a 2-leaf block at every position; tree67: of a block with a tree of 67 entries; planted:
    twelve bytes that look like a header, inside a payload"""
    edge = EDGES[edge_name]
    b = Builder(oracle, 100 + edge)
    if kind == "planted":
        b_positions = []
        for delta, p in positions(b, edge, HEADER2):
            b.lead(p + 512)                                   # (the blocks' own headers: far from every edge)
            b_positions.append((delta, p))
        for delta, p in b_positions:
            b.plant(p, planted(low_zero(delta) or 1))
    else:
        for delta, p in positions(b, edge, HEADER2):
            if b.size < p:
                b.lead(p)
            unit = low_zero(delta)
            if kind == "tree7":
                b.two_leaf(unit // 8 if unit else 40)
            else:
                b.tree_block(17, unit if unit else 300)
    b.pad_to(max(b.size + 4096, cm.PARALLEL_MIN + 4096))
    return b.case(f"sweep-{edge_name}-{kind}")


# ---- b. the stream's last wave ----------------------------------------------------------------------------------------
def last_wave(oracle, lanes: int, leaves: int, row: int = 0) -> Case:
    """length == avail, the last header inside the stream's last, partial wave of `lanes` active lanes.  row 0: the wave's
    other lanes are switched off (tree_grammar_complete_wave's slow branch); another row: they run along with nothing to
    test, and the wave takes the fast branch."""
    b = Builder(oracle, 200 + lanes + leaves)
    last, syms = (bytes(HEADER2 + 1), None) if leaves == 2 else hm.block(b.rng, leaves, 0.3, False, 20)[:2]
    tail = cm.PIECE * lanes - 3
    assert len(last) <= tail, (len(last), tail)
    total = 5 * cm.WORKGROUP + row * cm.ROW + cm.WAVE + tail
    b.pad_to(total - len(last) - 8192)
    b.lead(total - len(last))
    if leaves == 2:
        b.two_leaf(1)
    else:
        b.block(last, syms)
    assert b.size == total and -(-(total % cm.WAVE) // cm.PIECE) == lanes
    return b.case(f"last-wave-{lanes}-lanes-{4 * leaves - 1}-entries-row{row}")


def one_lane(oracle, leaves: int) -> Case:
    """length < avail: length = 1024 k + 1 and a header at 1024 k - one active lane in the last wave"""
    b = Builder(oracle, 300 + leaves)
    at = 5 * cm.WORKGROUP + cm.WAVE
    b.pad_to(at - 8192)
    b.lead(at)
    if leaves == 2:
        b.two_leaf(100)
    else:
        b.tree_block(leaves, 200)
    end = b.size
    b.pad(8192)
    return b.case(f"one-lane-{4 * leaves - 1}-entries", length=at + 1, index=[r for r in b.real if r <= at], consumed=end)


def cut_length(oracle, where: str) -> Case:
    """length ends at a block's edge, inside a later block's header, inside its payload: the chain ends behind the block that
    straddles length"""
    b = Builder(oracle, 400)
    b.pad(cm.PARALLEL_MIN + 3 * 4096)
    b.pad(3 * 4096)
    k = len(b.real) - 3
    p, nxt = b.real[k], b.real[k + 1]
    header_end = p + cm.HEADER_FIXED + 2 * int.from_bytes(b.buf[p + 8:p + 10], "little")
    length = {"edge": p, "header": p + (header_end - p) // 2, "payload": header_end + (nxt - header_end) // 2}[where]
    last = k - 1 if where == "edge" else k
    return b.case(f"cut-{where}", length=length, index=b.real[:last + 1], consumed=b.real[last + 1])


def garbage(oracle, nbytes: int) -> Case:
    b = Builder(oracle, 500 + nbytes)
    b.pad(cm.PARALLEL_MIN + 4096)
    end = b.size
    b.buf += bytes(range(0xa1, 0xa1 + nbytes))
    return b.case(f"garbage-{nbytes}", consumed=end, complete=False)


# ---- c. candidates per workgroup and their order ----------------------------------------------------------------------
def spread(n: int):
    """n offsets inside a workgroup, ascending, in all four rows, away from its edges"""
    return [200 + (i * (cm.WORKGROUP - 1000)) // n for i in range(n)]


def plant_workgroups(b: Builder, first: int, counts):
    """workgroup first + i gets counts[i] planted headers"""
    for i, n in enumerate(counts):
        for o in spread(n):
            b.plant((first + i) * cm.WORKGROUP + o)


def per_workgroup(oracle) -> Case:
    """workgroups of 0, 1, DISC_SLOTS, DISC_SLOTS + 1 and many candidates next to each other in both orders, under one
    block's payload (its own header is workgroup 0's one candidate)"""
    b = Builder(oracle, 600)
    s = cm.DISC_SLOTS
    counts = [0, 0, s, s + 1, s, 300, s, 0, s + 1, 1, s + 1, s + 1, 0, 300, 1]
    b.lead(len(counts) * cm.WORKGROUP + 100)
    plant_workgroups(b, 0, counts)
    b.pad(cm.PARALLEL_MIN)
    return b.case("per-workgroup")


def order_in_workgroup(oracle) -> Case:
    """a candidate of row 0 that a high thread owns in front of one of row 1 that a low thread owns - once alone in their
    workgroup (slots), once among more than DISC_SLOTS (verdict masks) -, and two candidates in ONE piece, both ways"""
    b = Builder(oracle, 700)
    b.lead(5 * cm.WORKGROUP + 100)
    for wg, more in ((1, 0), (2, cm.DISC_SLOTS)):
        base = wg * cm.WORKGROUP
        b.plant(base + 200 * cm.PIECE + 3)
        b.plant(base + cm.ROW + 5 * cm.PIECE + 9)
        for i in range(more):
            b.plant(base + 2 * cm.ROW + (17 + 40 * i) * cm.PIECE + i)
    for wg, more in ((3, 0), (4, cm.DISC_SLOTS)):
        base = wg * cm.WORKGROUP
        b.plant(base + cm.ROW + 77 * cm.PIECE, TWO, (0, 6))
        for i in range(more):
            b.plant(base + 3 * cm.ROW + (9 + 40 * i) * cm.PIECE + 2 * i)
    b.pad(max(cm.PARALLEL_MIN, TWO_NEEDS))
    return b.case("order-in-workgroup")


# ---- d. the walk ------------------------------------------------------------------------------------------------------
def long_jump(oracle, small: int) -> Case:
    """one block whose payload holds more planted headers than a chunk of the walk has candidates, back to back: its link
    jumps over a whole chunk.  small: that many small blocks in front (the jump then starts in chunk 0 and lands in chunk 2)"""
    b = Builder(oracle, 800 + small)
    b.small_blocks(small)
    n = cm.WALK_CHUNK + 808
    at = b.two_leaf(12 * n + 100)
    for i in range(n):
        b.plant(at + HEADER2 + 50 + 12 * i)
    b.pad(cm.PARALLEL_MIN)
    return b.case(f"long-jump-behind-{small}")


def not_at_zero(oracle) -> Case:
    """the stream starts with a block the reference takes and the strict test rejects: nothing is validated"""
    b = Builder(oracle, 900)
    b.buf += EMPTY
    b.pad(cm.PARALLEL_MIN + 4096)
    return b.case("not-at-zero", index=[], consumed=0, complete=False)


def chain_ends(oracle, how: str) -> Case:
    """behind candidate WALK_CHUNK, in the walk's second chunk: `bad`, a block whose probe fails (the chain ends in front of
    it); `notfound`, a good block with no strict header behind it (the chain ends behind it)"""
    b = Builder(oracle, 1000)
    b.small_blocks(cm.WALK_CHUNK + 1)
    if how == "bad":
        stop = b.size
        b.buf += DAMAGED
        extra = [stop]
    else:
        b.two_leaf(64)
        stop = b.size
        b.buf += EMPTY
        extra = []
    counted = list(b.real)
    b.pad(cm.PARALLEL_MIN)
    return b.case(f"chain-ends-{how}", index=counted, consumed=stop, complete=False, extra_cands=extra)


# ---- e. capacity and scan groups --------------------------------------------------------------------------------------
def few(oracle) -> Case:
    b = Builder(oracle, 1100)
    b.pad(cm.PARALLEL_MIN + 4096, 16384)
    return b.case("few")


def two_scan_groups(oracle) -> Case:
    """a little more than one scan group of workgroups, a slots workgroup and a masks workgroup on each side of its edge"""
    b = Builder(oracle, 1200)
    g = cm.DISC_SCAN_GROUP
    b.pad_to((g - 3) * cm.WORKGROUP - 70000, 65536)
    b.pad_to((g - 3) * cm.WORKGROUP - 8192, 2048)
    b.lead((g + 3) * cm.WORKGROUP + 100)
    s = cm.DISC_SLOTS
    plant_workgroups(b, g - 2, [s, s + 3, s + 1, 2])         # workgroups g - 2, g - 1 | g, g + 1
    b.pad(cm.PARALLEL_MIN, 65536)
    return b.case("two-scan-groups")


# ---- f. thresholds ----------------------------------------------------------------------------------------------------
def threshold_stream(oracle) -> Case:
    b = Builder(oracle, 1300)
    b.pad(cm.PARALLEL_MIN + 8192, 1024)
    return b.case("thresholds")


CASES = {}
for _edge in EDGES:
    for _kind in ("tree7", "tree67", "planted"):
        CASES[f"sweep-{_edge}-{_kind}"] = (lambda o, e=_edge, k=_kind: sweep(o, e, k))
for _lanes, _leaves, _row in ((2, 2, 0), (33, 2, 0), (63, 2, 0), (33, 60, 0), (63, 100, 0), (33, 2, 2), (63, 100, 2)):
    CASES[f"last-wave-{_lanes}-{_leaves}-row{_row}"] = (lambda o, a=_lanes, b=_leaves, c=_row: last_wave(o, a, b, c))
for _leaves in (2, 100):
    CASES[f"one-lane-{_leaves}"] = (lambda o, a=_leaves: one_lane(o, a))
for _where in ("edge", "header", "payload"):
    CASES[f"cut-{_where}"] = (lambda o, a=_where: cut_length(o, a))
for _n in (1, 9, 10):
    CASES[f"garbage-{_n}"] = (lambda o, a=_n: garbage(o, a))
CASES["per-workgroup"] = per_workgroup
CASES["order-in-workgroup"] = order_in_workgroup
CASES["long-jump-0"] = lambda o: long_jump(o, 0)
CASES["long-jump-8190"] = lambda o: long_jump(o, cm.WALK_CHUNK - 2)
CASES["not-at-zero"] = not_at_zero
CASES["chain-ends-bad"] = lambda o: chain_ends(o, "bad")
CASES["chain-ends-notfound"] = lambda o: chain_ends(o, "notfound")
CASES["few"] = few
CASES["two-scan-groups"] = two_scan_groups
CASES["thresholds"] = threshold_stream

_BUILT = {}


def get(oracle, name: str) -> Case:
    """the case, built once a process"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name](oracle)
    return _BUILT[name]

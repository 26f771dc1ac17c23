"""Blocks built to sit on the branches of the encoder's counting bodies - hist_tree_block (kernels/hist_tree.hpp), hl_count
(kernels/hist_lanes.hpp) and hist256_kernel (kernels/histogram.hpp) - with histograms whose tree changes when one count is
off by one.  A case is a histogram, a layout (where the bytes lie), a blocksize and the byte offset of the data behind an
aligned device address; its blocks all carry the same counts, so the block starts walk through the alignments.

census(body, block, addr) walks the index arithmetic of a body as written - head, nvec, the entry window, the four-loads
loops, the single loop, tail0, the hot pick from the wave's first four chunks, `act` in loops a wave has split in - and
returns the counts the body would produce and how often each event of EVENTS happened; `mutant` makes one defined mistake
on the way.  test_count_cases.py checks the table on the CPU, test_gpu_count_cases.py runs it through every encode route.
Test infrastructure (CPU, numpy)."""
from __future__ import annotations

import dataclasses
import zlib

import numpy as np

import tree_rounds_ref as M

HIST_THREADS = 256                      # kernels/histogram.hpp
HL_THREADS = 512                        # kernels/hist_lanes.hpp
HL_AHEAD = 8
HL_MIN_BLOCK = 32768                    # shorter blocks take the fused kernel
HT_PACKED_MAX_BLOCK = 131072            # the fused kernel's 16-bit counters up to here
HTP_ARRAYS = 2
HT_COPIES = 2
HIST_COPIES = 4
CHUNKED_FROM = 1 << 21
BIG_BLOCK = 1 << 22
CHUNK_SYMS = 262144
TREE_MAX_TOTAL = 1 << 22                # tree_rounds_ref.tree takes blocks below this

BODIES = ("fused_packed", "fused_unpacked", "hl_count", "hist256")
EVENTS = (
    "head_bytes", "tail_bytes",
    "window_in", "window_out",          # threads of a wave the entry window splits: inside, outside
    "uni_chunks",                       # 16 bytes of one value counted with one add
    "fold_full", "fold_partial",        # a wave step of one value counted with one add: all 64 lanes, fewer
    "fold_first_odd",                   # ... whose first active lane is odd (its `one` is the high half)
    "hot0_waves", "hot1_waves",         # waves that single out one value, two values
    "hot_side_bytes",                   # bytes counted in a lane's side words
    "max16",                            # the largest value a 16-bit counter reaches (not a count of events)
)
BODY_EVENTS = {
    "fused_packed": EVENTS,
    "fused_unpacked": tuple(e for e in EVENTS if e not in ("max16", "fold_first_odd")),      # (`one` is 1 in every lane)
    "hl_count": ("head_bytes", "tail_bytes", "window_in", "window_out", "max16"),
    "hist256": ("head_bytes", "tail_bytes", "uni_chunks", "fold_full", "fold_partial"),
}
MUTANTS = (
    "tail_dropped", "head_twice", "uni_15", "fold_popcount_minus_1", "fold_one_of_lane0", "side_not_added",
    "side1_to_hot0", "wrap_32768", "window_out_skipped",
)
# A fold that takes lane 0's `one` in the word of an odd first active lane moves the run from the high half of that word to
# its low half.  The halves are summed, and a wave's share of the largest packed block is 32 768 bytes, so neither half can
# pass 65 535: no count changes, on any input.  The census shows it only in max16 and the mutant is kept to say so.
EQUIVALENT = ("fold_one_of_lane0",)
# the bodies a mutant's branch exists in
MUTANT_BODIES = {
    "tail_dropped": BODIES, "head_twice": BODIES,
    "uni_15": ("fused_packed", "fused_unpacked", "hist256"),
    "fold_popcount_minus_1": ("fused_packed", "fused_unpacked", "hist256"),
    "fold_one_of_lane0": ("fused_packed",),
    "side_not_added": ("fused_packed", "fused_unpacked"), "side1_to_hot0": ("fused_packed", "fused_unpacked"),
    "wrap_32768": ("fused_packed", "hl_count"),
    "window_out_skipped": ("hl_count",),
}


# ---------------------------------------------------------------------------------------------------------------------
# histograms
# ---------------------------------------------------------------------------------------------------------------------
def ramp(n: int, k: int, first: int = 0) -> np.ndarray:
    """k counts base, base + 1, ... ascending with the byte value (first .. first + k - 1) that sum to n; what is left
    over goes one each to the top counts"""
    base, left = divmod(n - k * (k - 1) // 2, k)
    assert base >= 1 and first + k <= 256, (n, k)
    h = np.zeros(256, dtype=np.int64)
    h[first:first + k] = base + np.arange(k)
    if left:
        h[first + k - left:first + k] += 1
    assert h.sum() == n
    return h


def skewed(n: int, k: int, hot: int = 4, share: int = 8) -> np.ndarray:
    """`hot` values of at least n / share bytes each, counts H, H + 1, ..., at byte values above a ramp of k - hot values
    that holds the rest"""
    H = -(-n // share)
    rest = n - hot * H - hot * (hot - 1) // 2
    h = ramp(rest, k - hot, first=3)
    top = 3 + (k - hot) + 5
    h[top:top + hot] = H + np.arange(hot)
    assert h.sum() == n and h[:top].max() < H
    return h


def under(n: int, top: int, value: int, run: int = 256) -> np.ndarray:
    """byte `value` top times inside a run of step 1: top + 1 above it (byte value + 1), top - 1, top - 2, ... under it
    on as many values as n allows, and a small ramp of what is left"""
    h = np.zeros(256, dtype=np.int64)
    h[value + 1], h[value] = top + 1, top
    rest, c, v = n - 2 * top - 1, top - 1, value - 1
    while rest >= c and c > 64 and value - v <= run:
        h[v] = c
        rest, c, v = rest - c, c - 1, v - 1
    if rest:
        k = max(1, min(32, int((np.sqrt(8 * rest + 1) - 1) / 2)))
        small = ramp(rest, k, first=0)
        assert small.max() < c and k <= v
        h += small
    assert h.sum() == n
    return h


LAST_COUNTS = (2, 3, 4, 4, 4, 4)        # 21 bytes whose tree sees every miscount of +-1 and +16 (found by search)


# ---------------------------------------------------------------------------------------------------------------------
# layouts: where the bytes of a histogram lie in a block that starts `addr` bytes behind an aligned address.  A layout
# fixes some vectors and leaves the rest to _fill, which keeps the values of `avoid` - the ones whose miscount the tree
# would not show - out of the head, the tail and the vectors the fused body picks its hot values from.
# ---------------------------------------------------------------------------------------------------------------------
def geometry(length: int, addr: int):
    """(head, nvec, tail0) as every body computes them"""
    head = min(length, (16 - (addr & 15)) & 15)
    nvec = (length - head) >> 4
    return head, nvec, head + (nvec << 4)


def pick_region(nvec: int) -> np.ndarray:
    """the vectors the fused body has counted when a wave looks for its hot values: k * 256 + tid, k < 4, of the threads
    with tid + 3 * 256 < nvec"""
    t = min(HIST_THREADS, max(0, nvec - 3 * HIST_THREADS))
    return (np.arange(4)[:, None] * HIST_THREADS + np.arange(t)[None, :]).ravel()


def _pool(left: np.ndarray, rng) -> np.ndarray:
    d = np.repeat(np.arange(256, dtype=np.uint8), left)
    rng.shuffle(d)
    return d


def _fill(out, free, left, addr, rng, avoid=()):
    """the bytes of `left`, shuffled, into the positions free[] of out"""
    n = out.size
    head, nvec, tail0 = geometry(n, addr)
    pool = _pool(left, rng)
    assert pool.size == int(free.sum())
    pos = np.flatnonzero(free)
    strict = np.zeros(n, dtype=bool)
    strict[:head] = True
    strict[tail0:] = True
    reg = pick_region(nvec)
    if reg.size:
        strict[(head + 16 * reg[:, None] + np.arange(16)[None, :]).ravel()] = True
    strict = strict[pos]
    ok = ~np.isin(pool, np.asarray(list(avoid), dtype=np.uint8))
    k = int(strict.sum())
    good = np.flatnonzero(ok)
    assert good.size >= k, "not enough bytes the tree sees for the head, the tail and the first chunks"
    first = np.zeros(pool.size, dtype=bool)
    first[good[:k]] = True
    out[pos[strict]] = pool[first]
    out[pos[~strict]] = pool[~first]
    # a shuffled vector that came out as sixteen times one value of `avoid` would be a run of it: its first byte changes
    # places with the first byte of a free vector further on
    vec = out[head:tail0].reshape(nvec, 16)
    whole = free[head:tail0].reshape(nvec, 16).all(axis=1)
    bad = np.flatnonzero(whole & (vec == vec[:, :1]).all(axis=1) & np.isin(vec[:, 0], np.asarray(list(avoid), dtype=np.uint8)))
    inside = np.zeros(nvec, dtype=bool)
    inside[reg] = True
    for i in bad:
        j = next(j for j in range(i + 1, nvec) if whole[j] and not inside[j] and vec[j, 0] != vec[i, 0])
        vec[i, 0], vec[j, 0] = vec[j, 0], vec[i, 0]
    return out


def _vec_mask(n, head, vectors):
    m = np.zeros(n, dtype=bool)
    if len(vectors):
        m[(head + 16 * np.asarray(vectors)[:, None] + np.arange(16)[None, :]).ravel()] = True
    return m


def lay_shuffled(hist, addr, rng, avoid=(), **_):
    n = int(hist.sum())
    return _fill(np.empty(n, dtype=np.uint8), np.ones(n, dtype=bool), hist, addr, rng, avoid)


def lay_runs16(hist, addr, rng, avoid=(), **_):
    """as many 16-byte vectors of one value as each count allows (an eighth of the vectors stays mixed), at shuffled
    places among the vectors behind the head; the rest in mixed vectors"""
    n = int(hist.sum())
    head, nvec, tail0 = geometry(n, addr)
    left = hist.copy()
    full = left // 16
    full[list(avoid)] = 0
    while full.sum() > max(0, nvec - max(1, nvec // 8)):
        full[np.argmax(full)] -= 1
    vals = np.repeat(np.arange(256, dtype=np.uint8), full)
    left -= full * 16
    out = np.empty(n, dtype=np.uint8)
    rng.shuffle(vals)
    reg = pick_region(nvec)                                     # (those first: what stays mixed there has to avoid `avoid`)
    rest = np.setdiff1d(np.arange(nvec), reg)
    where = np.concatenate([rng.permutation(reg), rng.permutation(rest)])[:vals.size]
    out[head:tail0].reshape(nvec, 16)[where] = vals[:, None]
    return _fill(out, ~_vec_mask(n, head, where), left, addr, rng, avoid)


def lay_wave_steps(hist, addr, rng, avoid=(), **_):
    """spans of 64 vectors (a wave's step, 1 KiB) of one value: the last, partial span first, then every other span from
    the front, as long as a value has the bytes; everything else shuffled into the steps next to them"""
    n = int(hist.sum())
    head, nvec, tail0 = geometry(n, addr)
    left = hist.copy()
    usable = left.copy()
    usable[list(avoid)] = 0
    spans = -(-nvec // 64)
    size = [min(64, nvec - 64 * s) * 16 for s in range(spans)]
    out = np.empty(n, dtype=np.uint8)
    free = np.ones(n, dtype=bool)
    done = set()
    for s in ([spans - 1] if spans and size[-1] < 1024 else []) + list(range(0, spans, 2)):
        v = int(np.argmax(usable))
        if s in done or usable[v] < size[s] or len(done) > spans // 2:
            continue
        done.add(s)
        left[v] -= size[s]
        usable[v] -= size[s]
        lo = head + 1024 * s
        out[lo:lo + size[s]] = v
        free[lo:lo + size[s]] = False
    return _fill(out, free, left, addr, rng, avoid)


def _lay_vectors(hist, addr, rng, avoid, value, vectors):
    n = int(hist.sum())
    head, nvec, tail0 = geometry(n, addr)
    left = hist.copy()
    left[value] -= 16 * len(vectors)
    assert left[value] >= 0
    out = np.empty(n, dtype=np.uint8)
    m = _vec_mask(n, head, vectors)
    out[m] = value
    return _fill(out, ~m, left, addr, rng, avoid)


def lay_one_lane(hist, addr, rng, avoid=(), value=0, lane=0, **_):
    """every vector i = lane (mod 64) holds `value` (as many as its count allows); the rest shuffled around them"""
    nvec = geometry(int(hist.sum()), addr)[1]
    return _lay_vectors(hist, addr, rng, avoid, value, np.arange(lane, nvec, 64)[:int(hist[value]) // 16])


def lay_wave0(hist, addr, rng, avoid=(), value=0, **_):
    """the first 1 KiB of every 4 KiB - wave 0's share of a 256-thread body - holds `value`"""
    i = np.arange(geometry(int(hist.sum()), addr)[1])
    return _lay_vectors(hist, addr, rng, avoid, value, i[(i % 256) < 64])


LAYOUTS = {"shuffled": lay_shuffled, "runs16": lay_runs16, "wave_steps": lay_wave_steps, "one_lane": lay_one_lane,
           "wave0": lay_wave0}


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
def _xor_max(v: np.ndarray, act: np.ndarray) -> np.ndarray:
    """for (o = 1; o < 64; o <<= 1) v = max(v, wave_xor_any(v, o)) with the lanes outside `act` read as 0"""
    v = np.where(act, v, 0).astype(np.int64)
    lanes = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        v = np.where(act, np.maximum(v, v[lanes ^ o]), 0)
    return v


def census(body: str, block: np.ndarray, addr: int = 0, mutant: str | None = None, ahead: int = HL_AHEAD,
           picks: set | None = None):
    """(256 counts, {event: count}) of `body` on `block` lying `addr` bytes behind an aligned address; `picks` receives
    the values the waves single out"""
    assert body in BODIES and (mutant is None or mutant in MUTANTS)
    if mutant is not None and body not in MUTANT_BODIES[mutant]:
        mutant = None
    if body == "hl_count":
        return _census_lanes(block, addr, mutant, ahead)
    return _census_atomic(body, block, addr, mutant, picks)


def _census_lanes(block, addr, mutant, ahead):
    T = HL_THREADS
    ev = dict.fromkeys(BODY_EVENTS["hl_count"], 0)
    n = block.size
    head, nvec, tail0 = geometry(n, addr)
    vec = block[head:tail0].reshape(nvec, 16)
    i = np.arange(nvec)
    tid = i % T
    full8 = (np.arange(T) + (ahead - 1) * T) < nvec               # per thread
    keep = np.ones(nvec, dtype=bool)
    for w in range(T // 64):
        inside = int(full8[64 * w:64 * w + 64].sum())
        if 0 < inside < 64:
            ev["window_in"] += inside
            ev["window_out"] += 64 - inside
            if mutant == "window_out_skipped":
                out_tids = 64 * w + np.flatnonzero(~full8[64 * w:64 * w + 64])
                keep &= ~(np.isin(tid, out_tids) & (i < ahead * T))
    # a counter: lane l of every wave (l and l + 32 share a word, low and high half)
    lane = (i % 64)[keep]
    per = np.bincount((lane[:, None] * 256 + vec[keep].astype(np.int64)).ravel(), minlength=64 * 256).reshape(64, 256)
    hb, tb = block[:head], block[tail0:]
    ev["head_bytes"], ev["tail_bytes"] = int(hb.size), int(tb.size)
    np.add.at(per, (np.arange(hb.size) % 64, hb), 2 if mutant == "head_twice" else 1)
    if mutant != "tail_dropped":
        np.add.at(per, (np.arange(tb.size) % 64, tb), 1)
    ev["max16"] = int(per.max())
    assert ev["max16"] < 65536, "a lane's 16-bit counter overflows into its neighbour's"
    if mutant == "wrap_32768":
        per = per % 32768
    return per.sum(axis=0), ev


def _census_atomic(body, block, addr, mutant, picks):
    T = HIST_THREADS
    fused = body.startswith("fused")
    packed = body == "fused_packed"
    ev = dict.fromkeys(BODY_EVENTS[body], 0)
    n = block.size
    head, nvec, tail0 = geometry(n, addr)
    vec = block[head:tail0].reshape(nvec, 16)
    first = vec[:, 0].astype(np.int64) if nvec else np.zeros(0, dtype=np.int64)
    uni = (vec == vec[:, :1]).all(axis=1) if nvec else np.zeros(0, dtype=bool)
    lanes = np.arange(64)
    # what a 16-bit counter is: (wave, the lane's array, the lane's half) - `own` numbers them; 32-bit bodies: the copy
    arrs = HTP_ARRAYS if packed else (HT_COPIES if fused else HIST_COPIES)

    def counter(w, lane):
        if packed:
            return (w * arrs + ((lane >> 1) & (arrs - 1))) * 2 + (lane & 1)
        return w * arrs + (lane & (arrs - 1))
    ncounters = (T // 64) * arrs * (2 if packed else 1)
    per = np.zeros((ncounters, 256), dtype=np.int64)

    hb, tb = block[:head], block[tail0:]
    ev["head_bytes"], ev["tail_bytes"] = int(hb.size), int(tb.size)
    np.add.at(per, (counter(0, np.arange(hb.size)), hb), 2 if mutant == "head_twice" else 1)

    def plain(w, act, idx):
        """hist_add_chunk of the lanes `act` of wave w on the vectors idx[lane]"""
        la = np.flatnonzero(act)
        vi = idx[la]
        f = int(la[0])
        b0 = int(first[vi[0]])
        if bool((uni[vi] & (first[vi] == b0)).all()):
            ev["fold_full" if la.size == 64 else "fold_partial"] += 1
            if "fold_first_odd" in ev:
                ev["fold_first_odd"] += f & 1
            pop = la.size - (1 if mutant == "fold_popcount_minus_1" else 0)
            c = counter(w, f)
            if mutant == "fold_one_of_lane0" and packed and f & 1:
                c -= 1                                   # the word of lane f, the half of lane 0
            per[c, b0] += 16 * pop
            return
        u = uni[vi]
        ev["uni_chunks"] += int(u.sum())
        np.add.at(per, (counter(w, la[u]), first[vi[u]]), 15 if mutant == "uni_15" else 16)
        m = ~u
        np.add.at(per, (np.repeat(counter(w, la[m]), 16), vec[vi[m]].ravel()), 1)

    for w in range(T // 64):
        i = (64 * w + lanes).astype(np.int64)
        hot0 = np.full(64, 0x100)
        hot1 = np.full(64, 0x100)
        if fused:
            enter = i + 3 * T < nvec
            if 0 < int(enter.sum()) < 64:
                ev["window_in"] += int(enter.sum())
                ev["window_out"] += 64 - int(enter.sum())
            if enter.any():
                for k in range(4):
                    plain(w, enter, i + k * T)
                i = np.where(enter, i + 4 * T, i)
                # the wave's counts so far, bin = lane + 64 qd; the lanes outside the window are not there
                wave = per[counter(w, 0):counter(w, 0) + arrs * (2 if packed else 1)].sum(axis=0)
                cand = [(wave[lanes + 64 * qd] << 8) | (lanes + 64 * qd) for qd in range(4)]
                best = _xor_max(np.maximum(np.maximum(cand[0], cand[1]), np.maximum(cand[2], cand[3])), enter)
                pick = enter & ((best >> 8) >= 256) & ((best >> 8) < 4096)
                second = np.zeros(64, dtype=np.int64)
                for qd in range(4):
                    second = np.maximum(second, np.where(cand[qd] == best, 0, cand[qd]))
                second = _xor_max(second, pick)
                hot0 = np.where(pick, best & 0xff, 0x100)
                hot1 = np.where(pick & ((second >> 8) >= 256), second & 0xff, 0x100)
                ev["hot0_waves"] += int(pick.any())
                ev["hot1_waves"] += int((hot1 < 0x100).any())
                if picks is not None:
                    picks |= set(hot0[hot0 < 0x100].tolist()) | set(hot1[hot1 < 0x100].tolist())
            # the lanes with a hot value count everything they have left with hist_add_chunk_hot (no wave operation in it)
            for l in np.flatnonzero(hot0 < 0x100):
                mine = np.arange(int(i[l]), nvec, T)
                i[l] = nvec
                if not mine.size:
                    continue
                c = counter(w, int(l))
                by = vec[mine].ravel().astype(np.int64)
                wt = np.ones(by.size, dtype=np.int64)
                if mutant == "uni_15":
                    wt[np.repeat(uni[mine], 16) & (np.arange(by.size) % 16 == 0)] = 0
                ev["uni_chunks"] += int(uni[mine].sum())
                is0, is1 = by == hot0[l], by == hot1[l]
                ev["hot_side_bytes"] += int((wt * (is0 | is1)).sum())
                if mutant == "side_not_added":
                    wt = wt * ~(is0 | is1)
                if mutant == "side1_to_hot0":
                    by = np.where(is1, hot0[l], by)
                per[c] += np.bincount(by, weights=wt, minlength=256).astype(np.int64)
        cond = i + 3 * T < nvec
        while cond.any():
            for k in range(4):
                plain(w, cond, i + k * T)
            i = np.where(cond, i + 4 * T, i)
            cond = cond & (i + 3 * T < nvec)
        cond = i < nvec
        while cond.any():
            plain(w, cond, i)
            i = np.where(cond, i + T, i)
            cond = cond & (i < nvec)
    if mutant != "tail_dropped":
        np.add.at(per, (counter(0, np.arange(tb.size)), tb), 1)
    if packed:
        ev["max16"] = int(per.max())
        assert ev["max16"] < 65536, "a 16-bit counter overflows into its neighbour's"
        if mutant == "wrap_32768":
            per = per % 32768
    return per.sum(axis=0), ev


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: does the serialised tree change when one count is off?
# ---------------------------------------------------------------------------------------------------------------------
DELTAS = (1, -1, 16, -16)


def tree_of(hist) -> tuple:
    return tuple(M.tree(hist)[0])


def unseen(hist, deltas=DELTAS, symbols=None) -> dict:
    """{symbol: [deltas that leave the serialised tree as it is]} over the symbols present (a count never goes below 1:
    a value that vanishes always shows)"""
    hist = np.asarray(hist, dtype=np.int64)
    assert hist.sum() + max(deltas) < TREE_MAX_TOTAL
    base = tree_of(hist)
    out = {}
    for s in (np.flatnonzero(hist) if symbols is None else symbols):
        miss = []
        for d in deltas:
            if hist[s] + d < 1:
                continue
            h = hist.copy()
            h[s] += d
            if tree_of(h) == base:
                miss.append(d)
        if miss:
            out[int(s)] = miss
    return out


def unseen_oracle(oracle, hist, deltas=DELTAS, symbols=None) -> dict:
    """unseen() through the oracle's encoder, for a block tree_rounds_ref.tree does not take"""
    def tree(h):
        return tuple(M.oracle_tree(oracle, np.repeat(np.arange(256, dtype=np.uint8), h)))
    base = tree(hist)
    out = {}
    for s in (np.flatnonzero(hist) if symbols is None else symbols):
        miss = []
        for d in deltas:
            h = hist.copy()
            h[s] += d
            if h[s] >= 1 and tree(h) == base:
                miss.append(d)
        if miss:
            out[int(s)] = miss
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    hname: str                          # the histogram's name in BLIND
    hist: np.ndarray                    # the counts of every full block
    layout: str
    bs: int                             # the blocksize it is encoded with (= hist.sum())
    blocks: int                         # full blocks
    last: int                           # bytes of the short last block (0: none)
    offset: int                         # the data starts this many bytes behind an aligned device address
    bodies: tuple                       # the counting bodies its route runs
    claims: dict                        # {body: events at least one of its blocks reaches on that body}
    args: dict = dataclasses.field(default_factory=dict)       # the layout's
    group: str = ""                     # which test of test_gpu_count_cases.py runs it

    @property
    def n(self) -> int:
        return self.bs * self.blocks + self.last

    @property
    def blind(self) -> tuple:
        return BLIND[self.hname]

    def last_hist(self) -> np.ndarray:
        h = np.zeros(256, dtype=np.int64)
        if self.last == 21:
            h[100:106] = LAST_COUNTS
        elif self.last:
            h = ramp(self.last, 40, first=100)
        return h

    def last_blind(self) -> tuple:
        return () if self.last <= 21 else BLIND["last%d" % self.last]

    def data(self) -> np.ndarray:
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        parts = [LAYOUTS[self.layout](self.hist, self.offset + b * self.bs, rng, avoid=self.blind, **self.args)
                 for b in range(self.blocks)]
        if self.last:
            parts.append(lay_shuffled(self.last_hist(), self.offset + self.blocks * self.bs, rng, avoid=self.last_blind()))
        d = np.concatenate(parts)
        assert d.size == self.n
        return d

    def block_list(self, data):
        """[(bytes, address modulo 16, counts, the values of them the tree does not see)] of every block"""
        out = []
        for b in range(-(-self.n // self.bs)):
            blk = data[b * self.bs:(b + 1) * self.bs]
            full = blk.size == self.bs
            out.append((blk, (self.offset + b * self.bs) & 15, self.hist if full else self.last_hist(),
                        self.blind if full else self.last_blind()))
        return out

    def own_symbols(self, blk, addr) -> set:
        """the symbols a block of the case is about: the values in its head and tail positions, the values of its runs,
        the values a fused body's waves single out, the value on the loaded counter"""
        head, nvec, tail0 = geometry(blk.size, addr)
        own = set(blk[:head].tolist()) | set(blk[tail0:].tolist())
        if self.layout != "shuffled" and blk.size == self.bs:
            v = blk[head:tail0].reshape(nvec, 16)
            own |= set(v[(v == v[:, :1]).all(axis=1), 0].tolist())
            if "value" in self.args:
                own.add(self.args["value"])
        for body in self.bodies:
            if body.startswith("fused"):
                census(body, blk, addr, picks=own)
        return own


# Per histogram, the values whose miscount by +-1 or +-16 leaves the serialised tree as it is (tree_rounds_ref.tree; the
# oracle for the block of 4 MiB + 1).  Conditions on the inputs: test_count_cases.py computes them again and requires
# these, and no layout puts such a value where a case looks.  They are the ends of the runs of step 1 and the two values
# next to where a ramp's leftover starts.
BLIND = {
    "quarters4097": (24, 40, 42),
    "flat4097": (30, 31),
    "flat4097_48": (0, 6, 7, 47),
    "flat13009": (111, 127),
    "flat32767": (0, 64, 65, 127),
    "flat32769": (0, 62, 63, 127),
    "flat60001": (0, 94, 95, 127),
    "flat65537": (0, 62, 63, 127),
    "flat131072": (0, 63, 64, 127),
    "flat2097153": (0, 62, 63, 127),
    "skewed13009": (3, 17, 18, 62, 68, 71),
    "skewed32767": (3, 35, 36, 62, 68, 71),
    "skewed32769": (3, 37, 38, 62, 68, 71),
    "skewed60001": (3, 41, 42, 62, 68, 71),
    "skewed65537": (3, 33, 34, 62, 68, 71),
    "skewed131073": (3, 25, 26, 62, 68, 71),
    "skewed200001": (3, 61, 62, 68, 71),
    "skewed4194305": (3, 9, 10, 62, 68, 71),
    "under2097151": (0, 16, 17, 31, 138, 201),
    "under131072": (76, 78),
    "last13009": (100, 110, 111, 139),
    "last786453": (100, 106, 107, 139),
}

FUSED = ("fused_packed", "hist256")
LANES = ("hl_count", "hist256")
HEADTAIL = ("head_bytes", "tail_bytes")
WINDOW = ("window_in", "window_out")


def histograms() -> dict:
    h = {"quarters4097": skewed(4097, 35, hot=3, share=4), "flat4097": ramp(4097, 64), "flat4097_48": ramp(4097, 48)}
    for n in (13009, 32767, 32769, 60001, 65537, 131072, 2097153):
        h["flat%d" % n] = ramp(n, 128)
    for n in (13009, 32767, 32769, 60001, 65537, 131073, 200001, 4194305):
        h["skewed%d" % n] = skewed(n, 64)
    h["under2097151"] = under((1 << 21) - 1, 32768, 200)
    h["under131072"] = under(131072, 32768, 77, run=1)
    return h


def cases() -> list:
    out = []
    H = histograms()

    def add(name, hname, layout, blocks=17, last=21, offset=0, bodies=None, claims=None, group="", **args):
        hist = H[hname]
        bs = int(hist.sum())
        bodies = (FUSED if bs < HL_MIN_BLOCK else LANES) if bodies is None else bodies
        assert not any(c.name == name for c in out)
        out.append(Case(name, hname, hist, layout, bs, blocks, last, offset, tuple(bodies), claims or {}, args, group))

    # the fused packed route: 17 blocks whose starts take all 16 alignments, and a block of 21 bytes
    add("f4097_flat_shuffled", "flat4097", "shuffled", group="fused", claims={"fused_packed": HEADTAIL, "hist256": HEADTAIL})
    add("f4097_flat_runs16", "flat4097_48", "runs16", offset=5, group="fused",
        claims={"fused_packed": HEADTAIL + ("uni_chunks",), "hist256": ("uni_chunks",)})
    add("f4097_quarters_wave_steps", "quarters4097", "wave_steps", group="fused",
        claims={"fused_packed": ("fold_full", "fold_partial"), "hist256": ("fold_full", "fold_partial")})
    # ... 13 009: nvec is 812 or 813, inside the entry window (wave 0 splits at lane 44 or 45)
    add("f13009_flat_shuffled", "flat13009", "shuffled", group="fused", claims={"fused_packed": WINDOW})
    add("f13009_flat_runs16", "flat13009", "runs16", offset=11, group="fused", claims={"fused_packed": WINDOW + ("uni_chunks",)})
    add("f13009_skewed_shuffled", "skewed13009", "shuffled", group="fused", claims={"fused_packed": WINDOW + ("hot0_waves", "hot1_waves")})
    add("f13009_skewed_runs16", "skewed13009", "runs16", offset=11, group="fused", claims={"fused_packed": WINDOW + ("uni_chunks", "hot0_waves")})
    add("f13009_skewed_wave_steps", "skewed13009", "wave_steps", group="fused",
        claims={"fused_packed": WINDOW + ("fold_partial", "fold_first_odd", "hot0_waves"), "hist256": ("fold_partial",)})
    # ... 32 767: every thread enters, the waves' hot values are counted in the side words; thread 255 leaves the
    # four-loads loop alone (a fold of one lane, the first active lane odd)
    add("f32767_flat_shuffled", "flat32767", "shuffled", offset=5, group="fused")
    add("f32767_flat_runs16", "flat32767", "runs16", group="fused", claims={"fused_packed": ("uni_chunks", "fold_partial", "fold_first_odd")})
    add("f32767_skewed_shuffled", "skewed32767", "shuffled", offset=5, group="fused",
        claims={"fused_packed": ("hot0_waves", "hot1_waves", "hot_side_bytes")})
    add("f32767_skewed_runs16", "skewed32767", "runs16", group="fused",
        claims={"fused_packed": ("uni_chunks", "hot0_waves", "hot1_waves", "hot_side_bytes")})
    add("f32767_skewed_wave_steps", "skewed32767", "wave_steps", group="fused",
        claims={"fused_packed": ("fold_full", "hot0_waves", "hot_side_bytes")})

    # the lane-private route; 60 001: nvec is 3 750, inside the window of the eight vectors ahead
    add("l32769_flat_shuffled", "flat32769", "shuffled", group="lanes", claims={"hl_count": HEADTAIL})
    add("l32769_skewed_runs16", "skewed32769", "runs16", offset=5, group="lanes")
    add("l60001_flat_shuffled", "flat60001", "shuffled", group="lanes", claims={"hl_count": WINDOW})
    add("l60001_skewed_runs16", "skewed60001", "runs16", offset=11, group="lanes", claims={"hl_count": WINDOW})
    add("l60001_skewed_wave_steps", "skewed60001", "wave_steps", group="lanes", claims={"hl_count": WINDOW})
    add("l65537_flat_shuffled", "flat65537", "shuffled", offset=5, group="lanes")
    add("l65537_skewed_wave_steps", "skewed65537", "wave_steps", group="lanes")
    for lane in (7, 45):                # the low and the high half of the word
        add(f"l2097151_one_lane{lane}", "under2097151", "one_lane", blocks=1, last=0, group="lanes_big", bodies=("hl_count",),
            claims={"hl_count": ("max16",)}, value=200, lane=lane)

    # the chunked routes: chunks of 1 byte, block starts off alignment, empty chunks behind the short block; 64-bit sums
    add("c2097153_flat_shuffled", "flat2097153", "shuffled", blocks=2, last=3 * 262144 + 21, group="chunked", bodies=("hl_count",))
    add("c4194305_skewed_shuffled", "skewed4194305", "shuffled", blocks=1, last=21, offset=5, group="chunked", bodies=("hl_count",))

    # HUF_GPU_FUSED_HIST=1: the fused kernel above 32 KiB, packed to 128 KiB and with 32-bit counters beyond
    add("e65537_skewed_shuffled", "skewed65537", "shuffled", blocks=3, group="env", bodies=("fused_packed",),
        claims={"fused_packed": ("hot0_waves", "hot1_waves", "hot_side_bytes")})
    add("e131072_flat_shuffled", "flat131072", "shuffled", blocks=2, last=0, offset=5, group="env", bodies=("fused_packed",))
    add("e131072_wave0", "under131072", "wave0", blocks=1, last=21, group="env", bodies=("fused_packed",),
        claims={"fused_packed": ("max16", "fold_full")}, value=77)
    add("e131073_skewed_shuffled", "skewed131073", "shuffled", blocks=3, last=13009, group="env", bodies=("fused_unpacked",),
        claims={"fused_unpacked": HEADTAIL + WINDOW + ("hot0_waves", "hot1_waves", "hot_side_bytes")})
    add("e200001_skewed_wave_steps", "skewed200001", "wave_steps", blocks=2, group="env", bodies=("fused_unpacked",),
        claims={"fused_unpacked": ("fold_full", "fold_partial")})
    add("e200001_skewed_runs16", "skewed200001", "runs16", blocks=2, offset=11, group="env", bodies=("fused_unpacked",),
        claims={"fused_unpacked": ("uni_chunks", "hot0_waves", "hot_side_bytes")})
    return out


def chunk_blocks(case: Case, data: np.ndarray):
    """[(bytes, address modulo 16)] of the chunks hl_count sees on the chunked route"""
    out = []
    for b in range(-(-case.n // case.bs)):
        blk = data[b * case.bs:(b + 1) * case.bs]
        for c in range(0, blk.size, CHUNK_SYMS):
            out.append((blk[c:c + CHUNK_SYMS], (case.offset + b * case.bs + c) & 15))
    return out


# what a 16-bit counter of a body must at least reach in a case that claims max16
MAX16_AT_LEAST = 32767


# ---------------------------------------------------------------------------------------------------------------------
# the report: profiles/count_cases/sensitivity.txt
# ---------------------------------------------------------------------------------------------------------------------
def share(hist, miss: dict) -> tuple:
    """(changes not seen, changes tried) of a histogram"""
    tried = sum(1 for s in np.flatnonzero(hist) for d in DELTAS if hist[s] + d >= 1)
    return sum(len(v) for v in miss.values()), tried


def report_cases(unseen_of) -> str:
    """per case and kind of block: the share of miscounts of +-1 and +-16 the serialised tree does not show, and that
    share on the case's own symbols; unseen_of(name, hist) -> {symbol: [deltas]}"""
    lines = ["# case  block  symbols  changes not seen / tried  blind symbols  own symbols (blocks' union)  not seen on own symbols"]
    for c in cases():
        d = c.data()
        kinds = {}
        for blk, addr, hist, blind in c.block_list(d):
            k = "full" if blk.size == c.bs else "last"
            kinds.setdefault(k, [hist, blind, set()])[2].update(c.own_symbols(blk, addr))
        for k, (hist, blind, own) in kinds.items():
            miss = unseen_of(c.hname if k == "full" else "last%d" % c.last, hist)
            u, t = share(hist, miss)
            lines.append("%-28s %-4s %3d  %3d / %4d = %.3f  %-26s %3d  %d" % (
                c.name, k, int((hist > 0).sum()), u, t, u / t, ",".join(map(str, sorted(miss))) or "-", len(own),
                len(own & set(miss))))
    return "\n".join(lines) + "\n"


def report_existing() -> str:
    """the same shares for blocks of the generators the suite uses elsewhere, +-1 only: why those do not do this job"""
    from libhuffman_amd import datagen
    lines = ["# existing inputs: block  symbols  unseen at +1  unseen at -1"]
    for kind, n in (("zipf255", 65536), ("zipf255", 16384), ("logtext", 65536), ("uniform256", 65536)):
        hist = np.bincount(datagen.GENERATORS[kind](n), minlength=256).astype(np.int64)
        up, down = unseen(hist, deltas=(1,)), unseen(hist, deltas=(-1,))
        lines.append("%-10s %6d  %3d  %3d  %3d" % (kind, n, int((hist > 0).sum()), len(up), len(down)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.oracle import Oracle
    _o = Oracle()

    def _unseen_of(name, hist):
        if hist.sum() + 16 < TREE_MAX_TOTAL:
            return unseen(hist)
        return unseen_oracle(_o, hist)
    sys.stdout.write(report_cases(_unseen_of) + report_existing())

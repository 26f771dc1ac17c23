"""CPU model of the encoder's round-wise tree build, csrc/kernels/tree.hpp tree_fast_wave, walked as written: the keys in
their registers (position = lane * R + r), the compaction on entry, the `sorted` flag, sel / round_min / pairs / unp / was,
the scratch layout of a round, the optional sort of the new nodes, the half-cleaner network of wave_merge_r, the order
check behind it, the single merge that puts the new key where the smaller of the two stood, and the path doubling that
turns the links into depths, codes and preorder positions.  wave_sort_r is a sort and is modelled as one.

tree(hist) returns the serialised tree, the code lengths and the counts of the events the debug build (-DTREE_DEBUG)
counts in g_tree_dbg: EVENTS[i] is slot i.  Test infrastructure (CPU, plain Python)."""
from __future__ import annotations

KMAX = 0xffffffff
ANC_ROOT = 0x3ff
TREE_ROUND_MIN = 16
MASK32 = 0xffffffff

# slot order of g_tree_dbg (tree.hpp, TREE_DBG_*); "_rN": by the register count R the event happened at
EVENTS = (
    "blocks_r1", "blocks_r2", "blocks_r4",                      # blocks by R on entry (not the one-symbol ones)
    "one_symbol",                                               # the shortcut
    "round_sorted_r1", "round_sorted_r2", "round_sorted_r4",    # sorted rounds that had to sort
    "round_in_order_r1", "round_in_order_r2", "round_in_order_r4",   # ... that found the keys in order
    "single_r1", "single_r2", "single_r4",                      # single merges
    "r_4_2", "r_2_1", "r_4_1",                                  # a round changed R
    "nodes_in_order_r2", "nodes_in_order_r4",                   # the new nodes, by the R they go into: in order as made,
    "nodes_sorted1_r2", "nodes_sorted1_r4",                     #   sorted in one register,
    "nodes_sorted2_r2", "nodes_sorted2_r4",                     #   sorted in two,
    "nodes_chance_r1",                                          #   not looked at (into one register)
    "check_pass_r1", "check_pass_r2", "check_pass_r4",          # the order check behind the merge, by the new R
    "check_fail_r1", "check_fail_r2", "check_fail_r4",
    "wrap_root",
    "path_rounds_1", "path_rounds_2", "path_rounds_3", "path_rounds_4", "path_rounds_5", "path_rounds_6",
)
# Conditions, not measurements.  Behind a merge at R >= 2 the nodes were put in order first, so the sequence is bitonic
# by construction and the check cannot fail; paths double, so depth <= 32 is done in five rounds, and a sixth would
# mean a link that does not lead to the root.  One round is never enough: a leaf lies at least two links below the wrap
# root, and a round reads the leaves' ancestors in front of the nodes'.
NEVER = ("check_fail_r2", "check_fail_r4", "path_rounds_1", "path_rounds_6")


def half_cleaners(k: list) -> None:
    """wave_merge_r<R> over len(k) = 64 R positions: stages of distance len / 2 .. 1, the smaller key to the lower position"""
    jj = len(k) >> 1
    while jj:
        for i in range(len(k)):
            if not i & jj and k[i] > k[i | jj]:
                k[i], k[i | jj] = k[i | jj], k[i]
        jj >>= 1


def tree(hist, trace: list | None = None):
    """(serialised tree, {byte: code length}, {event: count}) of a block with these 256 counts; `trace` receives
    (R, sel, round_min, 'round' | 'single') per decision.  A fourth item holds the codes, {byte: the low 32 code bits}."""
    ev = dict.fromkeys(EVENTS, 0)
    rate = [int(x) for x in hist]
    assert len(rate) == 256 and all(0 <= x < 1 << 22 for x in rate) and sum(rate) < 1 << 22
    present = [s for s in range(256) if rate[s]]
    if len(present) == 1:
        ev["one_symbol"] += 1
        return [256, present[0], -1, -1, -1], {present[0]: 1}, ev, {present[0]: 0}
    assert present

    def key(s):
        return (rate[s] << 9) | (511 - s)

    # registers: k[lane * 4 + j] while R = 4 holds slot lane + 64 j
    live, R = len(present), 4
    if live <= 128:
        # compaction through LDS: register 0 of every lane first, then register 1 ... = ascending byte value
        R = 1 if live <= 64 else 2
        k = [key(s) for s in present] + [KMAX] * (64 * R - live)
    else:
        k = [KMAX] * 256
        for s in present:
            k[(s & 63) * 4 + (s >> 6)] = key(s)
    ev["blocks_r%d" % R] += 1

    # links: anc / depth / pos / code of a child, as tree_state() packs them
    anc, depth, pos, code, lcnt = {}, {}, {}, {}, {s: 1 for s in present}

    def make(n, x, y):
        xi, yi = 511 - (x & 511), 511 - (y & 511)
        anc[xi], depth[xi], pos[xi], code[xi] = n, 1, 1, 0
        anc[yi], depth[yi], pos[yi], code[yi] = n, 1, 4 * lcnt[xi], 1
        lcnt[n] = lcnt[xi] + lcnt[yi]
        return (((x >> 9) + (y >> 9)) << 9) | (511 - n)

    node, is_sorted = 256, False
    while True:
        if is_sorted:
            a, b = k[0], k[1]                   # (R = 1: lanes 0 and 1; R >= 2: registers 0 and 1 of lane 0)
        else:
            a = min(k)
            b = min((x for x in k if x != a), default=KMAX) if a != KMAX else KMAX
        assert a != KMAX
        if b == KMAX:
            i1 = 511 - (a & 511)
            anc[i1], depth[i1], pos[i1], code[i1] = node, 1, 1, 0
            lcnt[node] = lcnt[i1]
            root = node
            node += 1
            ev["wrap_root"] += 1
            break
        thr = (a >> 9) + (b >> 9)
        sel = sum(1 for x in k if (x >> 9) < thr)
        round_min = TREE_ROUND_MIN * R // 4
        if trace is not None:
            trace.append((R, sel, round_min, "round" if sel >= round_min else "single"))
        if sel >= round_min:
            pairs = sel >> 1
            if is_sorted:
                ev["round_in_order_r%d" % R] += 1
            else:
                k.sort()
                ev["round_sorted_r%d" % R] += 1
            for p in range(pairs):
                k[2 * p] = make(node + p, k[2 * p], k[2 * p + 1])
                k[2 * p + 1] = KMAX
            node += pairs
            was = live
            live -= pairs
            nr = 1 if live <= 64 else (2 if live <= 128 else 4)
            unp = live - pairs
            scratch = [None] * live
            for q in range(min(was, len(k))):
                if k[q] != KMAX:
                    scratch[unp + (q >> 1) if q < 2 * pairs else was - 1 - q] = k[q]
            assert None not in scratch
            if nr >= 2:
                nodes = scratch[unp:]
                if pairs <= 64:
                    if any(x > y for x, y in zip(nodes, nodes[1:])):
                        scratch[unp:] = sorted(nodes)
                        ev["nodes_sorted1_r%d" % nr] += 1
                    else:
                        ev["nodes_in_order_r%d" % nr] += 1
                else:
                    scratch[unp:] = sorted(nodes)
                    ev["nodes_sorted2_r%d" % nr] += 1
            else:
                ev["nodes_chance_r1"] += 1
            if nr != R:
                ev["r_%d_%d" % (R, nr)] += 1
            R = nr
            k = scratch + [KMAX] * (64 * R - live)
            half_cleaners(k)
            is_sorted = all(x <= y for x, y in zip(k, k[1:]))
            ev[("check_pass_r%d" if is_sorted else "check_fail_r%d") % R] += 1
            continue
        ia, ib = k.index(a), k.index(b)
        k[ia] = make(node, a, b)
        k[ib] = KMAX
        is_sorted = False
        ev["single_r%d" % R] += 1
        node += 1
        live -= 1
    anc[root], depth[root], pos[root], code[root] = ANC_ROOT, 0, 0, 0
    nodes = node
    tree_len = 4 * lcnt[root] + 1

    # paths doubled: lane l holds slots l + 64 j; per j every lane reads its ancestor's word, then every lane publishes
    have = [s for s in range(512) if (s < 256 and rate[s]) or 256 <= s < nodes]
    done = False
    for rnd in range(6):
        pending = False
        for j in range(8):
            mine = [s for s in have if s >> 6 == j and anc[s] != ANC_ROOT]
            read = {s: (anc[anc[s]], depth[anc[s]], pos[anc[s]], code[anc[s]]) for s in mine}
            for s in mine:
                ua, ud, up, uc = read[s]
                code[s] = (code[s] | (uc << (depth[s] & 31))) & MASK32       # (a 32-bit shift takes five bits of the amount)
                depth[s] += ud
                pos[s] += up
                anc[s] = ua
                pending = pending or ua != ANC_ROOT
        if not pending:
            ev["path_rounds_%d" % (rnd + 1)] += 1
            done = True
            break
    assert done, "paths not at the root after six rounds"
    tb = [None] * tree_len
    for s in have:
        tb[pos[s]] = s
        if s < 256:
            tb[pos[s] + 1] = tb[pos[s] + 2] = -1
    tb[tree_len - 1] = -1
    assert None not in tb
    return tb, {s: depth[s] for s in present}, ev, {s: code[s] for s in present}


def tree_lengths_and_codes(ent: list):
    """({byte: code length}, {byte: code}) of a serialised tree (preorder, -1 for a missing child), left = 0"""
    lens, codes = {}, {}
    stack = [(0, 0)]                                # (depth, code) of the entry that comes next
    i = 0
    while stack:
        d, c = stack.pop()
        v = ent[i]
        i += 1
        if v < 0:
            continue
        if v < 256:
            lens[v], codes[v] = d, c
            i += 2
            continue
        stack.append((d + 1, (c << 1) | 1))
        stack.append((d + 1, c << 1))
    assert i == len(ent)
    return lens, codes


def oracle_tree(oracle, data) -> list:
    """the serialised tree of the first block of the oracle's stream for `data` as one block"""
    import numpy as np
    s = oracle.encode(data, 0)
    tl = int(np.frombuffer(s[8:10].tobytes(), dtype="<i2")[0])
    return np.frombuffer(s[10:10 + 2 * tl].tobytes(), dtype="<i2").tolist()

"""Linked calls (bk_link_calls, include/breakid_hip.h) stated twice in Python, and how the command line prints a row.

expected()       the definition as it is written: every site against every other site (one numpy row of the n x n table at a time),
                 the 2 x 2 table N from the coordinates, the relation, the counts and the argmins, a union-find over the related pairs.
expected_runs()  the formulation the kernel follows: the breakends sorted, a window search per side, N of a pair collected from the hits
                 alone (never from the coordinates of the other site), each site counted at its first hit, the events as the components
                 of the graph of runs.
Both return abi.CALL_LINK rows; the tests hold them against each other and the kernel against expected()."""
import numpy as np

from breakid_amd import abi

NONE, DUPLICATE, RECIPROCAL, ADJACENT = range(4)


def as_sites(rows):
    """(tid1, pos1, right1, tid2, pos2, right2) tuples as abi.LINK_SITE rows"""
    s = np.zeros(len(rows), abi.LINK_SITE)
    for k, (t1, p1, r1, t2, p2, r2) in enumerate(rows):
        s[k]["tid1"], s[k]["pos1"], s[k]["right1"], s[k]["tid2"], s[k]["pos2"], s[k]["right2"] = t1, p1, r1, t2, p2, r2
    return s


def columns(sites):
    """tid, pos and right as (n, 2) int64 arrays"""
    tid = np.stack([sites["tid1"], sites["tid2"]], 1).astype(np.int64)
    pos = np.stack([sites["pos1"], sites["pos2"]], 1).astype(np.int64)
    right = np.stack([sites["right1"], sites["right2"]], 1).astype(np.int64)
    return tid, pos, right


def classify(N, ri, rj):
    """The relation of one pair from its table N[s][t] and the rights of the two sites, and the mappings that hold and are opposite
    (0 = straight, 1 = crossed)"""
    maps = []
    if N[0][0] and N[1][1]:
        maps.append((0, (ri[0], rj[0]), (ri[1], rj[1])))
    if N[0][1] and N[1][0]:
        maps.append((1, (ri[0], rj[1]), (ri[1], rj[0])))
    same = [m for m, a, b in maps if a[0] == a[1] and b[0] == b[1]]
    opposite = [m for m, a, b in maps if a[0] != a[1] and b[0] != b[1]]
    if same:
        return DUPLICATE, []
    if opposite:
        return RECIPROCAL, opposite
    if N[0][0] or N[0][1] or N[1][0] or N[1][1]:
        return ADJACENT, []
    return NONE, []


def relation(sites, i, j, D):
    """BK_LINK_* of the pair (i, j), straight from the definition"""
    tid, pos, right = columns(sites)
    if i == j:
        return NONE
    N = [[bool(tid[i][s] == tid[j][t] and tid[i][s] >= 0 and abs(int(pos[i][s]) - int(pos[j][t])) <= D) for t in range(2)] for s in range(2)]
    return classify(N, right[i], right[j])[0]


def mate_candidates(sites, i, D):
    """Every (sum, j, crossed, off0, off1) that site i may take its mate from: one per reciprocal partner and opposite mapping"""
    tid, pos, right = columns(sites)
    cands = []
    for j in range(len(sites)):
        if j == i:
            continue
        N = [[bool(tid[i][s] == tid[j][t] and tid[i][s] >= 0 and abs(int(pos[i][s]) - int(pos[j][t])) <= D) for t in range(2)] for s in range(2)]
        for crossed in classify(N, right[i], right[j])[1]:
            o0, o1 = int(pos[j][crossed] - pos[i][0]), int(pos[j][1 - crossed] - pos[i][1])
            cands.append((abs(o0) + abs(o1), j, crossed, o0, o1))
    return cands


class _Sets:
    def __init__(self, n):
        self.up = list(range(n))

    def find(self, a):
        while self.up[a] != a:
            self.up[a] = self.up[self.up[a]]
            a = self.up[a]
        return a

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.up[max(a, b)] = min(a, b)


def _mate_choice(cands):
    """cands: (sum, j, crossed, off0, off1); the smallest sum, then the smaller index, then straight"""
    return min(cands, key=lambda c: (c[0], c[1], c[2])) if cands else None


def _fill(out, i, dups, recips, adj, cands):
    out[i]["n_dup"], out[i]["n_recip"], out[i]["n_adj"] = len(dups), len(recips), adj
    out[i]["dup_of"] = min(dups) if dups else -1
    best = _mate_choice(cands)
    out[i]["mate"] = best[1] if best else -1
    if best:
        out[i]["mate_crossed"], out[i]["off"][0], out[i]["off"][1] = best[2], best[3], best[4]


def _events(out, sets, n):
    roots = [sets.find(i) for i in range(n)]
    smallest, size = {}, {}
    for i, r in enumerate(roots):
        smallest[r] = min(smallest.get(r, i), i)
        size[r] = size.get(r, 0) + 1
    for i, r in enumerate(roots):
        out[i]["event"], out[i]["event_size"] = smallest[r], size[r]


def expected(sites, D):
    sites = np.ascontiguousarray(sites, abi.LINK_SITE)
    n = len(sites)
    out = np.zeros(n, abi.CALL_LINK)
    tid, pos, right = columns(sites)
    sets = _Sets(n)
    for i in range(n):
        N = {}
        for s in range(2):
            for t in range(2):
                N[s, t] = (tid[:, t] == tid[i, s]) & (tid[i, s] >= 0) & (np.abs(pos[:, t] - pos[i, s]) <= D)
                N[s, t][i] = False
        dups, recips, adj, cands = [], [], 0, []
        for j in np.flatnonzero(N[0, 0] | N[0, 1] | N[1, 0] | N[1, 1]):
            j = int(j)
            rel, opposite = classify([[N[0, 0][j], N[0, 1][j]], [N[1, 0][j], N[1, 1][j]]], right[i], right[j])
            sets.join(i, j)
            if rel == DUPLICATE:
                dups.append(j)
            elif rel == RECIPROCAL:
                recips.append(j)
                for crossed in opposite:
                    o0, o1 = int(pos[j][crossed] - pos[i][0]), int(pos[j][1 - crossed] - pos[i][1])
                    cands.append((abs(o0) + abs(o1), j, crossed, o0, o1))
            else:
                adj += 1
        _fill(out, i, dups, recips, adj, cands)
    _events(out, sets, n)
    return out


def expected_runs(sites, D):
    sites = np.ascontiguousarray(sites, abi.LINK_SITE)
    n = len(sites)
    out = np.zeros(n, abi.CALL_LINK)
    tid, pos, right = columns(sites)
    ends = [(int(tid[i][s]) + 1 << 32 | int(pos[i][s]), 2 * i + s) for i in range(n) for s in range(2) if tid[i][s] >= 0]
    ends.sort()
    keys = np.array([k for k, _ in ends], np.uint64)
    vals = [v for _, v in ends]
    # runs: a new one where the contig changes or the gap exceeds D
    run_of, run = {}, -1
    for q, (k, v) in enumerate(ends):
        if q == 0 or k >> 32 != ends[q - 1][0] >> 32 or k - ends[q - 1][0] > D:
            run += 1
        run_of[v] = run
    for i in range(n):
        hits = {}  # j -> the entries (s, t) of N that a window of i found, in the order (0,0) (0,1) (1,0) (1,1) of their first
        for s in range(2):
            if tid[i][s] < 0:
                continue
            base = int(tid[i][s]) + 1 << 32
            lo = np.searchsorted(keys, np.uint64(base | max(int(pos[i][s]) - D, 0)), "left")
            hi = np.searchsorted(keys, np.uint64(base | min(int(pos[i][s]) + D, 0xFFFFFFFF)), "right")
            for q in range(lo, hi):
                j, t = vals[q] >> 1, vals[q] & 1
                if j != i:
                    hits.setdefault(j, set()).add((s, t))
        dups, recips, adj, cands = [], [], 0, []
        for j, found in hits.items():
            N = [[(s, t) in found for t in range(2)] for s in range(2)]
            rel, opposite = classify(N, right[i], right[j])
            if rel == DUPLICATE:
                dups.append(j)
            elif rel == RECIPROCAL:
                recips.append(j)
                for crossed in opposite:
                    o0, o1 = int(pos[j][crossed] - pos[i][0]), int(pos[j][1 - crossed] - pos[i][1])
                    cands.append((abs(o0) + abs(o1), j, crossed, o0, o1))
            else:
                adj += 1
        _fill(out, i, dups, recips, adj, cands)
    # the events: runs are the vertices, a site joins the runs of its two sides
    sets = _Sets(run + 1)
    for i in range(n):
        if 2 * i in run_of and 2 * i + 1 in run_of:
            sets.join(run_of[2 * i], run_of[2 * i + 1])
    smallest, size = {}, {}
    site_root = []
    for i in range(n):
        v = 2 * i if 2 * i in run_of else 2 * i + 1
        r = sets.find(run_of[v]) if v in run_of else ("alone", i)
        site_root.append(r)
        smallest[r] = min(smallest.get(r, i), i)
        size[r] = size.get(r, 0) + 1
    for i, r in enumerate(site_root):
        out[i]["event"], out[i]["event_size"] = smallest[r], size[r]
    return out


def touched(sites):
    """bk_timing_touched of the `link_calls` scope (include/breakid_hip.h)"""
    tid, _, _ = columns(np.ascontiguousarray(sites, abi.LINK_SITE))
    kept = tid[tid >= 0]
    m = len(kept)
    passes = (32 + int(kept.max() + 1).bit_length() + 7) // 8 if m else 0
    return len(sites) * 64 + m * (24 + 24 * passes)


def random_sites(rng, n, contigs=3, length=50000, D=100, p_none=0.03):
    """n sites on `contigs` contigs of `length` bases.  A third are drawn freely, one in five of those with both breakpoints on one
    spot; the others copy an earlier site and move both breakpoints by up to 2 D, flip both rights, one or none, swap the sides or
    keep them: partners of every kind, at and around the distance D.  One site in 30 loses the contig of its side 2."""
    rows = []
    for k in range(n):
        if k and rng.random() < 0.67:
            t1, p1, r1, t2, p2, r2 = rows[int(rng.integers(0, k))]
            step = [0, 1, D - 1, D, D + 1, 2 * D]
            p1 = min(max(p1 + int(rng.choice(step)) * int(rng.choice([-1, 1])), 1), length)
            p2 = min(max(p2 + int(rng.choice(step)) * int(rng.choice([-1, 1])), 1), length)
            how = int(rng.integers(0, 4))
            if how == 1:
                r1, r2 = 1 - r1, 1 - r2
            elif how == 2:
                r1 = 1 - r1
            if rng.random() < 0.4:
                t1, p1, r1, t2, p2, r2 = t2, p2, r2, t1, p1, r1
        else:
            t1, t2 = int(rng.integers(0, contigs)), int(rng.integers(0, contigs))
            p1, p2 = int(rng.integers(1, length + 1)), int(rng.integers(1, length + 1))
            r1, r2 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            if rng.random() < 0.2:  # a small event: both breakpoints on one spot, so that a partner can hold both mappings
                t2, p2 = t1, min(p1 + int(rng.choice([0, 1, D // 2, D])), length)
        if rng.random() < p_none:
            t2 = -1
        rows.append((t1, p1, r1, t2, p2, r2))
    return as_sites(rows)


# ---- how the command line prints a row ------------------------------------------------------------------------------------------------
LINK_COLUMNS = ["Lk_Event", "Lk_Size", "Lk_Dup", "Lk_Recip", "Lk_Adj", "Lk_DupOf", "Lk_Mate", "Lk_MateSide", "Lk_Off1", "Lk_Off2"]


def call_fields(c, rows):
    """The columns a *_link.txt twin adds for one abi.CALL_LINK row; rows[k] is the BK_STAGE_CLUSTERS row of site k"""
    mate = int(c["mate"])
    return ["ev%d" % rows[int(c["event"])], str(int(c["event_size"])), str(int(c["n_dup"])), str(int(c["n_recip"])), str(int(c["n_adj"])),
            "bk%d" % rows[int(c["dup_of"])] if int(c["dup_of"]) >= 0 else ".", "bk%d" % rows[mate] if mate >= 0 else ".",
            ("crossed" if int(c["mate_crossed"]) else "straight") if mate >= 0 else ".",
            str(int(c["off"][0])) if mate >= 0 else ".", str(int(c["off"][1])) if mate >= 0 else "."]


def info_fields(c, rows, side, in_file):
    """What breakend `side` (0 or 1) of a call ends its INFO with; in_file(row) says whether the records of that cluster row are in
    the same VCF"""
    s = ""
    if int(c["event_size"]) > 1:
        s += ";EVENT=ev%d" % rows[int(c["event"])]
    mate = int(c["mate"])
    if mate >= 0 and in_file(rows[mate]):
        s += ";PARID=bk%d_%d" % (rows[mate], (1 - side if int(c["mate_crossed"]) else side) + 1)
    return s

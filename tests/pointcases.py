"""Isolated-pair masking and the -fast window clustering of csrc/cluster.hip as plain Python loops, with the designed point sets at
which the kernels are pinned (tests/test_cpu_points.py checks the definitions against the oracle and that every case reaches the
edge it was built for, tests/test_gpu_points.py the kernels against the definitions, entry for entry).  No GPU import here.

The definitions follow oracle/oracle.cc (mask_pairs, remove_isolated, fast_cluster) and hold for inputs whose sort keys are distinct
(all x distinct and all y distinct within a group), so that no tie order of std::sort enters; the tie cases take their expectation
from the oracle.  Every size follows from the two constants of the build (capi.cluster_info(): FW_TILE, FW_LEVELS): the chain of
window anchors start -> nxt -> nxt ... of every group is followed in tiles of FW_TILE list positions (k_fw_exit, k_fw_chain,
k_fw_mark), so where a group, an anchor or the lost last element falls inside a tile is what a case places.

A case carries a witness: the property it exists for, computed from the plain definition's anchors and the constants."""
import numpy as np

TODAY = {"FW_TILE": 1024, "FW_LEVELS": 10}
W = 3000.0
MODES = ("mask", "iso", "fast")


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def _absdiff(a, b):
    """abs((int32)(a - b)) on uint32 operands, taken in long"""
    d = (int(a) - int(b)) & 0xFFFFFFFF
    if d >= 1 << 31:
        d -= 1 << 32
    return abs(d)


def mask_reference(x, y, dist):
    """mask_pairs_chr_pos on the points in the given order: the positions that survive, in output order.  Up to 2 points give
    nothing, the first and the last point never survive, and point 1 is first tried against point 2 alone and emitted before the
    loop emits it again."""
    n = len(x)
    out = []
    if n <= 2:
        return out
    if not (_absdiff(x[1], x[2]) > dist or _absdiff(y[1], y[2]) > dist):
        out.append(1)
    for i in range(1, n - 1):
        lx = min(_absdiff(x[i - 1], x[i]), _absdiff(x[i + 1], x[i]))
        ly = min(_absdiff(y[i - 1], y[i]), _absdiff(y[i + 1], y[i]))
        if not (lx > dist or ly > dist):
            out.append(i)
    return out


def iso_reference(x, y, w):
    """remove_isolated_pairs: sort by x, mask with (long) w, sort by y, mask, sort by x.  Point indices in output order."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    dist = int(w)  # (long) w truncates
    ids = sorted(range(len(x)), key=lambda i: x[i])
    ids = [ids[p] for p in mask_reference([x[i] for i in ids], [y[i] for i in ids], dist)]
    if ids:
        ids.sort(key=lambda i: y[i])  # (the two copies of an emitted-twice point tie, and are the same point)
        ids = [ids[p] for p in mask_reference([x[i] for i in ids], [y[i] for i in ids], dist)]
        ids.sort(key=lambda i: x[i])
    return ids


def window_pass(keys, w):
    """One anchored-window pass over ascending keys: a window takes members while key <= anchor + w (in double), the last element
    always breaks the window and is never flushed, a window with fewer than 2 members is dropped.  Returns the kept mask, the
    window ordinal of every kept element (from 1) and the positions of all anchors (the last element is always one)."""
    n = len(keys)
    kept, ordinal, anchors = [False] * n, [0] * n, []
    if n == 0:
        return kept, ordinal, anchors
    pre, members, k = int(keys[0]), [0], 1
    anchors.append(0)
    for i in range(1, n):
        if float(int(keys[i])) <= float(pre) + w and i != n - 1:
            members.append(i)
        else:
            if len(members) >= 2:
                for j in members:
                    kept[j], ordinal[j] = True, k
                k += 1
            pre, members = int(keys[i]), [i]
            anchors.append(i)
    return kept, ordinal, anchors


def _fast_steps(x, y, w):
    x, y = [int(v) for v in x], [int(v) for v in y]
    kept, k1, ax = window_pass(x, w)
    s = [i for i in range(len(x)) if kept[i]]
    s.sort(key=lambda i: y[i])
    kept2, k2, ay = window_pass([y[i] for i in s], w)
    t = [(i, k1[i], k2[p]) for p, i in enumerate(s) if kept2[p]]
    t.sort(key=lambda r: x[r[0]])
    count = {}
    for _, a, b in t:
        count[(a, b)] = count.get((a, b), 0) + 1
    ids, cl, number = [], [], {}
    for i, a, b in t:
        if count[(a, b)] >= 2:
            if (a, b) not in number:
                number[(a, b)] = len(number) + 1
            ids.append(i)
            cl.append(number[(a, b)])
    return ids, cl, ax, ay, len(s), len(t)


def fast_reference(x, y, w):
    """find_cluster_pairs_enspan_fast on x-ascending points: the pass on x, the survivors sorted by y and the pass on y, sorted by
    x, the ids k1:k2 with at least 2 members numbered from 1 by first appearance.  Returns point indices, cluster numbers, the
    anchors of the x pass (positions in the input) and of the y pass (positions among the y-sorted survivors)."""
    return _fast_steps(x, y, w)[:4]


def groups_reference(mode, x, y, group_off, w):
    """The per-group results concatenated: ids offset by the group's start, cluster numbers restarting at 1 in every group, and the
    group offsets of the result.  For mode fast also the two lists the window passes see ("passes": their group offsets and the
    list positions of all anchors; groups of fewer than 2 points are not clustered and are not in the first list)."""
    group_off = [int(v) for v in group_off]
    ids, cl, goff = [], [], [0]
    p1, p2 = {"goff": [0], "anchors": []}, {"goff": [0], "anchors": []}
    for g in range(len(group_off) - 1):
        b, e = group_off[g], group_off[g + 1]
        gx, gy = x[b:e], y[b:e]
        if mode == "mask":
            r, c = mask_reference(gx, gy, int(w)), []
        elif mode == "iso":
            r, c = iso_reference(gx, gy, w), []
        else:
            r, c, ax, ay, n1, _ = _fast_steps(gx, gy, w)
            if e - b < 2:
                ax, ay, n1 = [], [], 0
            p1["anchors"] += [p1["goff"][-1] + a for a in ax]
            p2["anchors"] += [p2["goff"][-1] + a for a in ay]
            p1["goff"].append(p1["goff"][-1] + (e - b if e - b >= 2 else 0))
            p2["goff"].append(p2["goff"][-1] + n1)
        ids += [b + i for i in r]
        cl += c if mode == "fast" else [0] * len(r)
        goff.append(len(ids))
    out = {"ids": np.asarray(ids, np.uint32), "cl": np.asarray(cl, np.int32), "goff": np.asarray(goff, np.uint64)}
    if mode == "fast":
        out["passes"] = (p1, p2)
    return out


def first_difference(got, exp):
    """index of the first entry that differs (or of the first missing one), None when equal"""
    got, exp = np.asarray(got), np.asarray(exp)
    m = min(len(got), len(exp))
    d = np.flatnonzero(got[:m] != exp[:m])
    if len(d):
        return int(d[0])
    return m if len(got) != len(exp) else None


def describe_difference(name, mode, got, exp, c=TODAY):
    """None when (ids, cl, goff) agree, else a line naming the case, the mode, the first differing output position, its group and
    its tile"""
    for field in ("ids", "cl", "goff"):
        d = first_difference(got[field], exp[field])
        if d is None:
            continue
        if field == "goff":
            return "%s / %s: group offsets differ first at group %d: got %s, expected %s" % (
                name, mode, d, got[field][d:d + 3].tolist(), exp[field][d:d + 3].tolist())
        group = int(np.searchsorted(np.asarray(exp["goff"], np.uint64), d, side="right")) - 1
        g = got[field][d] if d < len(got[field]) else "nothing"
        e = exp[field][d] if d < len(exp[field]) else "nothing"
        return "%s / %s: %s differ first at output position %d (group %d, tile %d): got %s, expected %s; counts %d / %d" % (
            name, mode, field, d, group, d // c["FW_TILE"], g, e, len(got[field]), len(exp[field]))
    return None


# ---- the builder --------------------------------------------------------------------------------------------------------------------
def from_sizes(sizes, w=W, x0=1000, ties=False):
    """Ascending distinct x whose anchored windows have exactly the listed sizes, plus one closing element: the lost last one, one
    above the last member, so it would belong to the last window but for the rule that the last element always breaks it.  Members
    are 1 apart, anchors floor(w) + 1 apart: the first key outside a window of two is exactly floor(w) away from its second member,
    so a window anchored one position late takes the wrong neighbour.  y = max(x) - x + 7: the y pass anchors from the other end
    and the ids k1:k2 split windows.
    ties: the second member of every window takes the anchor's key and the closing element the key before it (two equal keys per
    window and at the forced break), y = x // 3 (ties there too): the y order then comes from std::sort."""
    step = int(w) + 1
    x, a = [], x0
    for m in sizes:
        assert 1 <= m and m - 1 <= w, m
        x += [a + (0 if ties and j == 1 else j) for j in range(m)]
        a += step
    x.append(x[-1] + (0 if ties else 1) if x else x0)
    x = np.asarray(x, np.int64)
    y = x // 3 if ties else x.max() - x + 7
    assert x.max() < (1 << 31) and (np.diff(x) >= (0 if ties else 1)).all()
    return x.astype(np.uint32), y.astype(np.uint32)


def twos(n):
    """window sizes for n points (closing element included): windows of two, with one of three (or a lone one) where n is even"""
    if n < 2:
        return []
    m = n - 1
    if m % 2 == 0:
        return [2] * (m // 2)
    return [1] if m == 1 else [3] + [2] * ((m - 3) // 2)


def path(dx, dy, x0=500, y0=500000):
    """points from steps: x ascending by dx, y moving by dy (all of one sign, so that y is distinct)"""
    x = x0 + np.concatenate([[0], np.cumsum(np.asarray(dx, np.int64))]).astype(np.int64)
    y = y0 + np.concatenate([[0], np.cumsum(np.asarray(dy, np.int64))]).astype(np.int64)
    assert (np.diff(x) > 0).all() and ((np.diff(y) > 0).all() or (np.diff(y) < 0).all()) and y.min() >= 0
    return x.astype(np.uint32), y.astype(np.uint32)


class Case:
    def __init__(self, name, x, y, w, group_off=None, ties=False, witness="", check=None):
        self.name, self.w, self.ties = name, float(w), ties
        self.x, self.y = np.ascontiguousarray(x, np.uint32), np.ascontiguousarray(y, np.uint32)
        self.group_off = np.asarray([0, len(self.x)] if group_off is None else group_off, np.uint64)
        self.single = group_off is None
        self.witness, self._check, self._ref = witness, check, {}

    def __repr__(self):
        return self.name

    def reference(self, mode):
        """the plain definition's result (computed once)"""
        assert not self.ties
        if mode not in self._ref:
            self._ref[mode] = groups_reference(mode, self.x, self.y, self.group_off, self.w)
        return self._ref[mode]

    def holds(self, c=TODAY):
        """the witness at the constants c (the tie cases have the layout of their distinct twins: no witness of their own)"""
        return True if self._check is None else bool(self._check(self, c))


def concat(pieces):
    x = np.concatenate([np.asarray(p[0], np.uint32) for p in pieces] + [np.zeros(0, np.uint32)])
    y = np.concatenate([np.asarray(p[1], np.uint32) for p in pieces] + [np.zeros(0, np.uint32)])
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in pieces])]).astype(np.uint64)
    return x, y, off


# ---- what the witnesses are made of -------------------------------------------------------------------------------------------------
def tile_counts(anchors, n, c):
    """anchors per tile of the list"""
    t = c["FW_TILE"]
    return np.bincount(np.asarray(anchors, np.int64) // t, minlength=-(-n // t) if n else 0)


def _pass(case, k):
    p = case.reference("fast")["passes"][k]
    return p["anchors"], p["goff"][-1], p["goff"]


def full_tile(case, c, k=0):
    """some tile holds FW_TILE anchors: every position is a one-hop window, k_fw_exit needs its last doubling round to leave from the
    first position and k_fw_mark every level to reach the last one"""
    a, n, _ = _pass(case, k)
    return n > 0 and tile_counts(a, n, c).max() == c["FW_TILE"]


def skipped_tile(case, c, k=0):
    """some tile between the first and the last anchor holds none: k_fw_chain hops over it and k_fw_mark runs there without a seed"""
    a, n, _ = _pass(case, k)
    t = tile_counts(a, n, c)
    return len(t) >= 3 and (t[1:-1] == 0).any()


def start_locals(goff, c):
    """local tile positions at which the non-empty groups of a list start"""
    return {goff[g] % c["FW_TILE"] for g in range(len(goff) - 1) if goff[g + 1] > goff[g]}


def emptied_between_live(goff_before, goff_after):
    """groups that are empty in the second list, were not in the first, and have non-empty neighbours in the second"""
    size = lambda o, g: o[g + 1] - o[g]
    ng = len(goff_after) - 1
    return [g for g in range(1, ng - 1) if size(goff_before, g) and not size(goff_after, g) and size(goff_after, g - 1) and size(goff_after, g + 1)]


# ---- single-group cases (mode fast) -------------------------------------------------------------------------------------------------
def parity_trap_sizes(c=TODAY):
    t = c["FW_TILE"]
    return [(s, p) for s in (0, 1, t - 2, t - 1, t, t + 1) for p in (t // 2 + 1, t + 6)]


def one_hop_sizes(c=TODAY):
    """a tile of one-element windows at tile offset 0, live windows, then FW_TILE - 1 one-element windows and live windows again"""
    t = c["FW_TILE"]
    return [1] * t + [2, 3] * 700 + [1] * (t - 1) + [2] * 5


def one_hop_aligned_sizes(c=TODAY):
    """the same with the second run starting on a tile edge: it ends one short of the next edge, where a window of two is anchored"""
    t = c["FW_TILE"]
    mid = [2, 3] * ((3 * t) // 5)
    mid += twos(3 * t - sum(mid) + 1)
    assert sum(mid) == 3 * t
    return [1] * t + mid + [1] * (t - 1) + [2] * 5


SKIPPED_TILES = [2, 2500, 2, 1, 3000, 1, 1, 2, 1100, 2]


def _trap_check(s):
    def check(case, c):
        t = c["FW_TILE"]
        a, n, _ = _pass(case, 0)
        sizes = np.diff(a)  # (the closing element is the last anchor)
        ok = n > t and (sizes[:s] == 1).all() and (sizes[s:] == 2).all() and len(sizes) > s + t // 2
        return ok and (s < t - 1 or tile_counts(a, n, c).max() == t)
    return check


def _last_element_check(where):
    def check(case, c):
        t = c["FW_TILE"]
        a, n, _ = _pass(case, 0)
        local = (n - 1) % t
        alone = tile_counts(a, n, c)[-1] == 1
        return {"last": local == t - 1, "first": local == 0 and alone, "inside": local == t - 2}[where]
    return check


def window_edge_points(high):
    """w = 3000.75: neighbouring keys exactly floor(w) apart (inside) and floor(w) + 1 apart (outside), as the second element of a
    window and as its last admitted member, in (double)(long) key + w against (long) w; high: x reaches 2^31 - 1, else y does"""
    d = 3000
    steps = [d, d + 1,          # [a, a+d] | b
             1, d - 1, d + 1,   # [b, b+1, b+d] | c (outside by one)
             d + 1,             # [c] | e: a window of one
             d - 1, 1, d + 1,   # [e, e+d-1, e+d] | f
             d, 1,              # [f, f+d] | f+d+1 is outside of f, anchors the next
             d - 1, 2,          # [g, g+d-1] | outside by one again
             d, d, d + 1,       # every step inside a step of d, but only the first inside the anchor's window
             1, 1, d - 2, d + 1,
             2, 1]
    x = np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)
    top = (1 << 31) - 1
    if high:
        x = x + (top - x.max())
        y = x.max() - x + 7
    else:
        x = x + 11
        y = top - (x - x.min())
    return x.astype(np.uint32), y.astype(np.uint32)


def _window_edge_check(case, c):
    a, n, _ = _pass(case, 0)
    x = case.x.astype(np.int64)
    d = int(case.w)
    sizes = np.diff(a)
    inside_second = any(x[p + 1] - x[p] == d and s >= 2 for p, s in zip(a[:-1], sizes))
    inside_last = any(x[p + s - 1] - x[p] == d and s >= 3 for p, s in zip(a[:-1], sizes))
    outside_second = any(x[p + 1] - x[p] == d + 1 and s == 1 for p, s in zip(a[:-1], sizes))
    outside_last = any(x[p + s] - x[p] == d + 1 and s >= 2 for p, s in zip(a[:-1], sizes) if p + s < n)
    return case.w != d and inside_second and inside_last and outside_second and outside_last and max(int(case.x.max()), int(case.y.max())) == (1 << 31) - 1


def single_cases(c=TODAY, ties=False):
    """the single-group cases for mode fast (ties: the oracle-only twins of the parity trap and the one-hop families)"""
    t = c["FW_TILE"]
    out = []
    for s, p in parity_trap_sizes(c):
        x, y = from_sizes([1] * s + [2] * p, W, ties=ties)
        out.append(Case("parity_trap_s%d_p%d%s" % (s, p, "_ties" if ties else ""), x, y, W, ties=ties,
                        witness="%d one-element windows, then windows of two only, over more than a tile%s" % (s, "; some tile holds FW_TILE anchors" if s >= t - 1 else ""),
                        check=None if ties else _trap_check(s)))
    for name, sizes in (("one_hop", one_hop_sizes(c)), ("one_hop_aligned", one_hop_aligned_sizes(c))):
        x, y = from_sizes(sizes, W, ties=ties)
        need = 1 if name == "one_hop" else 2
        out.append(Case(name + ("_ties" if ties else ""), x, y, W, ties=ties, witness="%d tile(s) hold FW_TILE anchors, live windows behind each" % need,
                        check=None if ties else (lambda case, cc, need=need: int((tile_counts(*_pass(case, 0)[:2], cc) == cc["FW_TILE"]).sum()) >= need)))
    if ties:
        return out
    x, y = from_sizes(SKIPPED_TILES, W)
    out.append(Case("skipped_tiles", x, y, W, witness="some tile between the first and the last anchor holds none (windows longer than two tiles)",
                    check=lambda case, cc: skipped_tile(case, cc) and max(SKIPPED_TILES) > 2 * cc["FW_TILE"]))
    for n, where in ((t - 1, "inside"), (t, "last"), (t + 1, "first"), (2 * t, "last"), (2 * t + 1, "first")):
        x, y = from_sizes(twos(n), W)
        assert len(x) == n
        out.append(Case("length_%d" % n, x, y, W, witness={"inside": "the lost last element one short of a tile's last position", "last": "the lost last element is the last of a tile",
                                                           "first": "the lost last element is alone in its tile (nxt = END on a chain entry)"}[where],
                        check=_last_element_check(where)))
    x, y = from_sizes([3 * t], 4 * t)
    out.append(Case("one_window", x, y, 4 * t, witness="one window over three tiles: nxt clamps to the last element from everywhere",
                    check=lambda case, cc: _pass(case, 0)[0] == [0, 3 * cc["FW_TILE"]]))
    for n in (0, 1, 2, 3):
        x, y = from_sizes(twos(n), W) if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
        out.append(Case("degenerate_%d" % n, x, y, W, witness="%d point(s): nothing survives" % n,
                        check=lambda case, cc, n=n: len(case.x) == n and len(case.reference("fast")["ids"]) == 0))
    for high in (True, False):
        x, y = window_edge_points(high)
        out.append(Case("window_edge_%s_high" % ("x" if high else "y"), x, y, 3000.75,
                        witness="keys floor(w) and floor(w) + 1 from an anchor, as second element and as last admitted member; a key of 2^31 - 1", check=_window_edge_check))
    return out


# ---- multi-group cases (all three modes) --------------------------------------------------------------------------------------------
def _pieces(size_lists, w=W):
    """one from_sizes piece per group; a group's x starts one above the last x of the group before it, so that a kernel that looked
    across a group's end would find a close neighbour there"""
    pieces, x0 = [], 1000
    for sizes in size_lists:
        if sizes is None:
            pieces.append((np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
            continue
        x, y = from_sizes(sizes, w, x0=x0)
        pieces.append((x, y))
        x0 = int(x.max()) + 1
    return pieces


def group_sizes_on_tile_positions(c=TODAY):
    t = c["FW_TILE"]
    return [0, 1, 2, 3, t - 6, 0, 0, t, 1, t + 1, 2, 2 * t + 5, 4, 3]


def _starts_check(case, c):
    t = c["FW_TILE"]
    _, _, goff1 = _pass(case, 0)  # the list the first pass sees: groups of one point are gone
    locals_in = start_locals([int(v) for v in case.group_off], c)
    locals_1 = start_locals(goff1, c)
    ends_on_edge = any(goff1[g + 1] > goff1[g] and goff1[g + 1] % t == 0 for g in range(len(goff1) - 1))
    return {0, 1} <= locals_in and {0, t - 1} <= locals_1 and ends_on_edge


def small_group_shapes(k):
    """window sizes of 4 to 6 points, all shapes in turn"""
    shapes = [[3], [1, 2], [2, 1], [2, 2], [4], [1, 3], [3, 1], [2, 3], [3, 2], [5], [1, 2, 2], [2, 2, 1], [1, 1, 1], [1, 1, 1, 1, 1]]
    return shapes[k % len(shapes)]


def emptied_group_sizes(c=TODAY):
    """every third group holds one-element windows only; the live groups in front of the second and the third emptied group leave
    FW_TILE and 2 * FW_TILE elements to the second pass; the group of three points behind them is emptied by the second pass"""
    t = c["FW_TILE"]
    a, b = (t // 2) * 6 // 10, t // 2 - (t // 2) * 6 // 10
    live = [[2] * a, [2] * b, [3] * 50, twos(t - 150 + 1), [2] * 3, [2], [2] * (t // 2 + 88), [3] * 3]
    out = []
    for k in range(13):
        out.append([1] * (3 + k) if k % 3 == 0 else live.pop(0))
    return out


def _emptied_check(case, c):
    t = c["FW_TILE"]
    (_, _, g1), (_, _, g2) = _pass(case, 0), _pass(case, 1)
    gone = emptied_between_live(g1, g2)
    final = [int(v) for v in case.reference("fast")["goff"]]
    return len(gone) >= 3 and any(g2[g] and g2[g] % t == 0 for g in gone) and not g2[1] - g2[0] and not g2[-1] - g2[-2] and any(g2[g + 1] > g2[g] and final[g + 1] == final[g] for g in range(len(final) - 1))


def masking_groups(c=TODAY):
    """groups of 0 to 5 points next to each other (point 1 emitted twice, once, not at all; groups that masking empties), then
    groups of 2 * FW_TILE + 1 points with points more than (long) w from both neighbours in x only, in y only, in both, and controls
    exactly (long) w away.  w = 3000.75."""
    t = c["FW_TILE"]
    d, f = 3000, 3001
    small = [([], []), ([1, 1], [1, 1]), ([1, f], [1, 1]), ([f, f], [1, 1]), ([], []), ([1, 1], [-1, -f]), None, ([1], [1]), ([1, 1, 1], [-1, -1, -1]), ([f, 1, f], [1, 1, 1]),
             ([f, f, f], [1, 1, 1]), ([1, f, 1], [-1, -1, -1]), None, None, ([1, 1, 1, 1], [1, 1, 1, 1]), ([f, f, 1, 1], [-1, -1, -1, -1]), ([d, d, d, d], [-d, -d, -d, -d]),
             ([f, d, d, f], [d, d, f, f]), ([1, 1, 1, 1], [f, f, f, f]), ([1, 1], [d, d]), ([d, f], [1, 1]), ([], [])]
    pieces = []
    for s in small:
        if s is None:
            pieces.append((np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
        else:
            pieces.append(path(s[0], s[1], y0=500000))
    far = [5, 6, 400, t - 1, t, t + 1, t + 300, 2 * t - 2]
    exact = [50, t - 40, t + 40]
    for kind, sign in (("x", 1), ("y", -1), ("xy", 1), ("xy", -1)):
        dx, dy = np.ones(2 * t, np.int64), np.full(2 * t, sign, np.int64)
        for i in far:  # steps i-1 -> i and i -> i+1
            if "x" in kind:
                dx[i - 1] = dx[i] = f
            if "y" in kind:
                dy[i - 1] = dy[i] = sign * f
        for i in exact:
            dx[i - 1] = dx[i] = d
            dy[i - 1] = dy[i] = sign * d
        pieces.append(path(dx, dy, y0=500000 if sign > 0 else 500000 + 2 * t * 8 + (len(far) + len(exact)) * 2 * f))
    return pieces


def _masking_check(case, c):
    off = [int(v) for v in case.group_off]
    ref = case.reference("mask")
    ids, goff = ref["ids"].tolist(), [int(v) for v in ref["goff"]]
    twice, once, emptied = [], [], []
    for g in range(len(off) - 1):
        out = ids[goff[g]:goff[g + 1]]
        n = off[g + 1] - off[g]
        if n >= 3:
            k = out.count(off[g] + 1)
            (twice if k == 2 else once if k == 1 else emptied if not out else []).append(g)
    next_to = any(abs(a - b) == 1 for a in twice for b in once)
    iso = case.reference("iso")
    big = [g for g in range(len(off) - 1) if off[g + 1] - off[g] == 2 * c["FW_TILE"] + 1]
    sizes = {off[g + 1] - off[g] for g in range(len(off) - 1)}
    thinned = all(0 < int(iso["goff"][g + 1] - iso["goff"][g]) < 2 * c["FW_TILE"] - 8 for g in big)
    return next_to and emptied and {0, 1, 2, 3, 4, 5} <= sizes and len(big) >= 3 and thinned and case.w != int(case.w)


def multi_cases(c=TODAY):
    t = c["FW_TILE"]
    out = []
    x, y, off = concat(_pieces([twos(n) if n else None for n in group_sizes_on_tile_positions(c)]))
    assert np.diff(off).tolist() == group_sizes_on_tile_positions(c)
    out.append(Case("starts_on_tile_positions", x, y, W, off, check=_starts_check,
                    witness="groups start at local tile positions 0 and 1 in the input, at 0 and FW_TILE - 1 in the list the first pass sees, and one ends on a tile edge there"))
    for ng in (64, 65, 257):
        x, y, off = concat(_pieces([small_group_shapes(k) for k in range(ng)] + [twos(2 * t + 3)]))
        out.append(Case("small_groups_%d" % ng, x, y, W, off, witness="%d groups of 4 to 6 points, then one of 2 * FW_TILE + 3" % ng,
                        check=lambda case, cc, ng=ng: len(case.group_off) == ng + 2 and {4, 5, 6} == set(np.diff(case.group_off[:-1]).tolist())
                        and int(case.group_off[-1] - case.group_off[-2]) == 2 * cc["FW_TILE"] + 3))
    x, y, off = concat(_pieces(emptied_group_sizes(c)))
    out.append(Case("emptied_groups", x, y, W, off, check=_emptied_check,
                    witness="groups are empty after pass 1 and their neighbours are not, one of them at a tile edge of the compacted list; the first and the last group too; pass 2 empties another"))
    x, y, off = concat(masking_groups(c))
    out.append(Case("masking", x, y, 3000.75, off, check=_masking_check,
                    witness="groups of 0 to 5 points, point 1 emitted twice next to once, groups that masking empties, far points in x only / y only / both in groups of 2 * FW_TILE + 1"))
    return out


def all_cases(c=TODAY):
    return single_cases(c) + multi_cases(c)


# ---- the whole path -----------------------------------------------------------------------------------------------------------------
WHOLE_PATH_GROUPS = [(0, 1, 2100, 300, True), (0, 2, 2600, 300, True), (1, 2, 2300, 300, True), (0, 3, 1030, 200, False)]


def whole_path_dataset():
    """A record table whose chromosome-pair groups are long chains of short windows: (tid a, tid b, pairs, spacing, y descending)
    per group, pairs evenly spaced so that masking keeps all but the ends and the x windows have 5 members (7 in the short group,
    whose y ascends, so that its point 1 stays emitted twice); a few thousand proper pairs on a small contig set w (about 1326).
    Wherever the lanes cut their lists, every tile of a chain holds anchors."""
    from breakid_amd import synth
    contigs = [("chr1", 1_000_000), ("chr2", 1_000_000), ("chr3", 1_000_000), ("chr4", 1_000_000), ("chr5", 120_000)]
    ds = synth.Dataset(contigs)
    rng = np.random.default_rng(20250)
    for i in range(2200):
        ds.recs += synth._proper_pair(rng, i, 4, 1000, 119_000, 100, 350, 40)
    for g, (ta, tb, n, step, down) in enumerate(WHOLE_PATH_GROUPS):
        for k in range(n):
            pa = 10_000 + 37 * g + k * step
            pb = 900_000 - k * step if down else 20_000 + k * step
            ds.recs += synth._discordant_pair("d%d_%d" % (g, k), ta, pa, tb, pb, 100)
    ds.sort()
    return contigs, ds.to_soa()


def long_chains_of_short_windows(iso_rows, iso_off, w, c=TODAY, longest=5):
    """the groups of masked pair rows (STAGE_ISO) that exceed 2 * FW_TILE rows and have no x window above `longest` members"""
    out = []
    for g in range(len(iso_off) - 1):
        x = iso_rows["x"][int(iso_off[g]):int(iso_off[g + 1])]
        anchors = window_pass(x, w)[2]
        if len(x) > 2 * c["FW_TILE"] and max(np.diff(anchors)) <= longest:
            out.append(g)
    return out

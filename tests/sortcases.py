"""Inputs that put the std::sort replay (csrc/sortemu.hip, csrc/sortsvc.inc) on every size at which it changes its code path.
No GPU import here and no constant read from the source: every size follows from a dict of constants, `DOCUMENTED` + a stand-in
cap32 without a GPU (tests/test_cpu_sort_edges.py), capi.Context.debug_sort_info() on one (tests/test_gpu_sort_edges.py).

What decides the path of a segment is its length and the depth budget it has left (2 * floor(log2 n) of its group), so the
builder has to leave heap segments of an exact length with contents of its choice.  `adversary(m, fill)` does: a group of N keys
in which each of the D = 2 * floor(log2 N) levels of libstdc++'s introsort loop peels two or three keys off the left (the median
of first + 1, mid, last - 1 is the key at first + 1, the only key not above it sits at mid, so the Hoare scan swaps one pair and
cuts behind it), which leaves ONE heap segment, the last m positions of the group, holding `fill` in that order.  Stopped after
fewer levels it leaves a segment of chosen length and contents with budget to spare (partition nodes).  Every case claims its
heap segments; the claim is proved case by case by the oracle's probe (pyoracle.unit_sort_shape: the library's own partition
step), never by the arithmetic here.

Edges and the cases on them (`cases(c)`; names in brackets):
  F2_HB            heap in the finishing wave's own buffer / heap task pushed by the finisher      [heap_255 .. heap_257, fin_*]
  FIN_MAX          group to the finisher / to a partition node; heap pushed by a node              [heap_2047 .. heap_2049, node_*]
  HEAP_BIG_MIN     heap_small_body, narrow queue / heap_big_body (ranked entries), wide queue     [heap_4095 .. heap_4097, fill_*]
  SVC_WIDE_MIN     narrow / wide partition node                                                   [heap_16384, heap_16385, node_*]
  cap32            ranked heap all in LDS / hybrid with one, two, three leaves outside            [heap_cap32-1 .. heap_cap32+2, fill_*]
  HEAP_RANKED_MAX  ranked (hybrid) form / global heapsort down to HEAP_LARGE, then LDS            [heap_65533 .. heap_65536, heap_70001, fill_*]
  16 / 17          final / partitioned; the submit kernel's 256-thread stride                     [sizes_*]
  depth budget     2 * floor(log2 n) at n = 2^k - 1 and 2^k                                       [depth_*]
  the window sorts (two tilings of 32-element windows, groups of at most 16 elements)             [win_*]"""
import numpy as np

DOCUMENTED = {"FIN_MAX": 2048, "HEAP_BIG_MIN": 4096, "HEAP_RANKED_MAX": 65534, "HEAP_LARGE": 20000, "SVC_WIDE_MIN": 16384, "F2_HB": 256, "F2_EXT": 16,
              "HEAP_PAD": 32, "SJ_MAX_WIDE": 32, "SJ_MAX_NARROW": 32}
STAND_IN_CAP32 = 40947  # a cap32 as wide_lds_split() makes them (odd, 2 * (cap32 + 1) > 65534, 4 * (cap32 + 3) bytes fit 160 KB); an MI355X reported 40873
FILLS = ("equal", "two", "asc", "desc", "wide", "seven", "topbit", "max_last", "max_first", "distinct")
# partition nodes: rows of 64 keys per wave, TL_UNROLL (24) rows = 1536 keys per trip of a wave's count and place pass, i.e. trips
# of 6144 keys for a narrow node (4 waves) and 24576 for a wide one (16 waves) behind the pivot: nodes of 1 + that, and one less and more
NODE_LENGTHS = (2049, 2050, 6144, 6145, 6146, 12289, 16384, 16385, 24576, 24577, 24578)
WINDOW_TOTALS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 255, 256, 257, 272, 273)


def depth_budget(n):
    return 2 * (int(n).bit_length() - 1)


def fill(name, m, lo, seed=0):
    """m keys >= lo in heap-segment order"""
    rng = np.random.default_rng([seed, m, FILLS.index(name)])
    if name == "equal":
        v = np.full(m, lo + 5, np.int64)
    elif name == "two":
        v = lo + 1 + 8 * rng.integers(0, 2, m)
    elif name == "asc":
        v = lo + np.arange(m, dtype=np.int64)
    elif name == "desc":
        v = lo + m - 1 - np.arange(m, dtype=np.int64)
    elif name == "wide":
        v = rng.integers(lo, 1 << 32, m)
    elif name == "seven":
        v = lo + 11 * rng.integers(0, 7, m)
    elif name == "topbit":  # all distinct, top bit set, both ends of the range present
        v = 0x80000000 + 1 + np.arange(m, dtype=np.int64) * ((0x7FFFFFFE - 1) // max(m, 1))
        v[0], v[-1] = 0x80000000, 0xFFFFFFFF
        v = rng.permutation(v)
    elif name in ("max_last", "max_first"):  # the largest key exactly once, at the end the pops reach last / first
        v = lo + 11 * rng.integers(0, 7, m)
        v[-1 if name == "max_last" else 0] = 0xFFFFFFF0
    elif name == "distinct":  # m ranks
        v = lo + 3 * rng.permutation(m).astype(np.int64)
    else:
        raise KeyError(name)
    assert len(v) == m and v.min() >= lo and v.max() < (1 << 32)
    return v.astype(np.uint32)


def peel(n, levels, n3=0):
    """The peel plan on n slots: `levels` levels, the first n3 of them peel three keys, the others two.  Returns (val, rest):
    val[slot] = the key a level assigned (every other key must be >= 3 * levels + 3), rest = the slots of the segment left over,
    in the order the partitions leave them."""
    arr, val, first = list(range(n)), {}, 0
    for i in range(levels):
        mid = first + (n - first) // 2
        three = i < n3
        assert mid > first + (2 if three else 1), (n, levels, i)
        assert arr[first + 1] not in val and arr[mid] not in val and arr[first] not in val
        val[arr[first + 1]] = 3 * i + 2
        val[arr[mid]] = 3 * i + 1
        arr[first], arr[first + 1] = arr[first + 1], arr[first]
        if three:
            val[arr[first + 1]] = 3 * i  # (the slot that was at `first`)
            arr[first + 2], arr[mid] = arr[mid], arr[first + 2]
            first += 3
        else:
            arr[first + 1], arr[mid] = arr[mid], arr[first + 1]
            first += 2
    return val, arr[first:]


def adversary_size(m, levels=None):
    """the smallest group size N that leaves m elements after `levels` (default: all 2 * floor(log2 N)) levels -> (N, levels, n3)"""
    n = m + 1
    while True:
        lv = depth_budget(n) if levels is None else levels
        n3 = n - m - 2 * lv
        if 0 <= n3 <= lv <= depth_budget(n):
            return n, lv, n3
        n += 1
        assert n < m + 400, (m, levels)


def place(n, levels, n3, contents, base=0):
    """keys of the n slots: the plan's keys + base, `contents` (all >= base + 3 * levels + 3) on the left-over segment in order"""
    val, rest = peel(n, levels, n3)
    assert len(rest) == len(contents) and int(np.min(contents)) >= base + 3 * levels + 3
    key = np.zeros(n, np.uint32)
    for slot, v in val.items():
        key[slot] = base + v
    key[np.asarray(rest, np.int64)] = contents
    return key


def adversary(m, fill_name, levels=None, seed=0):
    """One group -> (keys, [(first, length)] of the heap segments it claims, relative to the group).  levels=None: every level
    peels, one heap segment [N - m, N) holding fill(fill_name) in that order.  levels=j: stopped after j levels, the segment
    [N - m, N) arrives with budget left and nothing is claimed to reach a heapsort (fills whose partitions stay balanced)."""
    n, lv, n3 = adversary_size(m, levels)
    key = place(n, lv, n3, fill(fill_name, m, 3 * lv + 3, seed))
    return key, ([(n - m, m)] if levels is None else [])


def no_swap_node(n, seed=0):
    """a node whose first partition swaps nothing: the pivot (at first + 1) is above the left two thirds and below the rest"""
    rng = np.random.default_rng([seed, n])
    c = 2 * n // 3
    key = np.concatenate([rng.integers(0, 1000, c), rng.integers(2000, 3000, n - c)]).astype(np.uint32)
    key[1] = 1500
    return key


def node_contents(name, n, seed=0):
    rng = np.random.default_rng([seed, n, 77])
    if name == "noswap":
        return no_swap_node(n, seed)
    if name == "equal":
        return np.full(n, 7, np.uint32)
    if name == "sorted":
        return np.arange(n, dtype=np.uint32) * 2
    if name == "reversed":
        return (np.arange(n, dtype=np.uint32) * 2)[::-1].copy()
    if name == "two":
        return (3 + 4 * rng.integers(0, 2, n)).astype(np.uint32)
    raise KeyError(name)


NODE_CONTENTS = ("noswap", "equal", "sorted", "reversed", "two")


def finisher_three_heaps(n=1400, seed=0):
    """One group of at most FIN_MAX keys whose finisher task leaves three heap tasks: two balanced levels that swap nothing (the
    median is the smallest key of the block that starts at mid) over three blocks, each an adversary for the budget that is left.
    Returns (keys, claimed segments)."""
    d = depth_budget(n)
    mid = n // 2
    f = mid + 1
    midp = f + (n - f) // 2
    len_a, len_c, len_d = mid + 1, midp + 1 - f, n - midp - 1
    key = np.zeros(n, np.uint32)
    claims = []
    # block A (left of the first cut, budget d - 1): arrives as [the pivot of level 0, A[1:], A[0]]
    base_a, base_c, base_d = 0, 100000, 200000
    for name, ln, lv, base, top in (("a", len_a, d - 1, base_a, base_c), ("c", len_c, d - 2, base_c + 1, base_d), ("d", len_d, d - 2, base_d + 1, None)):
        m = ln - 2 * lv
        val, rest = peel(ln, lv, 0)
        q = np.zeros(ln, np.int64)
        for slot, v in val.items():
            q[slot] = base + v
        q[np.asarray(rest, np.int64)] = fill("seven", m, base + 3 * lv + 3, seed)
        if name == "a":
            assert 0 in rest  # (slot 0 is free: it holds the pivot the level above left there, the block's largest key)
            key[0], key[1:mid], key[mid] = q[-1], q[1:-1], top
            claims.append((len_a - m, m))
        elif name == "c":
            assert 0 in rest
            key[mid + 1], key[mid + 2:midp], key[midp] = q[-1], q[1:-1], top
            claims.append((f + len_c - m, m))
        else:
            key[midp + 1:] = q
            claims.append((n - m, m))
    return key, claims


class Case:
    def __init__(self, name, groups, claims):
        """groups: key arrays; claims: None (nothing claimed) or a list of (group number, first inside it, length)"""
        self.name = name
        self.key = np.concatenate([np.asarray(g, np.uint32) for g in groups]) if groups else np.zeros(0, np.uint32)
        self.off = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
        self.claims = None if claims is None else sorted((int(self.off[g]) + f, m) for g, f, m in claims)


def _pad(k, seed=0):
    """small groups in front: what follows starts at an odd offset that is no multiple of 64"""
    rng = np.random.default_rng([seed, k])
    return [rng.integers(0, 3, s).astype(np.uint32) for s in ((5, 0, 8), (13,), (1, 16, 2), (0, 7))[k % 4]]


def _one(name, m, fill_name, pad, levels=None, seed=0):
    front = _pad(pad, seed)
    key, segs = adversary(m, fill_name, levels, seed)
    return Case(name, front + [key], [(len(front), f, ln) for f, ln in segs])


def heap_sizes(c):
    cap = c["cap32"]
    edge = [17, c["F2_HB"] - 1, c["F2_HB"], c["F2_HB"] + 1, c["FIN_MAX"] - 1, c["FIN_MAX"], c["FIN_MAX"] + 1, c["HEAP_BIG_MIN"] - 1, c["HEAP_BIG_MIN"],
            c["HEAP_BIG_MIN"] + 1, c["SVC_WIDE_MIN"], c["SVC_WIDE_MIN"] + 1, cap - 1, cap, cap + 1, cap + 2, c["HEAP_RANKED_MAX"] - 1, c["HEAP_RANKED_MAX"],
            c["HEAP_RANKED_MAX"] + 1, c["HEAP_RANKED_MAX"] + 2, 70001]
    return sorted(set(edge))


def fill_sizes(c):
    return [c["HEAP_BIG_MIN"], c["HEAP_BIG_MIN"] + 1, c["cap32"], c["cap32"] + 1, c["HEAP_RANKED_MAX"], c["HEAP_RANKED_MAX"] + 1]


def heap_cases(c):
    return [_one("heap_%d" % m, m, ("seven", "wide", "two")[k % 3], k, seed=k) for k, m in enumerate(heap_sizes(c))]


def fill_cases(c):
    return [_one("fill_%s_%d" % (name, m), m, name, j + k, seed=1) for k, m in enumerate(fill_sizes(c)) for j, name in enumerate(FILLS)]


def flight_cases(c):
    """a heap of every class in one call, and the same groups in reverse order"""
    cap = c["cap32"]
    sizes = [17, c["F2_HB"], c["F2_HB"] + 1, c["FIN_MAX"], c["FIN_MAX"] + 1, c["HEAP_BIG_MIN"], c["HEAP_BIG_MIN"] + 1, c["SVC_WIDE_MIN"] + 1, cap, cap + 1,
             c["HEAP_RANKED_MAX"], c["HEAP_RANKED_MAX"] + 1, 70001]
    built = [adversary(m, ("seven", "equal", "wide")[k % 3], seed=40 + k) for k, m in enumerate(sizes)]
    out = []
    for name, order in (("flight_up", list(range(len(built)))), ("flight_down", list(range(len(built)))[::-1])):
        groups, claims = _pad(1), []
        for k in order:
            groups.append(built[k][0])
            claims += [(len(groups) - 1, f, ln) for f, ln in built[k][1]]
            groups.append(np.full(3, 1, np.uint32))
        out.append(Case(name, groups, claims))
    return out


DEPTH_K = (5, 11, 12, 15, 16)


def depth_pair(k):
    """groups of 2^k - 1 and 2^k keys with one peel plan: 2 (k - 1) levels of two keys each, then all-equal keys.  The smaller
    group's budget is used up there (one heap segment: the rest), the larger one has two levels left (the all-equal rest is halved
    twice first).  At k = 5 the rest holds 15 and 16 keys: the budget cannot bind."""
    lv = 2 * (k - 1)
    out = []
    for n in ((1 << k) - 1, 1 << k):
        m = n - 2 * lv
        out.append(place(n, lv, 0, fill("equal", m, 3 * lv + 3)))
    return out


def depth_cases(c):
    out = []
    for k in DEPTH_K:
        small, large = depth_pair(k)
        rest = len(small) - 4 * (k - 1)
        out.append(Case("depth_%d_small" % k, _pad(k) + [small], [(len(_pad(k)), len(small) - rest, rest)] if rest > 16 else []))
        out.append(Case("depth_%d_large" % k, _pad(k + 1) + [large], None))
    return out


def size_cases(c):
    rng = np.random.default_rng(9)
    sizes = [0, 1, 2, 15, 16, 17, 18, 32, 33]
    out = [Case("sizes_neighbours", [rng.integers(0, 4, s).astype(np.uint32) for s in sizes + sizes[::-1]], [])]
    for g in (255, 256, 257):
        out.append(Case("sizes_%dx17" % g, [rng.integers(0, 3, 1).astype(np.uint32)] + [rng.integers(0, 3, 17).astype(np.uint32) for _ in range(g)], []))
    return out


def node_cases(c):
    out = []
    fin, wide = c["FIN_MAX"], c["SVC_WIDE_MIN"]
    lengths = sorted(set([fin, fin + 1, fin + 2, wide, wide + 1]) | {n for n in NODE_LENGTHS})
    for k, n in enumerate(lengths):
        # one call per length: a group of every kind of contents (each group is its own root node, or the finisher's at FIN_MAX)
        out.append(Case("node_%d" % n, _pad(k) + [node_contents(name, n, k) for name in NODE_CONTENTS], []))
    for m in (wide, wide + 1):
        # the same lengths reached from above: a wide workgroup carries a node on while it holds more than SVC_WIDE_MIN keys
        for name in ("equal", "asc", "desc", "two"):
            out.append(_one("node_carried_%d_%s" % (m, name), m, name, m & 3, levels=4, seed=3))
    return out


def finisher_cases(c):
    out = [_one("fin_heap_%d" % m, m, "seven", m & 3, seed=5) for m in (c["F2_HB"], c["F2_HB"] + 1)]
    key, claims = finisher_three_heaps(1400)
    assert len(key) <= c["FIN_MAX"]
    out.append(Case("fin_three_heaps", _pad(2) + [key], [(len(_pad(2)), f, m) for f, m in claims]))
    out.append(Case("fin_equal_%d" % c["FIN_MAX"], _pad(3) + [np.full(c["FIN_MAX"], 9, np.uint32)], []))
    return out


def window_split(n, s):
    """group sizes of at most 16 that add up to n: the first holds s, then 16 each (borders at s + 16 k: s = 1 .. 16 puts one on
    every offset of a 32-element window of both tilings); s = 0: sizes 1, 2, .. 16, 0, 1, .."""
    sizes, left = [], n
    if s:
        sizes.append(min(s, left))
        left -= sizes[-1]
        while left:
            sizes.append(min(16, left))
            left -= sizes[-1]
    else:
        k = 1
        while left:
            sizes.append(min(k % 17, left))
            left -= sizes[-1]
            k += 1
    return sizes


def window_case(n, s):
    """later groups hold smaller keys than earlier ones, three values per group (heavy ties), and the last group ends in a run of
    0xFFFFFFFF keys (next to the padding key of the lanes beyond n)"""
    rng = np.random.default_rng([n, s])
    sizes = window_split(n, s)
    groups = [(4 * (len(sizes) - g) + rng.integers(0, 3, sz)).astype(np.uint32) for g, sz in enumerate(sizes)]
    last = max(g for g, sz in enumerate(sizes) if sz)
    groups[last][len(groups[last]) // 2:] = 0xFFFFFFFF
    return Case("win_%d_%d" % (n, s), groups, [])


def window_cases(c):
    out, seen = [], set()
    for n in WINDOW_TOTALS:
        for s in range(17):
            sizes = tuple(window_split(n, s))
            if (n, sizes) not in seen:  # (small totals: several s give one split)
                seen.add((n, sizes))
                out.append(window_case(n, s))
    return out


FAMILIES = (("heap", heap_cases), ("fill", fill_cases), ("flight", flight_cases), ("depth", depth_cases), ("sizes", size_cases), ("node", node_cases),
            ("fin", finisher_cases), ("win", window_cases))


def cases(c, families=None):
    out = []
    for name, make in FAMILIES:
        if families is None or name in families:
            out += make(c)
    assert len({k.name for k in out}) == len(out)
    return out


def expected_heaps(segments, c):
    """What the task dispatch's job counts (SvcJob::max_heap, n_heap) for a sort whose heap segments are `segments`: a segment is
    counted when it leaves as a heap TASK - pushed by a partition node (every depth-0 segment it holds has more than FIN_MAX keys)
    or by the finisher (a depth-0 sub-segment of more than F2_HB keys; smaller ones are heapsorted in the wave's own buffer) - so
    exactly the segments of more than F2_HB keys count."""
    tasks = [m for _, m in segments if m > c["F2_HB"]]
    return (max(tasks) if tasks else 0), sum(tasks)

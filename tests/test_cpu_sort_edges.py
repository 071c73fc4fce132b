"""The cases of tests/sortcases.py without a GPU, at the documented constants and a stand-in cap32: every case sits on the edge it
names - the heap segments the oracle's probe finds (pyoracle.unit_sort_shape: libstdc++'s own partition step on a copy) are
exactly the ones the builder claims - the oracle's permutation is a permutation that sorts, the fills are what they are called,
and the hooks are exported, bound, declared and documented."""
import os
import re

import numpy as np
import pytest

from breakid_amd import capi
from oracle import pyoracle
from tests import sortcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")
C = dict(sc.DOCUMENTED, cap32=sc.STAND_IN_CAP32)


def test_hook_exported_bound_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "bk_debug_sort_info" in capi.EXPORTS and hasattr(capi.lib(), "bk_debug_sort_info") and callable(capi.Context.debug_sort_info)
    assert re.search(r"^int bk_debug_sort_info\(", header, re.M)
    assert hasattr(pyoracle.lib(), "ora_unit_sort_shape")
    item = design[design.index("The std::sort replay at its edges"):]
    for word in ("bk_debug_sort_info", "unit_sort_shape", "cap32", "n_heap") + tuple(sc.DOCUMENTED):
        assert word in item, word
    assert capi.Context.SORT_INFO[:10] == tuple(sc.DOCUMENTED) and capi.Context.SORT_INFO[10:] == ("cap32", "max_heap", "n_heap")


def test_documented_constants_are_the_source_s():
    """the CPU cases stand on the constants the build has today (a change moves DOCUMENTED with it; the GPU test asks the library)"""
    text = open(os.path.join(CSRC, "sortemu.hip")).read() + open(os.path.join(CSRC, "sortsvc.inc")).read()
    for name, v in sc.DOCUMENTED.items():
        assert re.search(r"constexpr uint32_t (?:\w+ = \d+, )?%s = %d[;,]" % (name, v), text), name
    cap = sc.STAND_IN_CAP32
    assert cap & 1 and 2 * (cap + 1) > sc.DOCUMENTED["HEAP_RANKED_MAX"] and 4 * (cap + 3) <= 160 * 1024


def test_the_probe_lists_what_the_statistics_count():
    rng = np.random.default_rng(3)
    key, _ = sc.adversary(300, "seven")
    parts = [rng.integers(0, 50, 40).astype(np.uint32), key, np.zeros(0, np.uint32), sc.adversary(17, "equal")[0]]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    segs = pyoracle.unit_sort_shape(np.concatenate(parts), off)
    assert segs == [(40 + len(key) - 300, 300), (int(off[3]) + 37 - 17, 17)]
    assert pyoracle.unit_sort_shape(np.zeros(0, np.uint32), np.zeros(1, np.uint64)) == []
    assert pyoracle.unit_sort_shape(rng.integers(0, 9, 5000).astype(np.uint32), np.array([0, 5000], np.uint64)) == []


def test_adversary_sizes_of_the_recipe():
    """the group sizes the recipe gives for the heap sizes on the constants (all levels peel two keys: N = m + 2 D)"""
    table = {17: 37, 18: 38, 255: 287, 256: 288, 257: 289, 2047: 2091, 2048: 2092, 2049: 2093, 4095: 4143, 4096: 4144, 4097: 4145, 16384: 16440, 16385: 16441,
             40945: 41005, 40947: 41007, 40948: 41008, 65533: 65597, 65534: 65598, 65535: 65599, 65536: 65600, 70001: 70065}
    for m, n in table.items():
        assert sc.adversary_size(m)[0] == n, m
    assert sc.adversary_size(16384, 4) == (16392, 4, 0)
    assert set(table) >= {m for m in sc.heap_sizes(C) if m not in (40946, 40949)}


@pytest.mark.parametrize("name", sc.FILLS)
def test_every_fill_reaches_the_ranked_and_the_hybrid_heap(name):
    for m in (C["HEAP_BIG_MIN"] + 1, C["cap32"] + 1):
        key, claim = sc.adversary(m, name, seed=2)
        off = np.array([0, len(key)], np.uint64)
        assert pyoracle.unit_sort_shape(key, off) == claim == [(len(key) - m, m)], (name, m)
        n, lv, n3 = sc.adversary_size(m)
        seg = key[np.asarray(sc.peel(n, lv, n3)[1])].astype(np.int64)  # the keys the levels leave on [N - m, N), in that order
        assert n == len(key) and np.array_equal(seg, sc.fill(name, m, 3 * lv + 3, 2))
        u = np.unique(seg)
        want = {"equal": len(u) == 1, "two": len(u) == 2, "asc": (np.diff(seg) > 0).all(), "desc": (np.diff(seg) < 0).all(), "wide": len(u) > m * 0.99 and seg.max() > 1 << 31,
                "seven": len(u) == 7, "topbit": len(u) == m and seg.min() == 0x80000000 and seg.max() == 0xFFFFFFFF,
                "max_last": seg[-1] == seg.max() and (seg == seg.max()).sum() == 1, "max_first": seg[0] == seg.max() and (seg == seg.max()).sum() == 1,
                "distinct": len(u) == m}[name]
        assert want, (name, m)
    assert len(np.unique(sc.fill("distinct", C["HEAP_RANKED_MAX"], 99))) == C["HEAP_RANKED_MAX"]  # the largest rank + 1 is 65534


@pytest.fixture(scope="module")
def all_cases():
    return sc.cases(C)


def test_every_case_sits_on_its_edge(all_cases):
    names = {k.name for k in all_cases}
    cap = C["cap32"]
    for m in (17, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 16384, 16385, cap - 1, cap, cap + 1, cap + 2, 65533, 65534, 65535, 65536, 70001):
        assert "heap_%d" % m in names
    for m in (4096, 4097, cap, cap + 1, 65534, 65535):
        for f in sc.FILLS:
            assert "fill_%s_%d" % (f, m) in names
    for k in all_cases:
        segs = sorted(pyoracle.unit_sort_shape(k.key, k.off))
        if k.claims is not None:
            assert segs == k.claims, (k.name, segs[:4], k.claims[:4])
        if k.name.startswith(("heap_", "fill_", "fin_heap_")):
            m = int(k.name.rsplit("_", 1)[1])
            assert segs == [(len(k.key) - m, m)] and int(k.off[-2]) % 64 and int(k.off[-2]) % 2, k.name  # one heap of exactly m keys, at an odd offset
        if k.name.startswith("win_"):
            assert max(np.diff(k.off.astype(np.int64))) <= 16 and segs == []


def test_the_oracle_s_order_is_a_sorting_permutation(all_cases):
    for k in all_cases:
        perm = pyoracle.unit_std_sort(k.key, k.off)
        assert np.array_equal(np.sort(perm), np.arange(len(k.key), dtype=np.uint32)), k.name
        for g in range(len(k.off) - 1):
            a, b = int(k.off[g]), int(k.off[g + 1])
            assert ((perm[a:b] >= a) & (perm[a:b] < b)).all() and (np.diff(k.key[perm[a:b]].astype(np.int64)) >= 0).all(), (k.name, g)


def test_several_heaps_in_flight(all_cases):
    by = {k.name: k for k in all_cases}
    up, down = by["flight_up"], by["flight_down"]
    cap = C["cap32"]
    for k in (up, down):
        assert sorted(m for _, m in k.claims) == [17, 256, 257, 2048, 2049, 4096, 4097, 16385, cap, cap + 1, 65534, 65535, 70001]
    assert [m for _, m in up.claims] == [m for _, m in down.claims][::-1]
    assert sc.expected_heaps(up.claims, C) == (70001, sum(m for _, m in up.claims) - 17 - 256)


@pytest.mark.parametrize("k", sc.DEPTH_K)
def test_depth_budget_at_powers_of_two(k):
    """2^k - 1 keys have 2 (k - 1) levels, 2^k keys two more: with one peel plan the smaller group's rest is ONE heap segment, the
    larger group's rest is partitioned twice more first (all-equal keys: halved), so its heap segments are shorter and several"""
    small, large = sc.depth_pair(k)
    assert (len(small), len(large)) == ((1 << k) - 1, 1 << k)
    assert sc.depth_budget(len(small)) == 2 * (k - 1) and sc.depth_budget(len(large)) == 2 * k
    s = pyoracle.unit_sort_shape(small, np.array([0, len(small)], np.uint64))
    g = pyoracle.unit_sort_shape(large, np.array([0, len(large)], np.uint64))
    rest = len(small) - 4 * (k - 1)
    if k == 5:
        assert rest == 15 and s == [] and g == []  # the budget cannot bind: two keys a level leave at most 16
        return
    assert s == [(len(small) - rest, rest)]
    assert len(g) == 4 and all(f >= 4 * (k - 1) for f, _ in g) and max(m for _, m in g) <= (rest + 1) // 4 + 2 and sum(m for _, m in g) >= rest - 3


def test_partition_node_and_finisher_cases(all_cases):
    by = {k.name: k for k in all_cases}
    fin, wide = C["FIN_MAX"], C["SVC_WIDE_MIN"]
    for n in (fin, fin + 1, fin + 2, wide, wide + 1) + sc.NODE_LENGTHS:
        k = by["node_%d" % n]
        sizes = np.diff(k.off.astype(np.int64))
        assert list(sizes[-len(sc.NODE_CONTENTS):]) == [n] * len(sc.NODE_CONTENTS)
    # a no-swap node: the library's first partition of it moves nothing but the pivot
    key = sc.no_swap_node(6145)
    assert int(key[1]) == 1500 and (key[:2 * 6145 // 3] < 1500).sum() == 2 * 6145 // 3 - 1 and (key[2 * 6145 // 3:] > 1500).all()
    for m in (wide, wide + 1):
        n, lv, n3 = sc.adversary_size(m, 4)
        assert (lv, n3) == (4, 0) and n == m + 8 and n > wide  # the root is a wide node, four levels later m keys are left
        # ... which the same plan carried on to the end proves: whatever the keys of the rest, every level peels its two
        full, claim = sc.adversary(m, "seven")
        assert pyoracle.unit_sort_shape(full, np.array([0, len(full)], np.uint64)) == claim
    three = by["fin_three_heaps"]
    assert len(three.claims) == 3 and all(m > C["F2_HB"] for _, m in three.claims) and np.diff(three.off.astype(np.int64))[-1] <= fin
    assert sc.expected_heaps(three.claims, C)[1] == sum(m for _, m in three.claims)
    assert sc.expected_heaps(by["fin_heap_256"].claims, C) == (0, 0) and sc.expected_heaps(by["fin_heap_257"].claims, C) == (257, 257)
    assert np.diff(by["fin_equal_2048"].off.astype(np.int64))[-1] == fin and len(np.unique(by["fin_equal_2048"].key[-fin:])) == 1


def test_window_cases_cover_every_border_offset():
    for n in sc.WINDOW_TOTALS:
        borders = set()
        for s in range(17):
            k = sc.window_case(n, s)
            sizes = np.diff(k.off.astype(np.int64))
            assert sizes.sum() == n and sizes.max() <= 16
            borders |= {int(b) % 32 for b in k.off[1:-1]}
            # later groups hold smaller keys (but for the run of 0xFFFFFFFF that ends the last group with any keys)
            tops = [int(k.key[int(a):int(b)].max()) for a, b in zip(k.off[:-1], k.off[1:]) if b > a]
            assert tops[-1] == 0xFFFFFFFF or n == 1
            assert all(x > y for x, y in zip(tops[:-2], tops[1:-1]))
            if n >= 4:
                assert int(k.key[-1]) == 0xFFFFFFFF
        assert borders >= set(range(min(32, n))) - {0} or n <= 32 and borders >= set(range(1, n)), (n, sorted(borders))

"""The masking and fast-clustering definitions of tests/pointcases.py without a GPU: against the oracle (oracle/oracle.cc, the port of
the reference's functions) on every designed case, group by group, that every case reaches the edge it was built for at today's
constants, and that the hooks are exported, bound, declared and documented."""
import os
import re

import numpy as np
import pytest

from breakid_amd import capi
from oracle import pyoracle
from tests import pointcases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")
HOOKS = ("bk_debug_points_groups", "bk_debug_cluster_info")

CASES = pc.all_cases()
TIES = pc.single_cases(ties=True)


def _built():
    return os.path.exists(capi.LIB_PATH)


def test_hooks_exported_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("Test hooks of the C ABI"):]
    item = item[:item.index("\n* ")]
    for name in HOOKS:
        assert name in capi.EXPORTS, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in item, name
        if _built():
            assert hasattr(capi.lib(), name), name
    assert callable(capi.Context.debug_points_groups) and callable(capi.cluster_info)
    assert "tests/test_gpu_points.py" in item


def test_constants_of_the_build():
    src = open(os.path.join(CSRC, "cluster.h")).read()
    assert re.search(r"constexpr uint32_t FW_TILE = %d, FW_LEVELS = %d;" % (pc.TODAY["FW_TILE"], pc.TODAY["FW_LEVELS"]), src)
    assert "static_assert((1ull << FW_LEVELS) >= FW_TILE" in src
    assert "FW_TILE =" not in open(os.path.join(CSRC, "cluster.hip")).read()
    assert 1 << pc.TODAY["FW_LEVELS"] == pc.TODAY["FW_TILE"]  # exactly enough: the one-hop tiles need every level
    if _built():  # (otherwise TODAY was compared with the source only)
        assert capi.cluster_info() == pc.TODAY  # a change of the tile moves every case with it: update TODAY


def test_case_names_and_sizes():
    names = [c.name for c in CASES + TIES]
    assert len(names) == len(set(names))
    t = pc.TODAY["FW_TILE"]
    by = {c.name: c for c in CASES + TIES}
    assert [len(by["parity_trap_s%d_p%d" % sp].x) for sp in ((0, 513), (1025, 1030))] == [1027, 3086]
    assert len(by["one_hop"].x) == 5558 and len(by["one_hop_aligned"].x) == 5 * t + 10 and len(by["skipped_tiles"].x) == 6612
    assert len(by["one_window"].x) == 3 * t + 1
    assert {len(by["length_%d" % n].x) for n in (t - 1, t, t + 1, 2 * t, 2 * t + 1)} == {t - 1, t, t + 1, 2 * t, 2 * t + 1}
    assert [len(by["degenerate_%d" % n].x) for n in range(4)] == [0, 1, 2, 3]
    assert max(len(c.x) for c in CASES + TIES) < 12000
    assert len(TIES) == 14 and all(c.ties and c.single for c in TIES)
    assert np.diff(by["starts_on_tile_positions"].group_off).tolist() == [0, 1, 2, 3, t - 6, 0, 0, t, 1, t + 1, 2, 2 * t + 5, 4, 3]
    # the sizes move with the constants
    wide = {"FW_TILE": 2048, "FW_LEVELS": 11}
    assert max(len(c.x) for c in pc.single_cases(wide)) == 5 * 2048 + 10
    assert all(c.holds(wide) for c in pc.all_cases(wide) if c.name in ("one_hop", "one_hop_aligned", "parity_trap_s2048_p2054", "length_2049", "starts_on_tile_positions", "emptied_groups"))


def test_sort_keys_are_distinct_where_the_plain_definitions_are_used():
    for c in CASES:
        off = [int(v) for v in c.group_off]
        for g in range(len(off) - 1):
            x, y = c.x[off[g]:off[g + 1]], c.y[off[g]:off[g + 1]]
            assert len(np.unique(x)) == len(x) and len(np.unique(y)) == len(y), (c.name, g)
            assert (np.diff(x.astype(np.int64)) > 0).all(), (c.name, g)  # mode fast takes its list x-sorted
    for c in TIES:
        assert (np.diff(c.x.astype(np.int64)) >= 0).all() and len(np.unique(c.x)) < len(c.x) and len(np.unique(c.y)) < len(c.y), c.name


def _oracle_groups(mode, c):
    off = [int(v) for v in c.group_off]
    ids, cl, goff = [], [], [0]
    for g in range(len(off) - 1):
        i, k, _ = pyoracle.unit_points(mode, c.x[off[g]:off[g + 1]], c.y[off[g]:off[g + 1]], c.w)
        ids += [off[g] + int(v) for v in i]
        cl += [int(v) for v in k] if mode == "fast" else [0] * len(i)
        goff.append(len(ids))
    return {"ids": np.asarray(ids, np.uint32), "cl": np.asarray(cl, np.int32), "goff": np.asarray(goff, np.uint64)}


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_plain_definitions_equal_the_oracle(case, mode):
    exp = _oracle_groups(mode, case)
    got = case.reference(mode)
    assert pc.describe_difference(case.name, mode, got, exp) is None
    if mode == "fast" and case.single:
        ids, cl, ax, ay = pc.fast_reference(case.x, case.y, case.w)
        assert ids == got["ids"].tolist() and cl == got["cl"].tolist()
        assert ax == got["passes"][0]["anchors"] or len(case.x) < 2


@pytest.mark.parametrize("case", CASES + TIES, ids=repr)
def test_witness_holds_today(case):
    assert case.holds(pc.TODAY), (case.name, case.witness)


def test_cases_are_not_trivial():
    """every mode has output at stake in the multi-group cases, and the tie cases cluster"""
    for c in pc.multi_cases():
        for mode in pc.MODES:
            r = c.reference(mode)
            assert len(r["ids"]) > 100 and len(r["goff"]) == len(c.group_off), (c.name, mode)
        assert c.reference("fast")["cl"].max() > 1
    for c in TIES:
        ids, cl, _ = pyoracle.unit_points("fast", c.x, c.y, c.w)
        assert len(ids) > 500 and cl.max() > 100, c.name
    # the masking case: point 1 of some group really comes out twice
    m = next(c for c in CASES if c.name == "masking")
    ids = m.reference("mask")["ids"].tolist()
    assert any(a == b for a, b in zip(ids, ids[1:]))


def test_window_pass_rules():
    kept, ordinal, anchors = pc.window_pass([10, 11, 12, 5000, 5001, 9000, 9001], 100.0)
    assert kept == [True, True, True, True, True, False, False] and ordinal[:5] == [1, 1, 1, 2, 2] and anchors == [0, 3, 5, 6]
    assert pc.window_pass([10, 110, 111], 100.0)[2] == [0, 2]           # key == anchor + w is inside; the last element breaks the window
    assert pc.window_pass([10, 110, 111, 112], 100.5)[0] == [True, True, False, False]
    assert pc.window_pass([], 1.0) == ([], [], []) and pc.window_pass([7], 1.0) == ([False], [0], [0])
    assert pc.mask_reference([1, 2, 3], [1, 2, 3], 5) == [1, 1] and pc.mask_reference([1, 2], [1, 2], 5) == []
    assert pc.mask_reference([1, 2, 9, 10], [1, 2, 9, 10], 5) == [1, 2]   # point 1: far from point 2, near point 0: once
    assert pc._absdiff(0, 0xFFFFFFFF) == 1 and pc._absdiff(0x80000000, 0) == 1 << 31
    assert pc.first_difference([1, 2], [1, 2]) is None and pc.first_difference([1, 2], [1, 3]) == 1 and pc.first_difference([1], [1, 3]) == 1


def test_whole_path_table_has_long_chains_of_short_windows():
    from breakid_amd import abi
    contigs, cols = pc.whole_path_dataset()
    assert 15000 < len(cols["tid"]) < 25000
    o = pyoracle.Oracle(contigs, cols)
    w, rc = o.run(20, fast=True)
    rows, off = o.fetch(abi.STAGE_ISO)
    clustered, _ = o.fetch(abi.STAGE_CLUSTERED)
    o.close()
    assert rc == 0 and 1300 < w < 1350 and len(off) == 5
    assert len(pc.long_chains_of_short_windows(rows, off, w)) >= 3
    assert len(clustered) > 7500 and clustered["cluster"].max() > 400

"""Isolated-pair masking and the -fast clustering of csrc/cluster.hip on the designed point sets of tests/pointcases.py, through
bk_debug_points (one group) and bk_debug_points_groups (the product functions on ONE list of many groups, as the lanes call them),
against the plain Python definitions, entry for entry: ids, cluster numbers, group offsets, count.  The tie cases take their
expectation from the oracle.  Every case's witness is asserted at the constants of the build first, so the case really places what
it was made for: FW_TILE anchors in one tile, tiles the chain hops over, the lost last element alone in its tile, groups that
start on a tile's last position, groups the first pass empties.  A failure names the case, the mode, the first differing output
position, its group and its tile."""
import os

import numpy as np
import pytest

from breakid_amd import abi, capi
from oracle import pyoracle
from tests import pointcases as pc

pytestmark = pytest.mark.gpu

CONSTS = capi.cluster_info() if os.path.exists(capi.LIB_PATH) else pc.TODAY  # (no GPU needed; the cases follow the build)
SINGLE = pc.single_cases(CONSTS)
TIES = pc.single_cases(CONSTS, ties=True)
MULTI = pc.multi_cases(CONSTS)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context([("chr1", 1_000_000), ("chr2", 1_000_000)])
    yield c
    c.close()


def _expected(case, mode):
    if not case.ties:
        return case.reference(mode)
    assert case.single and mode == "fast"
    ids, cl, _ = pyoracle.unit_points("fast", case.x, case.y, case.w)
    return {"ids": ids, "cl": cl, "goff": np.asarray([0, len(ids)], np.uint64)}


def _groups(ctx, case, mode):
    ids, cl, goff = ctx.debug_points_groups(mode, case.x, case.y, case.group_off, case.w)
    assert len(ids) == len(cl) and int(goff[-1]) == len(ids), (case.name, mode, len(ids), goff[-3:])
    return {"ids": ids, "cl": cl if mode == "fast" else np.zeros(len(ids), np.int32), "goff": goff}


def _check(case, mode, got):
    exp = _expected(case, mode)
    diff = pc.describe_difference(case.name, mode, got, exp, CONSTS)
    if diff:
        pytest.fail(diff + "\n  witness: " + case.witness)
    assert len(got["ids"]) == len(exp["ids"])


def test_constants():
    assert CONSTS == capi.cluster_info() and set(CONSTS) == {"FW_TILE", "FW_LEVELS"}
    assert capi.lib().bk_debug_cluster_info(None) == abi.BK_ERR_ARG


@pytest.mark.parametrize("case", SINGLE + TIES, ids=repr)
def test_single_group_fast(ctx, case):
    assert case.holds(CONSTS), (case.name, case.witness)
    ids, cl = ctx.debug_points("fast", case.x, case.y, case.w)
    one = {"ids": ids, "cl": cl, "goff": np.asarray([0, len(ids)], np.uint64)}
    _check(case, "fast", one)
    many = _groups(ctx, case, "fast")
    _check(case, "fast", many)
    assert all(one[k].tobytes() == many[k].tobytes() for k in ("ids", "cl", "goff"))


@pytest.mark.parametrize("mode", ["mask", "iso"])
def test_single_group_masking_of_the_window_edges(ctx, mode):
    """(long) w against w = 3000.75 and keys of 2^31 - 1 in the masking too"""
    for case in [c for c in SINGLE if c.name.startswith(("window_edge", "degenerate"))]:
        ids, _ = ctx.debug_points(mode, case.x, case.y, case.w)
        _check(case, mode, {"ids": ids, "cl": np.zeros(len(ids), np.int32), "goff": np.asarray([0, len(ids)], np.uint64)})
        _check(case, mode, _groups(ctx, case, mode))


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("case", MULTI, ids=repr)
def test_many_groups(ctx, case, mode):
    assert case.holds(CONSTS), (case.name, case.witness)
    _check(case, mode, _groups(ctx, case, mode))


@pytest.mark.parametrize("mode", pc.MODES)
def test_buffers_reused_across_sizes(ctx, mode):
    """the same case twice on one context with a small one in between: ClusterBufs grown for the large case are reused by the
    small one and again by the large one, and nothing an earlier call left behind may show"""
    by = {c.name: c for c in SINGLE + MULTI}
    for big, small in (("emptied_groups", "degenerate_3"), ("one_hop_aligned", "small_groups_64"), ("masking", "length_%d" % (CONSTS["FW_TILE"] + 1))):
        first = _groups(ctx, by[big], mode)
        between = _groups(ctx, by[small], mode)
        again = _groups(ctx, by[big], mode)
        _check(by[small], mode, between)
        _check(by[big], mode, again)
        assert all(first[k].tobytes() == again[k].tobytes() for k in ("ids", "cl", "goff")), (big, small, mode)


def test_argument_errors(ctx):
    L, h = capi.lib(), ctx.h
    x = np.arange(4, dtype=np.uint32)
    out, cl, goff, n = np.zeros(9, np.uint32), np.zeros(9, np.int32), np.zeros(3, np.uint64), capi.C.c_uint32()

    def call(off, mode=2, xs=x):
        off = np.asarray(off, np.uint64)
        return L.bk_debug_points_groups(h, mode, xs.ctypes.data, x.ctypes.data, off.ctypes.data, len(off) - 1, 3000.0, out.ctypes.data, cl.ctypes.data, goff.ctypes.data,
                                        capi.C.byref(n))
    assert call([0, 2, 4]) == abi.BK_OK
    assert call([0, 3, 2]) == abi.BK_ERR_ARG and call([1, 2, 4]) == abi.BK_ERR_ARG and call([0, 2, 4], mode=3) == abi.BK_ERR_ARG
    assert L.bk_debug_points_groups(h, 2, None, None, np.asarray([0, 4], np.uint64).ctypes.data, 1, 3000.0, out.ctypes.data, cl.ctypes.data, goff.ctypes.data,
                                    capi.C.byref(n)) == abi.BK_ERR_ARG
    # no group at all, and groups without a point
    ids, c, g = ctx.debug_points_groups("fast", [], [], [0], 3000.0)
    assert len(ids) == 0 and g.tolist() == [0]
    for mode in pc.MODES:
        ids, c, g = ctx.debug_points_groups(mode, [], [], [0, 0, 0], 3000.0)
        assert len(ids) == 0 and g.tolist() == [0, 0, 0]


def test_whole_path_long_chains_of_short_windows():
    """lanes, list_of_groups and merge_lists_many see such groups too: four chromosome-pair groups, three of them longer than two
    tiles after masking, in x windows of at most 5 pairs, every stage against the oracle at the default environment"""
    from tests.test_gpu_parity import _compare_stages, _run_gpu
    contigs, cols = pc.whole_path_dataset()
    ctx, mean, sd, w = _run_gpu(contigs, cols, fast=True)
    o = pyoracle.Oracle(contigs, cols)
    assert (mean, sd) == o.isize_stats()
    ow, rc = o.run(20, fast=True)
    assert rc == 0 and ow == w
    rows, off = o.fetch(abi.STAGE_ISO)
    assert len(pc.long_chains_of_short_windows(rows, off, w, CONSTS)) >= 3
    _compare_stages(ctx, o)
    ctx.close()
    o.close()

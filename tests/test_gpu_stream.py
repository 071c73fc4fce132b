"""The stream pass (csrc/stream.hip: k_stream under launch_stream, run_stream's repeat, the pass in pieces behind the feed) on the designed
tables of tests/streamcases.py (tests/test_cpu_stream.py pins them on their edges).  bk_debug_stream_blocks caps the grid, so a
table of a few thousand records runs many iterations per block.  Candidates (sorted by record: their order is not defined), the
insert-size sums, max_span and the evidence tuples are compared exactly with the numpy definition and the oracle."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch

from breakid_amd import abi, capi
from breakid_amd.sharded import tensor_from_ptr
from oracle import pyoracle
from tests import streamcases as sc

pytestmark = pytest.mark.gpu
_G = None


def geo():
    global _G
    if _G is None:
        info = capi.stream_info()
        _G = sc.Geo({k: info[k] for k in sc.TODAY})
        _G.resident = info["RESIDENT"]
    return _G


@pytest.fixture
def block_cap():
    try:
        yield capi.stream_blocks
    finally:
        capi.stream_blocks(0)


def shard_buffer(ctx, which, dtype):
    ptr, n, eb = C.c_void_p(), C.c_uint64(), C.c_uint32()
    ctx._check(ctx.L.bk_shard_buffer(ctx.h, which, C.byref(ptr), C.byref(n), C.byref(eb)))
    assert eb.value == dtype.itemsize
    ctx.sync()
    raw = tensor_from_ptr(ptr.value, n.value * eb.value, torch.device("cuda", 0)).cpu().numpy()
    return raw.view(dtype).copy() if n.value else np.zeros(0, dtype)


def oracle_tuples(contigs, cols):
    o = pyoracle.Oracle(contigs, cols)
    try:
        o.split_evidence()
        return o.fetch(abi.STAGE_SPLITS)[0]
    finally:
        o.close()


def check_ctx(ctx, contigs, cols, q=sc.QUAL, rec_base=0, tuples=True):
    """the state a finished stream pass left in `ctx` against the definition; returns the candidates as they lie in the buffer"""
    e = sc.expected(cols, q, rec_base)
    st = ctx.shard_get_stats()
    got = {"isize_sum": st.isize_sum, "isize_n": st.isize_n, "sumsq": st.sumsq, "vmax": st.vmax, "max_span": st.max_span, "n_cand": st.n_cand}
    exp = {"isize_sum": e.isize_sum, "isize_n": e.isize_n, "sumsq": e.sumsq, "vmax": e.vmax, "max_span": e.max_span, "n_cand": len(e.cand)}
    print(got, exp)
    assert got == exp
    raw = shard_buffer(ctx, abi.BUF_CANDIDATES, abi.CAND)
    cand = np.sort(raw, order="rec")
    assert len(cand) == len(e.cand) and np.array_equal(cand["rec"], e.cand["rec"])
    for f in abi.CAND.names:
        assert np.array_equal(cand[f], e.cand[f]), f
    if tuples:
        exp_t = oracle_tuples(contigs, cols)
        exp_t["rec"] += np.uint64(rec_base)
        got_t = shard_buffer(ctx, abi.BUF_TUPLES, abi.SPLIT)
        assert st.n_split == len(exp_t) == len(got_t)
        assert set(int(r) - rec_base for r in got_t["rec"]) <= set(int(i) for i in e.sa)
        assert np.array_equal(np.sort(got_t, order="rec"), np.sort(exp_t, order="rec"))
        if rec_base == 0:
            assert ctx.split_evidence() == len(exp_t)  # and through the project's own split sort
            assert np.array_equal(ctx.fetch(abi.STAGE_SPLITS)[0], exp_t)
    return raw, e


def run_case(plan, cap, set_cap, q=sc.QUAL):
    contigs, cols = sc.build(plan)
    ctx = capi.Context(contigs)
    try:
        ctx.upload(cols)
        set_cap(cap)
        ctx.shard_begin(0, q)
        set_cap(0)
        return check_ctx(ctx, contigs, cols, q)
    finally:
        ctx.close()


def test_info_and_cap(block_cap):
    info = capi.stream_info()
    assert info["RESIDENT"] >= 256 and info["STREAM_V"] in (4, 8)  # at least a block per CU
    assert capi.lib().bk_debug_stream_info(None) == abi.BK_ERR_ARG


# ---- the two bins --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", range(6))
def test_candidate_window_edges(edge, block_cap):
    """one block: ST_CAND_CAP / 2 - 1, ST_CAND_CAP / 2, ST_CAND_CAP - 1, ST_CAND_CAP, ST_CAND_CAP + 1 and 4 B candidates before the first look
    at the bin, 3 in the window behind it: the half-full threshold, the bin's last slot, the first direct append, the bin reused"""
    g = geo()
    run_case(sc.window_case(g, "cand", sc.cand_edges(g)[edge]), 1, block_cap)


@pytest.mark.parametrize("edge", range(6))
def test_sa_window_edges(edge, block_cap):
    g = geo()
    raw, e = run_case(sc.window_case(g, "sa", sc.sa_edges(g)[edge]), 1, block_cap)
    assert len(e.sa) == sc.sa_edges(g)[edge] + 3


@pytest.mark.parametrize("edge", [1, 4, 5])
def test_both_kinds_on_the_same_records(edge, block_cap):
    g = geo()
    run_case(sc.window_case(g, "both", sc.cand_edges(g)[edge]), 1, block_cap)


@pytest.mark.parametrize("which", range(3))
def test_both_bins_at_one_look(which, block_cap):
    """the same look finds only the candidate bin half full, only the SA bin, both"""
    run_case(sc.both_bins_cases(geo())[which][1], 1, block_cap)


@pytest.mark.parametrize("first", ["half", "below"])
def test_half_full_bin_leaves_at_the_first_look(first, block_cap):
    """WHEN a bin is flushed shows in where its rows lie.  One block; ST_CAND_CAP / 2 candidates in the first window: the look after
    the fourth iteration flushes them, so the first rows of the buffer are exactly the first window's.  One fewer: they stay, the
    second window (every record a candidate) overflows the bin in its first iteration, and those direct appends lie in front."""
    g = geo()
    n1 = g.CC // 2 - (first == "below")
    raw, e = run_case(sc.order_of_flushes_case(g, n1), 1, block_cap)
    head = set(int(r) for r in raw["rec"][:n1])
    window1 = set(int(r) for r in e.cand["rec"] if r < g.W)
    assert len(window1) == n1
    if first == "half":
        assert head == window1
    else:
        assert int(raw["rec"][0]) >= g.W and not head <= window1


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", sc.GEOMETRY_CAPS)
@pytest.mark.parametrize("k", sc.GEOMETRY_K)
def test_geometry(cap, k, block_cap):
    """n = k B cap + r: idle blocks and idle lanes in the last round, tails of 0 .. STREAM_V - 1 records, 1, 4 and 5 iterations (+ 1)"""
    g = geo()
    for rest in sc.geometry_rests(g):
        print("rest", rest)
        p = sc.geometry_case(g, cap, k, rest)
        if not cap:
            assert g.blocks(p.n, 0, g.resident) == (p.n // g.V + 256) // 256  # the card takes the whole table in one round
        run_case(p, cap, block_cap)


@pytest.mark.parametrize("cap", [0, 1])
def test_tail_only_tables(cap, block_cap):
    g = geo()
    for n in sc.tail_only_sizes(g):
        run_case(sc.random_plan(n, n, cand=0.6, sa=0.5, proper=0.4), cap, block_cap)
    p = sc.Plan(g.V - 1)
    p.is_candidate[:] = p.has_sa[:] = True
    run_case(p, cap, block_cap)


# ---- neighbours and order --------------------------------------------------------------------------------------------------------------------
PLACES = sorted(sc.places(sc.Geo(), sc.places_n(sc.Geo())))


@pytest.mark.parametrize("place", PLACES)
def test_neighbour_loads(place, block_cap):
    """the one record with four CIGAR words, SA text and the longest span sits where its offsets' end comes from another lane, from
    global memory at the edge of a wave or of the table, or in the tail path"""
    p, at = sc.neighbour_case(geo(), place)
    raw, e = run_case(p, 1, block_cap)
    assert e.max_span == sc.LONG_SPAN


@pytest.mark.parametrize("by", ["pos", "tid"])
@pytest.mark.parametrize("place", PLACES)
def test_one_inversion_is_rejected(place, by, block_cap):
    p, at = sc.unsorted_case(geo(), place, by)
    contigs, cols = sc.build(p)
    ctx = capi.Context(contigs)
    try:
        ctx.upload(cols)
        block_cap(1)
        with pytest.raises(capi.BreakIDError) as err:
            ctx.shard_begin(0, sc.QUAL)
        assert err.value.code == abi.BK_ERR_UNSORTED
    finally:
        ctx.close()


def test_equal_neighbours_are_sorted(block_cap):
    run_case(sc.equal_neighbours_case(geo()), 1, block_cap)


# ---- capacity repeat -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_capacity_repeat(which, block_cap):
    """more candidates / SA-bearing records than the first attempt of run_stream has room for on a fresh context: the pass is repeated,
    counts and contents are exact, and so is a small table uploaded into the same context afterwards"""
    g = geo()
    plan = sc.capacity_cases()[which]
    contigs, cols = sc.build(plan)
    ctx = capi.Context(contigs)
    try:
        ctx.upload(cols)
        ctx.shard_begin(0, sc.QUAL)
        raw, e = check_ctx(ctx, contigs, cols)
        cc, sa = sc.first_capacity(plan.n)
        assert len(e.cand) > cc if which == 0 else len(e.sa) > sa
        small = sc.random_plan(3 * g.B + 2, 5)
        contigs2, cols2 = sc.build(small)
        ctx.upload(cols2)
        block_cap(2)
        ctx.shard_begin(0, sc.QUAL)
        check_ctx(ctx, contigs2, cols2)
    finally:
        ctx.close()


# ---- the pass in pieces ------------------------------------------------------------------------------------------------------------------------
def test_pieces_behind_the_feed(monkeypatch, capfd, block_cap):
    """bk_bam_decode_device_ctx with small feed chunks and one block: k_stream is launched with q_begin > 0 several times; candidates
    and stats equal those of the host decoder's table uploaded whole"""
    from breakid_amd import synth
    contigs = [("chr1", 6_000_000), ("chr2", 5_000_000)]
    ds = synth.make_cfg(17, contigs, 60_000, 60, 40, 600, jitter=250, read_len=100)
    monkeypatch.setenv("BREAKID_FEED_CHUNK_MB", "0.25")
    monkeypatch.setenv("BK_DEBUG", "feed")
    with tempfile.TemporaryDirectory() as t:
        path = os.path.join(t, "a.bam")
        ds.write_bam(path, aligned=True)
        block_cap(1)
        ctx, table = capi.decode_bam_device_ctx(path, qual=sc.QUAL)
        block_cap(0)
        contigs2, cols = capi.decode_bam(path)
    try:
        err = capfd.readouterr().err
        assert "[feed/stream] stream pass overlapped" in err, err[-600:]
        done, total = [int(v) for v in err.split("[feed/stream] stream pass overlapped:")[1].split("records")[0].replace("of", " ").split()]
        print("pieces", done, total)
        assert total == len(cols["tid"]) and 0 < done <= total and contigs2 == contigs
        raw, e = check_ctx(ctx, contigs, cols, tuples=False)
        assert len(e.cand) > 100
        ref = capi.Context(contigs)
        try:
            ref.upload(cols)
            ref.shard_begin(0, sc.QUAL)
            a, b = ctx.shard_get_stats(), ref.shard_get_stats()
            assert all(getattr(a, f) == getattr(b, f) for f, _ in abi.ShardStats._fields_)
            assert np.array_equal(np.sort(raw, order="rec"), np.sort(shard_buffer(ref, abi.BUF_CANDIDATES, abi.CAND), order="rec"))
            ta, tb = shard_buffer(ctx, abi.BUF_TUPLES, abi.SPLIT), shard_buffer(ref, abi.BUF_TUPLES, abi.SPLIT)
            assert np.array_equal(np.sort(ta, order="rec"), np.sort(tb, order="rec"))
        finally:
            ref.close()
    finally:
        ctx.close()
        table.close()


# ---- flags -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1])
def test_flag_gates(cap, block_cap):
    """every combination of PAIRED, PROPER, UNMAP, SECONDARY, QCFAIL and DUP with mapq q - 1 and q: the three memberships are the
    reference's three predicates"""
    raw, e = run_case(sc.flag_gate_case(), cap, block_cap)
    assert (len(e.cand), len(e.sa), e.isize_n) == (4, 32, 2)

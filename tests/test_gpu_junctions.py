"""Split junctions (`bk_split_junctions`, `-junctions`): the kernels against the two statements of tests/junctioncases.py byte for
byte.  No tuples; eligible-tuple counts around one and two scan blocks and radix tiles; one read with two alignments in each form;
every kind of dropped tuple alone; chains, staircases and sides under three tolerances; a hot window with the representative's tie;
min_reads; the claimed row straight, crossed, both ways, 3 bp off and before the breakpoint stage; the designed 6-tuple without
bk_fetch; every table form, every refusal, two runs; and the command line's files against the statements."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import junctioncases as jc

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = cc.CONTIGS
NAMES = cc.NAMES
TLEN = [l for _, l in CONTIGS]
# callcases.LOCI and one locus whose first side lies on the higher contig
LOCI = cc.LOCI + [("LR_back", 3, 100_000, "L", 0, 1_500_000, "R")]


def assert_rows(got, exp):
    assert got.dtype == abi.SPLIT_JUNCTION and len(got) == len(exp), (len(got), len(exp))
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def one_tuple(recs):
    """the reads' partners lose their SA tag: one tuple per read, the own record's"""
    for r in recs:
        if r.flag & 0x900:
            r.sa = ""
    return recs


def reads_at(tag, n, ta, bpa, da, tb, bpb, db, **kw):
    return [r for k in range(n) for r in cc.designed_split("%s_%d" % (tag, k), ta, bpa, da, tb, bpb, db, **kw)]


class Case:
    """a context after bk_split_evidence, its tuples and its record columns"""

    def __init__(self, recs, where="host", contigs=CONTIGS):
        self.ds = jc.dataset(contigs, recs)
        self.cols = self.ds.to_soa()
        self.tlen = [l for _, l in contigs]
        self.ctx, self.hold = cc.make_ctx(contigs, self.cols, where)
        self.ctx.split_evidence()
        self.splits = self.ctx.fetch(abi.STAGE_SPLITS)[0]

    def check(self, mapq_min=QUAL, tol=2, min_reads=1, clusters=None):
        """the call against both statements; returns (rows, info of the brute-force statement)"""
        info = {}
        args = (self.splits, self.cols["flag"], self.cols["mapq"], self.tlen, mapq_min, tol, min_reads, clusters)
        exp = jc.expected(*args, info=info)
        assert exp.tobytes() == jc.expected_sweep(*args).tobytes()
        got = self.ctx.split_junctions(mapq_min, tol, min_reads)
        assert_rows(got, exp)
        cnt = self.ctx.split_junction_counts()
        assert (cnt["tuples"], cnt["eligible"], cnt["exact"], cnt["calls"]) == (len(self.splits), info["eligible"], info["exact"], info["calls"])
        assert cnt["claimed"] == int((exp["call"] >= 0).sum())
        info["rounds"] = cnt["rounds"]
        return got, info

    def reasons(self, mapq_min=QUAL):
        return [jc.why_dropped(s, self.cols["flag"], self.cols["mapq"], self.tlen, mapq_min) for s in self.splits]

    def close(self):
        self.ctx.close()


def background(n=40, seed=3):
    rng = np.random.default_rng(seed)
    return [r for i in range(n) for r in synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)]


# ---- 1. no tuples ----------------------------------------------------------------------------------------------------------------------
def test_no_tuples():
    c = Case(background(200))
    assert len(c.splits) == 0
    got, info = c.check()
    assert len(got) == 0 and info["eligible"] == 0 and info["rounds"] == 0
    c.close()


# ---- 2. sizes across the boundaries of the scan and the radix sort ------------------------------------------------------------------------
def sized_recs(e, n_junctions):
    """e eligible tuples: designed reads of two tuples each over n_junctions loci 50 bases apart, and one read of one tuple when e is odd"""
    recs = background(20)
    for k in range(e // 2):
        j = k % n_junctions
        recs += cc.designed_split("z%d" % k, 0, 10_000 + 50 * j, "L", 1, 20_000 + 50 * j, "R")
    if e & 1:
        recs += one_tuple(cc.designed_split("odd", 2, 5_000, "R", 3, 7_000, "L"))
    return recs


def size_cases():
    p = capi.prims_info()
    assert p["SCAN_TILE"] == p["RS_TILE"]  # (one list serves both; were they to differ, both lists would be needed)
    t = p["RS_TILE"]
    return [t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 301, p["SCAN_ONE_MAX"] + 2]


@pytest.mark.parametrize("which", range(8))
def test_sizes_across_boundaries(which):
    e = size_cases()[which]
    c = Case(sized_recs(e, 700 if e < 10_000 else 500))
    got, info = c.check(tol=2)
    assert info["eligible"] == e and len(c.splits) == e, (info["eligible"], len(c.splits), e)
    assert int(got["n_tuples"].sum()) == e and info["exact"] == len(got) >= 500
    c.close()


# ---- 3. one read, two alignments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0x800, 0x100, 0x100 | 0x800])
def test_one_read_two_alignments(form):
    c = Case(background() + synth._split_pair("two", NAMES, 0, 300_000, 1, 700_000, partner_flag=form))
    got, info = c.check()
    assert len(got) == 1 and len(c.splits) == 2
    r = got[0]
    assert (int(r["n_reads"]), int(r["n_tuples"]), int(r["n_exact"]), list(r["n_own"]), list(r["mapq_sum"])) == (1, 2, 1, [1, 1], [60, 60])
    assert (int(r["tid1"]), int(r["pos1"]), int(r["right1"]), int(r["tid2"]), int(r["pos2"]), int(r["right2"])) == (0, 300_000, 0, 1, 700_000, 1)
    c.close()


def test_canonical_order_swaps_the_ends():
    """the own end of the SA-bearing primary on the higher contig; on one contig at the higher position; at one position with the other side"""
    designs = [(3, 400_000, "L", 1, 900_000, "R"), (2, 800_000, "R", 2, 300_000, "L"), (0, 600_000, "R", 0, 600_000, "L")]
    recs = background()
    for k, d in enumerate(designs):
        recs += one_tuple(cc.designed_split("sw%d" % k, *d))
    c = Case(recs)
    got, info = c.check()
    assert len(got) == 3 and all(list(r["n_own"]) == [0, 1] for r in got)
    want = sorted((jc.canonical_design(*d) for d in designs), key=jc.order_key)
    assert [(int(r["tid1"]), int(r["pos1"]), int(r["right1"]), int(r["tid2"]), int(r["pos2"]), int(r["right2"])) for r in got] == want
    assert want[0] == (0, 600_000, 0, 0, 600_000, 1)
    c.close()


# ---- 4. dropped tuples, each alone ---------------------------------------------------------------------------------------------------------
def dropped_read(kind):
    if kind == "poison":
        return [synth.Rec("bad", 0x1 | 0x2 | 0x40 | 0x20, 2, 99_960, 60, "5M95S", 2, 100_100, 250, sa="chr2,200001,+,50M50M,60,0;"),
                synth.Rec("bad", 0x1 | 0x2 | 0x80 | 0x10, 2, 100_100, 60, "100M", 2, 99_960, -250)]
    r = one_tuple(cc.designed_split("drop", 2, 500_000, "L", 3, 800_000, "R"))
    if kind == "other_contig":
        r[0].sa = r[0].sa.replace("chr4,", "chrUn_x,")
    elif kind == "position_zero":
        r[0].sa = "chr4,0,+,60S40M,60,0;"
    elif kind == "position_beyond":
        r[0].sa = "chr4,2000001,+,60S40M,60,0;"
    elif kind == "mapq":
        r[0].mapq = QUAL - 1
    elif kind == "qcfail":
        r[0].flag |= 0x200
    elif kind == "identical":
        r = one_tuple(cc.designed_split("drop", 2, 500_000, "L", 2, 500_000, "L"))
    return r


@pytest.mark.parametrize("kind", ["poison", "other_contig", "position_zero", "position_beyond", "mapq", "qcfail", "identical"])
def test_dropped_tuples_each_alone(kind):
    c = Case(background() + reads_at("good", 3, 0, 300_000, "L", 1, 700_000, "R") + dropped_read(kind))
    reasons = [r for r in c.reasons() if r is not None]
    assert reasons == [kind.split("_")[0] if kind.startswith("position") else kind], reasons
    got, info = c.check()
    assert len(got) == 1 and int(got[0]["n_reads"]) == 3 and info["eligible"] == len(c.splits) - 1 == 6
    if kind == "mapq":
        got, info = c.check(mapq_min=QUAL - 1)
        assert len(got) == 2 and info["eligible"] == 7
    c.close()


# ---- 5. linkage ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linkage():
    """a chain of 70 exact junctions 25 apart in pos1 (pos2 fixed); a staircase 2 apart in pos1 and 30 apart in pos2; one position pair
    with all four combinations of sides; pairs exactly tol and tol + 1 apart for tol 2 and 25"""
    recs = background()
    for k in range(70):
        recs += one_tuple(cc.designed_split("chain%d" % k, 0, 100_000 + 25 * k, "L", 1, 500_000, "R"))
    for k in range(12):
        recs += one_tuple(cc.designed_split("stair%d" % k, 0, 300_000 + 2 * k, "L", 1, 900_000 + 30 * k, "R"))
    for k, (da, db) in enumerate((("L", "L"), ("L", "R"), ("R", "L"), ("R", "R"))):
        recs += one_tuple(cc.designed_split("side%d" % k, 2, 400_000, da, 3, 600_000, db))
    for k, d in enumerate((2, 3, 25, 26)):
        recs += one_tuple(cc.designed_split("gapA%d" % k, 1, 1_000_000 + 1000 * k, "L", 2, 1_000_000, "R"))
        recs += one_tuple(cc.designed_split("gapB%d" % k, 1, 1_000_000 + 1000 * k + d, "L", 2, 1_000_000 - d, "R"))
    c = Case(recs)
    yield c
    c.close()


@pytest.mark.parametrize("tol", [0, 2, 25])
def test_linkage(linkage, tol):
    got, info = linkage.check(tol=tol)
    assert info["exact"] == 70 + 12 + 4 + 8
    chain = got[(got["tid1"] == 0) & (got["tid2"] == 1) & (got["pos2"] == 500_000)]
    stair = got[(got["tid1"] == 0) & (got["tid2"] == 1) & (got["pos2"] >= 900_000)]
    sides = got[(got["tid1"] == 2) & (got["tid2"] == 3)]
    gaps = got[(got["tid1"] == 1) & (got["tid2"] == 2)]
    assert len(sides) == 4 and np.all(sides["n_exact"] == 1) and len(stair) == 12
    assert len(gaps) == {0: 8, 2: 7, 25: 5}[tol]
    if tol == 25:
        assert len(chain) == 1 and int(chain[0]["n_exact"]) == 70 and (int(chain[0]["lo1"]), int(chain[0]["hi1"])) == (100_000, 100_000 + 25 * 69)
        assert int(chain[0]["pos1"]) == 100_000 and info["rounds"] > 1  # every exact junction has one read: the smallest is the representative
    else:
        assert len(chain) == 70 and info["rounds"] == (1 if tol == 0 else 2)  # (tol 2 joins one of the gap pairs)


def test_a_label_that_travels_against_the_table_order():
    """A U of 304 exact junctions at tol 25: the lower arm runs along pos1 at one pos2, a column of four joins it at its far end to
    the upper arm 75 bases up in pos2, which runs back.  The two arms alternate in the sorted table, so the upper arm first settles on
    its own smallest member (index 1) and the call's smallest label enters it from its far end, against the order of the table.  One
    round cannot carry it across 150 members (each step needs a wavefront that started earlier to read what one that started later
    wrote), the round in which index 1 falls to 0 changes something, and one more finds nothing to change: at least three rounds."""
    recs, arm = background(), 150
    for k in range(arm):
        recs += one_tuple(cc.designed_split("lo%d" % k, 0, 100_000 + 25 * k, "L", 1, 500_000, "R"))
        recs += one_tuple(cc.designed_split("up%d" % k, 0, 100_000 + 25 * k, "L", 1, 500_075, "R"))
    for k in range(4):
        recs += one_tuple(cc.designed_split("col%d" % k, 0, 100_000 + 25 * arm, "L", 1, 500_000 + 25 * k, "R"))
    c = Case(recs)
    got, info = c.check(tol=25)
    assert len(got) == 1 and int(got[0]["n_exact"]) == 2 * arm + 4 == info["exact"] and int(got[0]["n_reads"]) == 2 * arm + 4
    assert (int(got[0]["pos1"]), int(got[0]["pos2"]), int(got[0]["hi2"])) == (100_000, 500_000, 500_075)
    assert 3 <= info["rounds"] <= 40, info["rounds"]  # (far fewer than the arm's 150: the root is hooked, the rest jumps)
    got, info = c.check(tol=24)
    assert len(got) == 2 * arm + 4 and info["rounds"] == 1
    c.close()


# ---- 6. a hot window -----------------------------------------------------------------------------------------------------------------------
def test_hot_window_and_the_tie_rule():
    """150 exact junctions with pos1 inside one window of 2 * tol + 1 positions (pos2 spreads them): more than two steps of 64.  Those
    within tol in pos2 too form calls; two exact junctions of the largest call have 3 reads each, the most: the smaller one wins."""
    recs = background()
    for k in range(150):
        n = 3 if k in (7, 9) else 1
        recs += one_tuple(reads_at("hot%d" % k, n, 0, 700_000 + k % 5, "L", 1, 800_000 + 4 * (k // 5) + (200 if k >= 100 else 0), "R"))
    c = Case(recs)
    got, info = c.check(tol=4)
    assert info["exact"] == 150 and len(got) == 2
    big = got[0]
    assert int(big["n_exact"]) == 100 and int(big["top_reads"]) == 3 and int(big["n_reads"]) == 104
    assert (int(big["pos1"]), int(big["pos2"])) == (700_000 + 7 % 5, 800_000 + 4 * (7 // 5))
    keys = info["keys"]
    assert keys.index((0, 700_002, 0, 1, 800_004, 1)) < keys.index((0, 700_004, 0, 1, 800_004, 1))
    c.close()


# ---- 7. min_reads --------------------------------------------------------------------------------------------------------------------------
def test_min_reads_order_and_indices():
    recs = background()
    sizes = [1, 4, 2, 3, 1, 5, 3]
    for k, n in enumerate(sizes):
        recs += reads_at("mr%d" % k, n, 0, 200_000 + 1000 * k, "L", 2, 300_000, "R")
    c = Case(recs)
    all_rows, _ = c.check(min_reads=1)
    assert list(all_rows["n_reads"]) == sizes
    got, _ = c.check(min_reads=3)
    assert list(got["n_reads"]) == [4, 3, 5, 3] and [int(p) for p in got["pos1"]] == [201_000, 203_000, 205_000, 206_000]
    assert all(got[i].tobytes() == all_rows[j].tobytes() for i, j in enumerate((1, 3, 5, 6)))
    got, _ = c.check(min_reads=6)
    assert len(got) == 0
    c.close()


# ---- 8. claimed ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def designed():
    """callcases.designed_tumor (eight voted loci), a junction 3 bp off the first locus, and a deletion and
    a duplication that no pair cluster stands behind"""
    ds = cc.designed_tumor(mix=False, n_proper=4000, loci=LOCI)
    name, ta, bpa, da, tb, bpb, db = cc.LOCI[0]
    ds.recs += reads_at("off3", 2, ta, bpa + 3, da, tb, bpb, db)
    ds.recs += reads_at("del", 5, 1, 1_700_000, "L", 1, 1_700_250, "R") + reads_at("dup", 3, 2, 200_400, "L", 2, 200_000, "R")
    ds.sort()
    cols = ds.to_soa()
    ctx = capi.Context(CONTIGS)
    ctx.upload(cols)
    ctx.split_evidence()
    splits = ctx.fetch(abi.STAGE_SPLITS)[0]
    args = (splits, cols["flag"], cols["mapq"], TLEN, QUAL)
    before = ctx.split_junctions(QUAL, 0, 1)
    ctx.run(qual=QUAL, fast=True)
    cl = ctx.fetch(abi.STAGE_CLUSTERS)[0]
    yield dict(ctx=ctx, cl=cl, args=args, before=before, ds=ds, cols=cols)
    ctx.close()


def test_claimed(designed):
    ctx, cl, args = designed["ctx"], designed["cl"], designed["args"]
    assert np.all(designed["before"]["call"] == -1) and np.all(designed["before"]["call_crossed"] == 0)
    assert_rows(designed["before"], jc.expected(*args, 0, 1, None))
    for tol in (0, 2):
        exp = jc.expected(*args, tol, 1, cl)
        assert exp.tobytes() == jc.expected_sweep(*args, tol, 1, cl).tobytes()
        got = ctx.split_junctions(QUAL, tol, 1)
        assert_rows(got, exp)
        seen = dict(straight=0, crossed=0)
        for name, ta, bpa, da, tb, bpb, db in LOCI:
            rows = cc.rows_of(cl, ta, bpa, tb, bpb)
            assert len(rows) == 1, name
            k = jc.canonical_design(ta, bpa, da, tb, bpb, db)
            mine = [r for r in got if (int(r["tid1"]), int(r["pos1"]), int(r["right1"]), int(r["tid2"]), int(r["pos2"]), int(r["right2"])) == k]
            assert len(mine) == 1 and int(mine[0]["call"]) == rows[0][0], name
            a_first = (ta, bpa) <= (tb, bpb)
            assert int(mine[0]["call_crossed"]) == int(rows[0][1] != a_first)
            seen["crossed" if int(mine[0]["call_crossed"]) else "straight"] += 1
        # A context's own rows put the lower (contig, position) first, as the canonical form does: every locus is claimed straight, the
        # locus designed the other way round included.  The crossed match: test_claimed_straight_crossed_and_both_ways.
        assert seen == dict(straight=len(LOCI), crossed=0), seen
        # 3 bp off the first locus: a call of its own (3 > tol) that no row claims (3 > 2); the deletion and the duplication have no row
        free = got[got["call"] < 0]
        assert [(int(r["tid1"]), int(r["pos1"])) for r in free] == [(0, 300_003), (1, 1_700_000), (2, 200_000)] and len(got) == len(LOCI) + 3


def test_claimed_straight_crossed_and_both_ways():
    """bk_debug_split_junctions looks the claimed row up in a table of the caller's, whose rows may state their two sides in either
    order: claimed straight; claimed crossed only; a row that matches both ways (straight wins); the smallest row wins; an unvoted row
    and a row 3 bp off claim nothing"""
    recs = background()
    recs += reads_at("j1", 3, 0, 300_000, "L", 1, 700_000, "R") + reads_at("j2", 2, 2, 400_000, "L", 3, 600_000, "R")
    recs += reads_at("j3", 2, 1, 100_000, "L", 1, 100_500, "R") + reads_at("j4", 2, 0, 900_000, "R", 2, 50_000, "L")
    recs += reads_at("j5", 2, 2, 900_000, "L", 2, 900_002, "R")
    c = Case(recs)
    rows = [(0, 300_000, 1, 700_000, 1),   # 0: matches j1 straight, but is not voted
            (3, 600_002, 2, 399_998, 3),   # 1: j2 crossed only, 2 bp off on both ends
            (0, 300_001, 1, 699_999, 3),   # 2: j1 straight
            (1, 700_000, 0, 300_000, 3),   # 3: j1 crossed, a larger row: row 2 keeps it
            (1, 100_500, 1, 100_000, 3),   # 4: j3 crossed only, on one contig
            (2, 900_001, 2, 900_001, 3),   # 5: j5 both ways
            (0, 900_003, 2, 50_000, 3),    # 6: 3 bp off j4
            (2, 50_000, 0, 900_000, 1)]    # 7: j4 crossed, not voted
    cl = np.zeros(len(rows), abi.CLUSTER)
    for r, (t1, e1, t2, e2, flags) in zip(cl, rows):
        r["p1_tid"], r["p1_exact"], r["p2_tid"], r["p2_exact"], r["flags"] = t1, e1, t2, e2, flags
    for tol in (0, 2):
        args = (c.splits, c.cols["flag"], c.cols["mapq"], TLEN, QUAL, tol, 1, cl)
        exp = jc.expected(*args)
        assert exp.tobytes() == jc.expected_sweep(*args).tobytes()
        got = c.ctx.debug_split_junctions(QUAL, tol, 1, cl)
        assert_rows(got, exp)
        by_end = {(int(r["tid1"]), int(r["pos1"])): (int(r["call"]), int(r["call_crossed"])) for r in got}
        assert by_end == {(0, 300_000): (2, 0), (2, 400_000): (1, 1), (1, 100_000): (4, 1), (0, 900_000): (-1, 0), (2, 900_000): (5, 0)}, by_end
        assert c.ctx.split_junction_counts()["claimed"] == 4
    # without rows, and through the call itself before the breakpoint stage: nothing is claimed
    assert np.all(c.ctx.debug_split_junctions(QUAL, 2, 1, cl[:0])["call"] == -1) and np.all(c.ctx.split_junctions(QUAL, 2, 1)["call"] == -1)
    # the refusals of the call, and its own
    import ctypes as C
    L, out, n = capi.lib(), C.c_void_p(), C.c_uint64()
    assert L.bk_debug_split_junctions(c.ctx.h, QUAL, 2, 1, None, 3, C.byref(out), C.byref(n)) == abi.BK_ERR_ARG and b"null rows" in L.bk_last_error(c.ctx.h)
    assert L.bk_debug_split_junctions(c.ctx.h, QUAL, 101, 1, cl.ctypes.data, len(cl), C.byref(out), C.byref(n)) == abi.BK_ERR_ARG
    c.close()


# ---- 9. independent of bk_fetch ------------------------------------------------------------------------------------------------------------
def test_designed_reads_give_their_six_tuple():
    designs = [(t[1], t[2], t[3], t[4], t[5], t[6]) for t in cc.LOCI]
    recs = background()
    for k, d in enumerate(designs):
        recs += reads_at("d%d" % k, k + 1, *d)
    cols = jc.dataset(CONTIGS, recs).to_soa()
    ctx = capi.Context(CONTIGS)
    ctx.upload(cols)
    ctx.split_evidence()
    got = ctx.split_junctions(QUAL, 0, 1)
    want = sorted(((jc.canonical_design(*d), k + 1) for k, d in enumerate(designs)), key=lambda t: jc.order_key(t[0]))
    assert [((int(r["tid1"]), int(r["pos1"]), int(r["right1"]), int(r["tid2"]), int(r["pos2"]), int(r["right2"])), int(r["n_reads"])) for r in got] == want
    assert all(int(r["n_tuples"]) == 2 * int(r["n_reads"]) and int(r["n_own"][0]) == int(r["n_own"][1]) and int(r["n_exact"]) == 1 for r in got)
    assert all((int(r["lo1"]), int(r["hi1"]), int(r["lo2"]), int(r["hi2"])) == (int(r["pos1"]), int(r["pos1"]), int(r["pos2"]), int(r["pos2"])) for r in got)
    ctx.close()


# ---- 10. table forms, errors, two runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "device_side", "exclude_host", "exclude_device", "decode_ctx"])
def test_table_forms(form, designed):
    import torch
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(300_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
        cols = {k: dcols[k].cpu().numpy().view(dt)[:dcols["n"]] for k, dt in (("flag", np.uint16), ("mapq", np.uint8))}
        tlen = [l for _, l in contigs]
    elif form == "decode_ctx":
        cols, tlen = designed["cols"], TLEN
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            designed["ds"].write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        cols, tlen = designed["cols"], TLEN
        t, hold = cc.make_ctx(CONTIGS, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            tid, beg, end = np.asarray([1, 0], np.int32), np.asarray([1_699_000, 0], np.int32), np.asarray([1_701_000, 5_000], np.int32)
            assert t.exclude_regions(tid, beg, end) > 10
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, tid, beg, end))
    t.split_evidence()
    splits = t.fetch(abi.STAGE_SPLITS)[0]
    assert len(splits) > 10
    for tol, min_reads in ((2, 1), (0, 3)):
        args = (splits, cols["flag"], cols["mapq"], tlen, QUAL, tol, min_reads)
        exp = jc.expected(*args)
        assert exp.tobytes() == jc.expected_sweep(*args).tobytes()
        got = t.split_junctions(QUAL, tol, min_reads)
        assert_rows(got, exp)
        assert t.split_junctions(QUAL, tol, min_reads).tobytes() == got.tobytes()  # two runs, the same bytes
    assert len(got) > 0
    if form.startswith("exclude"):
        assert not np.any((got["tid1"] == 1) & (got["pos1"] == 1_700_000))  # the deletion lies in the excluded interval
    after = t.fetch(abi.STAGE_SPLITS)[0]
    assert after.tobytes() == splits.tobytes()  # it changes nothing a later bk_fetch returns
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


def test_errors_and_timing(designed):
    import ctypes as C
    t = capi.Context(CONTIGS)
    t.upload(designed["cols"])
    with pytest.raises(capi.BreakIDError) as e:
        t.split_junctions(QUAL, 2, 1)
    assert e.value.code == abi.BK_ERR_ARG and "bk_split_evidence first" in str(e.value)
    t.split_evidence()
    for args, word in (((-1, 2, 1), "mapq_min below 0"), ((QUAL, 101, 1), "tol above 100"), ((QUAL, 2, 0), "min_reads must be at least 1")):
        with pytest.raises(capi.BreakIDError) as e:
            t.split_junctions(*args)
        assert e.value.code == abi.BK_ERR_ARG and word in str(e.value), args
    L = capi.lib()
    out, n = C.c_void_p(), C.c_uint64()
    assert L.bk_split_junctions(t.h, QUAL, 2, 1, None, C.byref(n)) == abi.BK_ERR_ARG and b"null output" in L.bk_last_error(t.h)
    assert L.bk_split_junctions(t.h, QUAL, 2, 1, C.byref(out), None) == abi.BK_ERR_ARG
    assert L.bk_split_junction_counts(t.h, None) == abi.BK_ERR_ARG
    assert len(t.split_junctions(QUAL, 100, 1)) > 0  # the largest tol is accepted
    # timing: the scope and its byte model
    t.timing_enable(True)
    got = t.split_junctions(QUAL, 2, 1)
    cnt = t.split_junction_counts()
    names = [name for name, *_ in t.timing()]
    assert "split_junctions" in names
    touched = dict(zip(names, t.timing_touched()))["split_junctions"]
    bits = lambda v: int(v).bit_length()  # noqa: E731
    p1 = 8 + (2 * bits(2_000_000) + 7) // 8 + (bits(((3 * 4 + 3) << 2) | 3) + 7) // 8
    p2, p3 = (bits(cnt["eligible"]) + bits(cnt["exact"]) + 7) // 8, (bits(cnt["exact"]) + 7) // 8
    assert touched == (cnt["tuples"] * 96 + cnt["eligible"] * (123 + 36 * p1 + 132 + 64 + 24 + 36 * p2 + 48) + cnt["exact"] * (80 + 36 * p3 + 24) + cnt["calls"] * 84 + len(got) * 72)
    t.timing_enable(False)
    t.close()
    # a sharded context is refused
    s = capi.Context(CONTIGS)
    s.upload(designed["cols"])
    s.shard_begin(0, QUAL)
    with pytest.raises(capi.BreakIDError) as e:
        s.split_junctions(QUAL, 2, 1)
    assert e.value.code == abi.BK_ERR_ARG and "sharded" in str(e.value)
    s.close()


# ---- 11. the command line ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    """proper pairs; a 250-base deletion with 5 split reads and no discordant pair; a tandem duplication with 3; a junction with 2 reads
    between two genes; the first voted translocation of callcases.designed_tumor"""
    with tempfile.TemporaryDirectory() as tmp:
        ds = cc.designed_tumor(mix=False, n_proper=3000, loci=cc.LOCI[:1])
        ds.recs += reads_at("del", 5, 1, 1_700_000, "L", 1, 1_700_250, "R") + reads_at("dup", 3, 2, 200_400, "L", 2, 200_000, "R")
        ds.recs += reads_at("two", 2, 0, 305_000, "L", 1, 705_000, "R")
        ds.sort()
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        cols = ds.to_soa()
        t = capi.Context(ds.contigs)
        t.upload(cols)
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        splits = t.fetch(abi.STAGE_SPLITS)[0]
        t.close()
        base = [BIN, "-i", bam, "-n", side["nib"], "-fast", "-all"]
        runs = {}
        for name, extra in (("a", []), ("b", ["-junctions", "-bedpe"]), ("c", ["-junctions", "-jsupport", "2", "-jtol", "0"])):
            r = subprocess.run(base + ["-o", os.path.join(tmp, name)] + (["-bedpe"] if name == "a" else []) + extra, env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name] = r
        yield dict(tmp=tmp, cols=cols, cl=cl, splits=splits, runs=runs, base=base, env=env)


def expected_files(run, tol, support, sample):
    cols = run["cols"]
    rows = jc.expected(run["splits"], cols["flag"], cols["mapq"], TLEN, QUAL, tol, support, run["cl"])
    info = {}
    jc.expected(run["splits"], cols["flag"], cols["mapq"], TLEN, QUAL, tol, 1, run["cl"], info=info)
    endpos = cc.rec_endpos(cols)
    genes = {(0, 305_000): "GA_LR_x", (1, 705_000): "GB_LR_x"}
    lines, bed = ["\t".join(jc.COLUMNS)], []
    for i, r in enumerate(rows):
        if int(r["call"]) >= 0:
            continue
        ends = [(int(r["tid1"]), int(r["pos1"])), (int(r["tid2"]), int(r["pos2"]))]
        depth = [cc.single_base_depth(cols, endpos, t, p) for t, p in ends]
        lines.append("\t".join(jc.row_fields(i, r, NAMES, depth[0], depth[1], *[genes.get(e, "intergenic") for e in ends])))
        bed.append(jc.bedpe_line(i, r, NAMES, sample))
    stdout = "junctions: %d tuples eligible, %d exact, %d calls, %d claimed by a voted call, %d written" % (
        info["eligible"], info["exact"], len(rows), int((rows["call"] >= 0).sum()), len(lines) - 1)
    return "\n".join(lines) + "\n", "".join(l + "\n" for l in bed), stdout


def test_cli_junction_files(cli):
    tmp = cli["tmp"]
    table, bed, stdout = expected_files(cli, 2, 3, "b")
    got = open(os.path.join(tmp, "b_junctions.txt")).read()
    assert got == table, (got, table)
    rows = [l.split("\t") for l in got.split("\n")[1:-1]]
    # exactly the deletion and the duplication, in the order of the call's table; the translocation is claimed and counted
    assert [(f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]) for f in rows] == [("chr2", "1700000", "L", "chr2", "1700250", "R", "deletion", "250", "5"),
                                                                                       ("chr3", "200000", "R", "chr3", "200400", "L", "duplication", "400", "3")]
    assert all(f[15] == f[16] == "60.0" and f[21] == f[22] == "intergenic" and int(f[19]) > 0 for f in rows)
    assert stdout in cli["runs"]["b"].stdout.split("\n") and stdout.endswith("3 calls, 1 claimed by a voted call, 2 written")
    assert open(os.path.join(tmp, "b_junctions.bedpe")).read() == bed and bed.count("\n") == 2
    assert "junctions:" not in cli["runs"]["a"].stdout and not os.path.exists(os.path.join(tmp, "a_junctions.txt"))
    # -jsupport 2 adds the third junction, with its genes; -jtol 0 changes nothing here; no -bedpe, no BEDPE file
    table, _, stdout = expected_files(cli, 0, 2, "c")
    got = open(os.path.join(tmp, "c_junctions.txt")).read()
    assert got == table and got.count("\n") == 4 and "sj1\tchr1\t305000\tL\tchr2\t705000\tR\ttranslocation\t.\t2\t4\t1\t2\t2\t2\t60.0\t60.0\t305000-305000\t705000-705000" in got
    assert "\tGA_LR_x\tGB_LR_x\n" in got and stdout in cli["runs"]["c"].stdout.split("\n")
    assert not os.path.exists(os.path.join(tmp, "c_junctions.bedpe"))


def test_cli_every_other_file_is_unchanged(cli):
    tmp = cli["tmp"]
    files = sorted(f[2:] for f in os.listdir(tmp) if f.startswith("a_"))
    assert "fusion.txt" in files and "fusion_all.txt" in files and "fusion_all.bedpe" in files and "params.txt" in files
    assert sorted(f[2:] for f in os.listdir(tmp) if f.startswith("b_")) == sorted(files + ["junctions.txt", "junctions.bedpe"])
    a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    for f in files:
        ta, tb = open(os.path.join(tmp, "a_" + f), "rb").read(), open(os.path.join(tmp, "b_" + f), "rb").read()
        if f == "params.txt":
            assert tb.decode() == ta.decode().replace("out_file\t" + a, "out_file\t" + b) + "junction_min_support\t3\njunction_tol\t2\n"
        elif f == "performance.txt":  # (the last four columns are times)
            assert [l.split("\t")[:5] for l in ta.decode().split("\n")] == [l.split("\t")[:5] for l in tb.decode().split("\n")]
        elif f.endswith(".bedpe"):  # (the name column is the prefix's base name)
            assert ta.replace(b"\ta\t", b"\tb\t") == tb and ta.count(b"\ta\t") == ta.count(b"\n") > 0, f
        else:
            assert ta.replace(a.encode(), b.encode()) == tb, f
    quiet = lambda out: [l for l in out.split("\n") if "costs time" not in l and not l.startswith("junctions:")]  # noqa: E731
    assert quiet(cli["runs"]["a"].stdout) == quiet(cli["runs"]["b"].stdout.replace(b, a))
    assert open(os.path.join(tmp, "c_params.txt")).read().endswith("junction_min_support\t2\njunction_tol\t0\n")


def test_cli_junction_bedpe_is_a_known_panel(cli):
    tmp = cli["tmp"]
    panel = os.path.join(tmp, "b_junctions.bedpe")
    r = subprocess.run(cli["base"] + ["-o", os.path.join(tmp, "d"), "-known", panel, "-knownslop", "0"], env=cli["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "known: 2 entries, 0 on contigs the input lacks, 0 calls with a hit\n" in r.stdout and "Warning" not in r.stderr
    assert open(os.path.join(tmp, "d_fusion_all_known.txt")).read().count("\n") == 2  # the header and the translocation


def test_cli_refusals(cli):
    tmp = cli["tmp"]
    base = cli["base"] + ["-o", os.path.join(tmp, "z")]
    for args, word in ((["-jtol", "1"], "-jsupport and -jtol need -junctions."), (["-jsupport", "5"], "-jsupport and -jtol need -junctions."),
                       (["-junctions", "-gpus", "2"], "-junctions cannot be combined with -gpus."), (["-junctions", "-jsupport", "0"], "-jsupport must be a number from 1 to 1000000."),
                       (["-junctions", "-jsupport", "1000001"], "-jsupport must be a number from 1 to 1000000."), (["-junctions", "-jtol", "101"], "-jtol must be a number from 0 to 100."),
                       (["-junctions", "-jtol", "-1"], "-jtol must be a number from 0 to 100.")):
        r = subprocess.run(base + args, env=cli["env"], capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-500:])
    assert not any(f.startswith("z_") for f in os.listdir(tmp))

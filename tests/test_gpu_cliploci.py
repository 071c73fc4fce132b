"""Soft-clip loci (`bk_clip_loci`, `-cliploci`): the kernels against the two statements of tests/cliplocicases.py byte for byte.  No
events; event counts around the tiles of the scan and the radix sort and record counts around the tiles of the record pass; every kind
of dropped record alone and min_clip at its edges; the leading walk; a contig's end; the linkage under three tolerances; facing at every
offset around pair_dist, a window of more than 64 loci, a partner that is not mutual and one that min_reads drops; the claim; every
table form, two runs and a later bk_run; every refusal and the byte model; the identities with bk_clip_reads; and the command line's
files against the formatters."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import cliplocicases as lc

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = cc.CONTIGS
NAMES = cc.NAMES
TLEN = [l for _, l in CONTIGS]
NONE = lc.NONE


def assert_rows(got, exp):
    assert got.dtype == abi.CLIP_LOCUS and len(got) == len(exp), (len(got), len(exp))
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


class Case:
    """a context with a freshly uploaded table: no stage has run"""

    def __init__(self, recs, where="host", contigs=CONTIGS):
        self.cols = lc.dataset(contigs, recs).to_soa()
        self.tlen = [l for _, l in contigs]
        self.ctx, self.hold = cc.make_ctx(contigs, self.cols, where)

    def check(self, mapq_min=QUAL, min_clip=10, tol=2, pair_dist=50, min_reads=1):
        """the call against both statements; returns (rows, counts, info of the first statement)"""
        info = {}
        exp, counts = lc.both(self.cols, self.tlen, mapq_min, min_clip, tol, pair_dist, min_reads, None, info)
        got = self.ctx.clip_loci(None, mapq_min, min_clip, tol, pair_dist, min_reads)
        assert_rows(got, exp)
        assert self.ctx.clip_locus_counts() == counts
        return got, counts, info

    def reasons(self, mapq_min=QUAL, min_clip=10):
        return [lc.why_dropped(self.cols, i, self.tlen, mapq_min, min_clip) for i in range(len(self.cols["tid"]))]

    def close(self):
        self.ctx.close()


def background(n=40, seed=3):
    rng = np.random.default_rng(seed)
    return [r for i in range(n) for r in synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)]


# ---- 1. no events ----------------------------------------------------------------------------------------------------------------------
def test_no_events():
    c = Case([])
    got, counts, _ = c.check()
    assert len(got) == 0 and counts == dict(zip(lc.COUNTS, [0] * 8))
    c.close()
    c = Case(background(200) + [lc.read("gap%d" % k, 1, 5000 + 10 * k, "30M25D30M9S") for k in range(50)])
    got, counts, _ = c.check()
    assert len(got) == 0 and counts["records"] == counts["eligible"] == 450 and counts["events"] == counts["beyond"] == 0
    c.close()


def test_hand_example():
    contigs, recs = lc.hand_example()
    c = Case(recs, contigs=contigs)
    got, counts, _ = c.check()
    assert counts == dict(zip(lc.COUNTS, (10, 8, 7, 0, 4, 3, 2, 3)))
    assert [(int(r["pos"]), int(r["dir"]), int(r["n_reads"]), int(r["flags"]), int(r["mate"]), int(r["mate_off"])) for r in got] == [
        (999, 0, 4, 3, 1, -9), (990, 1, 2, 3, 0, -9), (5001, 1, 1, 0, NONE, 0)]
    c.close()


# ---- 2. sizes ----------------------------------------------------------------------------------------------------------------------------
def sized_recs(e, n_sites):
    """e events: one record with two, the others with one, LEFT and RIGHT in turn over n_sites blunt sites 200 bases apart"""
    recs = background(20) + [lc.read("two", 2, 50_000, "20S60M20S")]
    for k in range(e - 2):
        p = 10_000 + 200 * ((k // 2) % n_sites)
        recs.append(lc.left_clip("z%d" % k, 0, p) if k % 2 == 0 else lc.right_clip("z%d" % k, 0, p + 1))
    return recs


def size_cases():
    p = capi.prims_info()
    assert p["SCAN_TILE"] == p["RS_TILE"]  # (one list serves both; were they to differ, both lists would be needed)
    t = p["RS_TILE"]
    return [t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 301, p["SCAN_ONE_MAX"] + 2]


@pytest.mark.parametrize("which", range(8))
def test_event_counts_across_boundaries(which):
    e = size_cases()[which]
    c = Case(sized_recs(e, 300))
    got, counts, _ = c.check()
    assert counts["events"] == e and int(got["n_rows"].sum()) == e and counts["exact"] == len(got) == 602 and counts["mutual"] == 600
    c.close()


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025])
def test_record_counts_around_the_tiles(n):
    """events in the first and the last record of the table and of every tile boundary inside it"""
    marked = {i for i in (0, 255, 256, 1023, 1024, n - 1) if i < n}
    recs = [lc.read("b%d" % i, 0, 1000 + 150 * i, "60M40S" if i in marked else "100M") for i in range(n)]
    c = Case(recs)
    assert [int(p) for p in c.cols["pos"][:3]] == [1000, 1150, 1300]  # record i is the i-th of the table
    got, counts, _ = c.check()
    assert counts["records"] == n and counts["events"] == len(got) == len(marked)
    assert [int(p) for p in got["pos"]] == [1000 + 150 * i + 60 for i in sorted(marked)]
    c.close()


# ---- 3. dropped records, each alone ------------------------------------------------------------------------------------------------------
def dropped_read(kind):
    if kind.startswith("flag"):
        return lc.left_clip("drop", 2, 500_000, flag=lc.PROPER | int(kind[4:], 16))
    if kind == "unmapped":
        return lc.read("drop", -1, 100, "60M40S")
    if kind == "mapq":
        return lc.left_clip("drop", 2, 500_000, mapq=QUAL - 1)
    if kind == "mapq_at":
        return lc.left_clip("drop", 2, 500_000, mapq=QUAL)
    if kind == "aux":
        return lc.left_clip("drop", 2, 500_000, sa=lc.SA)
    if kind == "no_ref":
        return lc.read("drop", 2, 500_000, "40S60I")
    if kind == "no_cigar":
        return lc.read("drop", 2, 500_000, "*")
    if kind == "no_clip":
        return lc.read("drop", 2, 500_000, "100M")
    assert kind == "short"
    return lc.left_clip("drop", 2, 500_000, m=91, s=9)


@pytest.mark.parametrize("kind", ["flag4", "flag100", "flag200", "flag400", "flag800", "unmapped", "mapq", "mapq_at", "aux", "no_ref", "no_cigar", "no_clip", "short"])
def test_dropped_records_each_alone(kind):
    c = Case(background() + [lc.left_clip("good%d" % k, 0, 300_000) for k in range(3)] + [dropped_read(kind)])
    reasons = [r for r in c.reasons() if r not in (None, "no_clip")] + (["no_clip"] if kind == "no_clip" else [])
    kept = kind.endswith("_at")
    want = kind[:4] if kind.startswith("flag") else "no_ref" if kind == "no_cigar" else kind
    assert reasons == ([] if kept else [want]), reasons
    got, counts, _ = c.check()
    assert len(got) == (2 if kept else 1) and int(got[0]["n_reads"]) == 3 and counts["events"] == (4 if kept else 3)
    assert counts["eligible"] == 80 + 3 + (kind in ("mapq_at", "no_clip", "short"))
    if kind == "mapq":
        got, counts, _ = c.check(mapq_min=QUAL - 1)
        assert len(got) == 2 and counts["events"] == 4
    c.close()


def test_min_clip_edges():
    c = Case(background() + [lc.read("both", 1, 400_000, "25S50M25S")])
    for min_clip, n in ((24, 2), (25, 2), (26, 0), (1, 2)):
        got, counts, _ = c.check(min_clip=min_clip)
        assert counts["events"] == n == len(got)
    c.close()


# ---- 4. the leading walk and a contig's end -----------------------------------------------------------------------------------------------
WALK = [("5H30S65M", [(1, 1)]),                     # a leading clip behind H
        ("30S5I100M", [(1, 1)]),                    # no aligned base follows the clip at once
        ("30S65M5H", [(1, 1)]), ("65M30S5H", [(0, 65)]), ("3H2H12S60M12S5H", [(1, 1), (0, 60)]),
        ("30S5I", []), ("5H30S", []), ("5H", []), ("30S40N30S", [(1, 1), (0, 40)]),  # N has a reference length
        ("30S20M10D20M", [(1, 1)]), ("20M10D20M30S", [(0, 50)]), ("20=5X30S", [(0, 25)]), ("30S2P20M", [(1, 1)])]


def test_leading_walk_and_every_operation():
    recs = background()
    for k, (cigar, _) in enumerate(WALK):
        recs.append(lc.read("w%d" % k, 0, 10_000 * (k + 1), cigar))
    c = Case(recs)
    got, counts, info = c.check()
    want = sorted((d, 0, 10_000 * (k + 1) + off) for k, (_, ev) in enumerate(WALK) for d, off in ev)
    assert info["exact_keys"] == want and counts["events"] == len(want) == len(got)
    c.close()


def test_contig_end():
    end = 2_000_000
    recs = background() + [lc.left_clip("at", 3, end), lc.left_clip("past", 3, end + 1), lc.right_clip("lead_at", 2, end, m=1),
                           lc.read("mid", 1, 5000, "30S70M", flag=0x1 | 0x40)]
    c = Case(recs)
    got, counts, _ = c.check()
    assert counts["events"] == 4 and counts["beyond"] == 1 and sorted((int(r["tid"]), int(r["pos"])) for r in got) == [(1, 5001), (2, end), (3, end)]
    assert [int(r["n_improper"]) for r in got if int(r["tid"]) == 1] == [1]
    c.close()


# ---- 5. linkage ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linkage():
    """pairs of sites 0 1 2 3 100 101 apart; chains of 70 sites 2 and 100 apart; a LEFT and a RIGHT site at one position; one position
    on four contigs"""
    recs = background()
    for k, d in enumerate((0, 1, 2, 3, 100, 101)):
        recs += [lc.left_clip("sa%d" % k, 0, 100_000 + 1000 * k), lc.left_clip("sb%d" % k, 0, 100_000 + 1000 * k + d)]
    for k in range(70):
        recs += [lc.right_clip("c2_%d" % k, 2, 100_000 + 2 * k), lc.right_clip("c100_%d" % k, 2, 300_000 + 100 * k)]
    recs += [lc.left_clip("kl", 3, 100_000), lc.right_clip("kr", 3, 100_000)]
    recs += [lc.left_clip("t%d" % t, t, 700_000) for t in range(4)]
    c = Case(recs)
    yield c
    c.close()


@pytest.mark.parametrize("tol", [0, 2, 100])
def test_linkage(linkage, tol):
    got, counts, _ = linkage.check(tol=tol, pair_dist=0)
    on = lambda tid, lo, hi: got[(got["tid"] == tid) & (got["pos"] >= lo) & (got["pos"] < hi)]  # noqa: E731
    assert len(on(0, 100_000, 110_000)) == sum(1 if d <= tol else 2 for d in (0, 1, 2, 3, 100, 101))
    c2, c100 = on(2, 100_000, 200_000), on(2, 300_000, 400_000)
    assert len(c2) == (70 if tol < 2 else 1) and len(c100) == (70 if tol < 100 else 1)
    if tol >= 2:
        assert (int(c2[0]["n_exact"]), int(c2[0]["lo_pos"]), int(c2[0]["hi_pos"]), int(c2[0]["pos"])) == (70, 100_000, 100_138, 100_000)
    assert [int(k) for k in on(3, 100_000, 100_001)["dir"]] == [0, 1] and len(got[got["pos"] == 700_000]) == 4
    assert counts["exact"] >= counts["loci"] == len(got)


def test_distinct_reads_tie_and_strands():
    recs = background()
    # one read twice in one locus (its two mates): one read, two rows; one read name in two loci
    recs += [lc.left_clip("mates", 0, 200_000, flag=lc.PROPER | 0x40), lc.left_clip("mates", 0, 200_001, flag=lc.PROPER | 0x80 | 0x10)]
    recs += [lc.left_clip("twice", 1, 200_000), lc.left_clip("twice", 1, 900_000), lc.left_clip("other", 1, 900_000)]
    # a tie of the representative: 300 001 and 300 000 with two reads each; then a third read makes the later one win
    recs += [lc.right_clip("t%d" % k, 2, 300_001, s=30) for k in range(2)] + [lc.right_clip("u%d" % k, 2, 300_000, s=45, flag=0x10, mapq=33) for k in range(2)]
    recs += [lc.right_clip("v%d" % k, 2, 500_000) for k in range(2)] + [lc.right_clip("w%d" % k, 2, 500_002, flag=0x1 | 0x8) for k in range(3)]
    c = Case(recs)
    got, counts, _ = c.check()
    by = {(int(r["tid"]), int(r["lo_pos"])): r for r in got}
    m = by[(0, 200_000)]
    assert (int(m["n_reads"]), int(m["n_rows"]), int(m["n_exact"]), int(m["n_fwd"]), int(m["n_rev"])) == (1, 2, 2, 1, 1)
    assert int(by[(1, 200_000)]["n_reads"]) == 1 and int(by[(1, 900_000)]["n_reads"]) == 2
    t = by[(2, 300_000)]
    assert (int(t["pos"]), int(t["top_reads"]), int(t["n_reads"]), int(t["n_rev"]), int(t["max_clip"]), int(t["clip_sum"]), int(t["mapq_sum"])) == (300_000, 2, 4, 2, 45, 150, 186)
    t = by[(2, 500_000)]
    assert (int(t["pos"]), int(t["top_reads"]), int(t["n_reads"]), int(t["n_orphan"]), int(t["hi_pos"])) == (500_002, 3, 5, 3, 500_002)
    c.close()


# ---- 6. facing -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facing():
    """a LEFT site with two reads every 1000 bases and a RIGHT site with one read at every offset -52 .. 52 around blunt"""
    recs = background()
    for k, off in enumerate(range(-52, 53)):
        p = 100_000 + 1000 * k
        recs += [lc.left_clip("fl%d_%d" % (k, j), 1, p) for j in range(2)] + [lc.right_clip("fr%d" % k, 1, p + 1 + off)]
    c = Case(recs)
    yield c
    c.close()


@pytest.mark.parametrize("pair_dist", [0, 50])
def test_facing_offsets_around_pair_dist(facing, pair_dist):
    got, counts, _ = facing.check(pair_dist=pair_dist)
    left = got[got["dir"] == 0]
    assert len(left) == 105
    for k, off in enumerate(range(-52, 53)):
        r = left[k]
        assert int(r["pos"]) == 100_000 + 1000 * k
        if abs(off) <= pair_dist:
            assert (int(r["flags"]), int(r["mate_off"]), int(r["mate_pos"]), int(r["mate_reads"])) == (3, off + 1, int(r["pos"]) + 1 + off, 1), (off, r)
            assert int(got[int(r["mate"])]["mate"]) == k and int(got[int(r["mate"])]["mate_off"]) == off + 1
        else:
            assert (int(r["flags"]), int(r["mate"]), int(r["mate_off"]), int(r["mate_pos"])) == (0, NONE, 0, 0), (off, r)
    assert counts["mutual"] == 2 * (2 * pair_dist + 1)


def test_facing_window_of_more_than_64_loci_partner_rules():
    recs = background()
    # 101 RIGHT loci (tol 0) inside the window of one LEFT locus; the two with two reads lie 50 away on either side: the smaller position wins
    p = 400_000
    recs += [lc.left_clip("wl", 0, p)] + [lc.right_clip("wr%d" % k, 0, p + 1 - 50 + k) for k in range(101)]
    recs += [lc.right_clip("wx", 0, p + 1 - 50), lc.right_clip("wy", 0, p + 1 + 50)]
    # a partner that is not mutual: A (3 reads) and C (5) both face B (2); B faces C
    q = 800_000
    recs += [lc.left_clip("a%d" % k, 2, q) for k in range(3)] + [lc.right_clip("b%d" % k, 2, q + 1) for k in range(2)] + [lc.left_clip("c%d" % k, 2, q + 10) for k in range(5)]
    # equal reads: the smaller distance wins
    recs += [lc.left_clip("d", 3, q)] + [lc.right_clip("e1", 3, q + 1 + 7), lc.right_clip("e2", 3, q + 1 - 6)]
    c = Case(recs)
    got, counts, _ = c.check(tol=0, pair_dist=50)
    w = got[(got["tid"] == 0) & (got["dir"] == 0)][0]
    assert (int(w["mate_pos"]), int(w["mate_reads"]), int(w["mate_off"]), int(w["flags"])) == (p - 49, 2, -49, 3)
    a, cc_ = got[(got["tid"] == 2) & (got["dir"] == 0)]
    b = got[(got["tid"] == 2) & (got["dir"] == 1)][0]
    assert (int(a["flags"]), int(a["mate_pos"])) == (1, q + 1) and (int(cc_["flags"]), int(cc_["mate_pos"])) == (3, q + 1) and (int(b["flags"]), int(b["mate_pos"])) == (3, q + 10)
    assert int(b["mate_off"]) == -9 and int(a["mate_off"]) == 1
    d = got[(got["tid"] == 3) & (got["dir"] == 0)][0]
    assert (int(d["mate_pos"]), int(d["mate_off"])) == (q + 1 - 6, -5)
    # min_reads drops the partner: mate is NONE, the rest stays filled
    got2, _, _ = c.check(tol=0, pair_dist=50, min_reads=3)
    assert [(int(r["pos"]), int(r["flags"]), int(r["mate"]), int(r["mate_pos"]), int(r["mate_reads"])) for r in got2] == [(q, 1, NONE, q + 1, 2), (q + 10, 3, NONE, q + 1, 2)]
    c.close()


# ---- 7. claim, table forms ------------------------------------------------------------------------------------------------------------------
CLAIM_LOCI = [("a", 0, 300_000, "L", 1, 700_000, "R"), ("b", 1, 700_090, "R", 3, 900_000, "R")]


def clip_reads():
    """chr2: RIGHT clips at 700 002 and 700 088 (one locus at tol 100, two voted breakpoints at its -2 and +2); chr1: LEFT clips at
    299 998 (-2), 299 997 (-3) and 300 003 (+3); chr3: a blunt mutual pair inside a gene and an orphan locus"""
    recs = [lc.right_clip("ca%d" % k, 1, 700_002) for k in range(3)] + [lc.right_clip("cb%d" % k, 1, 700_088) for k in range(3)]
    recs += [lc.left_clip("cc%d" % k, 0, 299_998) for k in range(3)] + [lc.left_clip("cd%d" % k, 0, 299_997) for k in range(3)] + [lc.left_clip("ce%d" % k, 0, 300_003) for k in range(4)]
    recs += [lc.left_clip("ml%d" % k, 2, 1_200_000) for k in range(4)] + [lc.right_clip("mr%d" % k, 2, 1_199_991, flag=0x1 | 0x8 | 0x40) for k in range(3)]
    recs += [lc.right_clip("or%d" % k, 2, 1_500_000, flag=0x1 | 0x8 | 0x80 | 0x10, mapq=30 + k) for k in range(3)]
    return recs


@pytest.fixture(scope="module")
def designed():
    ds = cc.designed_tumor(mix=False, n_proper=3000, loci=CLAIM_LOCI)
    ds.recs += clip_reads()
    ds.sort()
    cols = ds.to_soa()
    ref = capi.Context(CONTIGS)  # a context that never makes the call
    ref.upload(cols)
    ref.run(qual=QUAL, fast=True)
    fetched = {st: ref.fetch(st)[0].tobytes() for st in (abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)}
    clusters = ref.fetch(abi.STAGE_CLUSTERS)[0].copy()
    ref.close()
    return dict(ds=ds, cols=cols, fetched=fetched, clusters=clusters)


def test_claim(designed):
    cols, cl = designed["cols"], designed["clusters"]
    ra, rb = cc.rows_of(cl, 0, 300_000, 1, 700_000), cc.rows_of(cl, 1, 700_090, 3, 900_000)
    assert len(ra) == 1 and len(rb) == 1, (ra, rb, cl)
    t = capi.Context(CONTIGS)
    t.upload(cols)
    exp, counts = lc.both(cols, TLEN, QUAL, 10, 100, 50, 1)
    assert_rows(t.clip_loci(None, QUAL, 10, 100, 50, 1), exp)  # calls NULL, before any stage
    assert np.all(exp["claim"] == NONE)
    t.run(qual=QUAL, fast=True)
    assert t.fetch(abi.STAGE_CLUSTERS)[0].tobytes() == cl.tobytes()
    # tol 100: the chr2 locus 700 002 .. 700 088 is claimed by both rows, the smaller one is named
    exp, counts = lc.both(cols, TLEN, QUAL, 10, 100, 50, 1, cl)
    got = t.clip_loci(t, QUAL, 10, 100, 50, 1)
    assert_rows(got, exp)
    two = got[(got["tid"] == 1) & (got["dir"] == 1)]
    assert len(two) == 1 and (int(two[0]["lo_pos"]), int(two[0]["hi_pos"]), int(two[0]["claim"])) == (700_002, 700_088, min(ra[0][0], rb[0][0]))
    # tol 0: +-2 claims, +-3 does not
    exp, counts = lc.both(cols, TLEN, QUAL, 10, 0, 50, 1, cl)
    got = t.clip_loci(t, QUAL, 10, 0, 50, 1)
    assert_rows(got, exp)
    assert t.clip_locus_counts() == counts
    claim = {int(r["pos"]): int(r["claim"]) for r in got if int(r["tid"]) == 0}
    assert claim == {299_997: NONE, 299_998: ra[0][0], 300_003: NONE}
    assert {int(r["pos"]): int(r["claim"]) for r in got if int(r["tid"]) == 1} == {700_002: ra[0][0], 700_088: rb[0][0]}
    # another context as `calls`, with the same reference list; one with another list is refused
    other = capi.Context(CONTIGS)
    other.upload(cols)
    assert_rows(other.clip_loci(t, QUAL, 10, 0, 50, 1), exp)
    other.close()
    odd = capi.Context(CONTIGS[:3] + [("chrX", 2_000_000)])
    odd.upload(cols)
    with pytest.raises(capi.BreakIDError) as e:
        odd.clip_loci(t)
    assert e.value.code == abi.BK_ERR_ARG
    odd.close()
    t.close()


@pytest.mark.parametrize("form", ["host", "device", "exclude_host", "exclude_device", "decode_ctx"])
def test_table_forms(form, designed):
    hold = None
    cols = designed["cols"]
    if form == "decode_ctx":
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            designed["ds"].write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        t, hold = cc.make_ctx(CONTIGS, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            tid, beg, end = np.asarray([2, 0], np.int32), np.asarray([1_199_000, 0], np.int32), np.asarray([1_201_000, 5_000], np.int32)
            assert t.exclude_regions(tid, beg, end) > 6
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, tid, beg, end))
    for tol, min_reads in ((2, 1), (0, 4)):
        exp, counts = lc.both(cols, TLEN, QUAL, 10, tol, 50, min_reads)
        got = t.clip_loci(None, QUAL, 10, tol, 50, min_reads)
        assert_rows(got, exp)
        assert t.clip_locus_counts() == counts
        assert t.clip_loci(None, QUAL, 10, tol, 50, min_reads).tobytes() == got.tobytes()  # two runs, the same bytes
    assert [(int(r["tid"]), int(r["pos"])) for r in got] == ([(0, 300_003)] if form.startswith("exclude") else [(0, 300_003), (2, 1_200_000)])
    if form == "host":  # a later bk_run and bk_fetch return what they return without the call
        t.run(qual=QUAL, fast=True)
        for st, want in designed["fetched"].items():
            assert t.fetch(st)[0].tobytes() == want
        assert t.clip_loci(None, QUAL, 10, 0, 50, 4).tobytes() == got.tobytes()
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


# ---- 8. refusals and timing ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_timing(designed):
    import ctypes as C
    t = capi.Context(CONTIGS)
    with pytest.raises(capi.BreakIDError) as e:
        t.clip_loci()
    assert e.value.code == abi.BK_ERR_ARG and "holds no record table" in str(e.value)
    t.upload(designed["cols"])
    for kw, word in ((dict(mapq_min=-1), "mapq_min below 0"), (dict(min_clip=0), "min_clip must be at least 1"), (dict(tol=101), "tol above 100"),
                     (dict(pair_dist=100_001), "pair_dist above 100000"), (dict(min_reads=0), "min_reads must be at least 1"),
                     (dict(calls=t), "call bk_split_breakpoints on the calls context first")):
        with pytest.raises(capi.BreakIDError) as e:
            t.clip_loci(**kw)
        assert e.value.code == abi.BK_ERR_ARG and word in str(e.value), kw
    L = capi.lib()
    out, n = C.c_void_p(), C.c_uint64()
    assert L.bk_clip_loci(t.h, None, QUAL, 10, 2, 50, 3, None, C.byref(n)) == abi.BK_ERR_ARG and b"null output" in L.bk_last_error(t.h)
    assert L.bk_clip_loci(t.h, None, QUAL, 10, 2, 50, 3, C.byref(out), None) == abi.BK_ERR_ARG and b"null output" in L.bk_last_error(t.h)
    assert L.bk_clip_locus_counts(t.h, None) == abi.BK_ERR_ARG and b"null out" in L.bk_last_error(t.h)
    assert len(t.clip_loci(tol=100, pair_dist=100_000, min_reads=1)) == 5  # the largest values are accepted
    # timing: the scope and its byte model, recomputed from the counts
    t.run(qual=QUAL, fast=True)
    t.timing_enable(True)
    for calls in (None, t):
        got = t.clip_loci(calls, QUAL, 10, 2, 50, 1)
        cnt = t.clip_locus_counts()
        names = [name for name, *_ in t.timing()]
        touched = dict(zip(names, t.timing_touched()))
        bits = lambda v: int(v).bit_length()  # noqa: E731
        tiles, ev = (cnt["records"] + 255) // 256, cnt["events"] - cnt["beyond"]
        records = 15 * cnt["records"] + 56 * tiles + 2816 * min(ev, tiles) + 48 * ev
        p2, p3 = (bits(2_000_000) + bits(3) + 1 + 7) // 8, (bits(cnt["loci"]) + bits(ev) + 7) // 8
        b = 2 * len(designed["clusters"]) if calls is not None else 0
        model = ev * (36 * (8 + p2 + p3) + 376) + 176 * cnt["loci"] + 224 * len(got) + b * (36 * ((33 + bits(3) + 7) // 8) + 40)
        assert ev == 26 and len(got) == 7 and (b > 0) == (calls is not None)
        assert (touched["clip_loci_records"], touched["clip_loci_calls"], touched["clip_loci"]) == (records, model, records + model)
    t.timing_enable(False)
    t.close()
    # a sharded context is refused
    s = capi.Context(CONTIGS)
    s.upload(designed["cols"])
    s.shard_begin(0, QUAL)
    with pytest.raises(capi.BreakIDError) as e:
        s.clip_loci()
    assert e.value.code == abi.BK_ERR_ARG and "sharded" in str(e.value)
    s.close()


# ---- 9. identities with merged code ---------------------------------------------------------------------------------------------------------
def test_identities_with_clip_reads():
    rng = np.random.default_rng(77)
    tlen = [3000, 1500, 800]
    contigs = [("c%d" % k, l) for k, l in enumerate(tlen)]
    cols = lc.random_cols(rng, 3000, tlen)
    t = capi.Context(contigs)
    t.upload(cols)
    exp, counts = lc.both(cols, tlen, QUAL, 10, 2, 50, 1)
    got = t.clip_loci(None, QUAL, 10, 2, 50, 1)
    assert_rows(got, exp)
    assert t.clip_locus_counts() == counts and counts["beyond"] > 0 and counts["mutual"] > 0
    assert int(got["n_rows"].sum()) == counts["events"] - counts["beyond"]
    single = got[got["lo_pos"] == got["hi_pos"]]
    assert len(single) > 20
    t.isize_stats()
    sites = np.zeros(len(single), abi.CLIP_SITE)
    sites["tid"], sites["pos"], sites["tol"], sites["dir"] = single["tid"], single["pos"], 0, single["dir"]
    n = t.clip_reads(sites, QUAL, 10, listing=False)
    n = n[0] if isinstance(n, tuple) else n
    assert [int(v) for v in n] == [int(v) for v in single["n_rows"]]
    assert t.clip_loci(None, QUAL, 10, 2, 50, 1).tobytes() == got.tobytes()  # after a stage, the same bytes
    t.close()


# ---- 10. the command line ------------------------------------------------------------------------------------------------------------------
EXCLUDE = (np.asarray([2], np.int32), np.asarray([1_199_000], np.int32), np.asarray([1_201_000], np.int32))


@pytest.fixture(scope="module")
def cli(designed):
    with tempfile.TemporaryDirectory() as tmp:
        ds = designed["ds"]
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        bed = os.path.join(tmp, "x.bed")
        with open(bed, "w") as f:
            for t, s, e in zip(*EXCLUDE):
                f.write("%s\t%d\t%d\n" % (NAMES[t], s, e))
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        base = [BIN, "-i", bam, "-n", side["nib"], "-fast"]
        runs = {}
        for name, extra in (("a", ["-all", "-bedpe"]), ("b", ["-all", "-cliploci", "-bedpe"]),
                            ("c", ["-all", "-cliploci", "-locisupport", "4", "-locitol", "0", "-locipair", "8", "-minclip", "40"]), ("d", ["-cliploci", "-x", bed])):
            r = subprocess.run(base + ["-o", os.path.join(tmp, name)] + extra, env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name] = r
        # the clusters of the run with -x, for its claims
        t = capi.Context(CONTIGS)
        t.upload(designed["cols"])
        t.exclude_regions(*EXCLUDE)
        t.run(qual=QUAL, fast=True)
        x_clusters = t.fetch(abi.STAGE_CLUSTERS)[0].copy()
        t.close()
        x_cols = cc.filtered(designed["cols"], ~cc.excluded_mask(designed["cols"], *EXCLUDE))
        yield dict(tmp=tmp, cols=designed["cols"], clusters=designed["clusters"], x_cols=x_cols, x_clusters=x_clusters, runs=runs, base=base, env=env)


def expected_files(cols, cl, sample, min_clip=10, tol=2, pair_dist=50, min_reads=3):
    rows, counts = lc.both(cols, TLEN, QUAL, min_clip, tol, pair_dist, min_reads, cl)
    endpos = cc.rec_endpos(cols)
    lines = ["\t".join(lc.COLUMNS)]
    for i in lc.written(rows):
        r = rows[i]
        tid, pos = int(r["tid"]), int(r["pos"])
        gene = "GA_LR_x" if tid == 0 and 290_000 <= pos <= 310_000 else "GB_LR_x" if tid == 1 and 690_000 <= pos <= 710_000 else "intergenic"
        lines.append("\t".join(lc.row_fields(i, r, rows, NAMES, cc.single_base_depth(cols, endpos, tid, pos), gene)))
    bed = [lc.bedpe_line(i, j, rows, NAMES, sample) for i, j in lc.bedpe_pairs(rows)]
    return "\n".join(lines) + "\n", "".join(l + "\n" for l in bed), lc.stdout_line(counts, rows)


def test_cli_cliploci_files(cli):
    tmp = cli["tmp"]
    table, bed, stdout = expected_files(cli["cols"], cli["clusters"], "b")
    got = open(os.path.join(tmp, "b_cliploci.txt")).read()
    assert got == table, (got, table)
    rows = [l.split("\t") for l in got.split("\n")[1:-1]]
    # the loci at chr1:299 997-299 998 and the two on chr2 are claimed: their numbers are missing
    assert [f[:5] for f in rows] == [["cl1", "chr1", "300003", "L", "4"], ["cl2", "chr3", "1200000", "L", "4"], ["cl5", "chr3", "1199991", "R", "3"], ["cl6", "chr3", "1500000", "R", "3"]]
    assert rows[1][16:21] == ["cl5", "1199991", "3", "-9", "1"] and rows[2][16:21] == ["cl2", "1200000", "4", "-9", "1"] and rows[3][14] == "3" and rows[0][22] == "GA_LR_x"
    assert stdout in cli["runs"]["b"].stdout.split("\n") and stdout.endswith("26 events, 0 beyond a contig's end, 8 exact, 7 loci, 2 with a mutual partner, 3 claimed by a voted call, 4 written")
    assert open(os.path.join(tmp, "b_cliploci.bedpe")).read() == bed == "chr3\t1199999\t1200000\tchr3\t1199990\t1199991\tb\t7\t+\t-\tcl2\tinsertion_site\t0\t7\n"
    assert "cliploci:" not in cli["runs"]["a"].stdout and not os.path.exists(os.path.join(tmp, "a_cliploci.txt"))
    # the dials: -locisupport 4 and -locitol 0 leave two loci, -locipair 8 ends their facing; no -bedpe, no BEDPE file
    table, _, stdout = expected_files(cli["cols"], cli["clusters"], "c", min_clip=40, tol=0, pair_dist=8, min_reads=4)
    got = open(os.path.join(tmp, "c_cliploci.txt")).read()
    assert got == table and got.count("\n") == 3 and stdout in cli["runs"]["c"].stdout.split("\n")
    assert not os.path.exists(os.path.join(tmp, "c_cliploci.bedpe"))
    assert open(os.path.join(tmp, "c_params.txt")).read().endswith("cliploci_tol\t0\ncliploci_pair\t8\ncliploci_min_support\t4\n")
    # -x by itself: the excluded interval's loci are gone; without -all the file is made the same way
    table, _, stdout = expected_files(cli["x_cols"], cli["x_clusters"], "d")
    got = open(os.path.join(tmp, "d_cliploci.txt")).read()
    assert got == table and [l.split("\t")[2] for l in got.split("\n")[1:-1]] == ["300003", "1500000"] and stdout in cli["runs"]["d"].stdout.split("\n")


def test_cli_every_other_file_is_unchanged(cli):
    tmp = cli["tmp"]
    files = sorted(f[2:] for f in os.listdir(tmp) if f.startswith("a_"))
    assert "fusion.txt" in files and "fusion_all.txt" in files and "fusion_all.bedpe" in files and "params.txt" in files
    assert sorted(f[2:] for f in os.listdir(tmp) if f.startswith("b_")) == sorted(files + ["cliploci.txt", "cliploci.bedpe"])
    a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    for f in files:
        ta, tb = open(os.path.join(tmp, "a_" + f), "rb").read(), open(os.path.join(tmp, "b_" + f), "rb").read()
        if f == "params.txt":
            assert tb.decode() == ta.decode().replace("out_file\t" + a, "out_file\t" + b) + "cliploci_tol\t2\ncliploci_pair\t50\ncliploci_min_support\t3\n"
        elif f == "performance.txt":  # (the last four columns are times)
            assert [l.split("\t")[:5] for l in ta.decode().split("\n")] == [l.split("\t")[:5] for l in tb.decode().split("\n")]
        elif f.endswith(".bedpe"):  # (the name column is the prefix's base name)
            assert ta.replace(b"\ta\t", b"\tb\t") == tb and ta.count(b"\ta\t") == ta.count(b"\n") > 0, f
        else:
            assert ta.replace(a.encode(), b.encode()) == tb, f
    quiet = lambda out: [l for l in out.split("\n") if "costs time" not in l and not l.startswith("cliploci:")]  # noqa: E731
    assert quiet(cli["runs"]["a"].stdout) == quiet(cli["runs"]["b"].stdout.replace(b, a))


def test_cli_refusals(cli):
    tmp = cli["tmp"]
    base = cli["base"] + ["-o", os.path.join(tmp, "z")]
    need = "-locitol, -locipair and -locisupport need -cliploci."
    for args, word in ((["-locitol", "1"], need), (["-locipair", "5"], need), (["-locisupport", "5"], need),
                       (["-minclip", "5"], "-minclip and -clipsupport need -clip."),
                       (["-cliploci", "-gpus", "2"], "-cliploci cannot be combined with -gpus."),
                       (["-cliploci", "-minclip", "0"], "-minclip must be a number from 1 to 2147483647."),
                       (["-cliploci", "-locitol", "101"], "-locitol must be a number from 0 to 100."), (["-cliploci", "-locitol", "-1"], "-locitol must be a number from 0 to 100."),
                       (["-cliploci", "-locipair", "100001"], "-locipair must be a number from 0 to 100000."),
                       (["-cliploci", "-locisupport", "0"], "-locisupport must be a number from 1 to 1000000."),
                       (["-cliploci", "-locisupport", "1000001"], "-locisupport must be a number from 1 to 1000000.")):
        r = subprocess.run(base + args, env=cli["env"], capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-500:])
    assert not any(f.startswith("z_") for f in os.listdir(tmp))

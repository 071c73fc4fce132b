"""CIGAR gaps (`bk_cigar_gaps`, `-gaps`): the kernels against the two statements of tests/gapcases.py byte for byte.  No events; event
counts around the tiles of the scan and the radix sort and record counts around a tile of the record pass; the walk over every
operation and every bound; every kind of dropped record alone; the two linkages under three tolerances; distinct reads, the
representative's tie rule and the strands; min_reads; every table form, two runs and a later bk_run; every refusal and the byte model;
and the command line's files against the formatters."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import gapcases as gc

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = cc.CONTIGS
NAMES = cc.NAMES
TLEN = [l for _, l in CONTIGS]
PAIRED_FWD, PAIRED_REV = 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x80 | 0x10


def assert_rows(got, exp):
    assert got.dtype == abi.CIGAR_GAP and len(got) == len(exp), (len(got), len(exp))
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


class Case:
    """a context with a freshly uploaded table: no stage has run"""

    def __init__(self, recs, where="host", contigs=CONTIGS):
        self.cols = gc.dataset(contigs, recs).to_soa()
        self.tlen = [l for _, l in contigs]
        self.ctx, self.hold = cc.make_ctx(contigs, self.cols, where)

    def check(self, mapq_min=QUAL, min_len=20, anchor=10, tol=2, min_reads=1):
        """the call against both statements; returns (rows, counts, info of the first statement)"""
        info = {}
        exp, counts = gc.both(self.cols, self.tlen, mapq_min, min_len, anchor, tol, min_reads, info)
        got = self.ctx.cigar_gaps(mapq_min, min_len, anchor, tol, min_reads)
        assert_rows(got, exp)
        assert self.ctx.cigar_gap_counts() == counts
        return got, counts, info

    def reasons(self, **kw):
        p = dict(mapq_min=QUAL, min_len=20, anchor=10)
        p.update(kw)
        return [gc.why_dropped(self.cols, i, self.tlen, p["mapq_min"], p["min_len"], p["anchor"]) for i in range(len(self.cols["tid"]))]

    def close(self):
        self.ctx.close()


def background(n=40, seed=3):
    rng = np.random.default_rng(seed)
    return [r for i in range(n) for r in synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)]


def gap_pair(name, tid, pos, cigar, mate_cigar="100M", mate_off=250, mapq=60):
    """a proper pair whose first read carries `cigar` at 0-based pos"""
    return [synth.Rec(name, PAIRED_FWD, tid, pos, mapq, cigar, tid, pos + mate_off, mate_off + 100),
            synth.Rec(name, PAIRED_REV, tid, pos + mate_off, mapq, mate_cigar, tid, pos, -(mate_off + 100))]


# ---- 1. no events ----------------------------------------------------------------------------------------------------------------------
def test_no_events():
    c = Case([])
    got, counts, _ = c.check()
    assert len(got) == 0 and counts == dict(zip(gc.COUNTS, [0] * 8))
    c.close()
    c = Case(background(200) + [gc.read("clip%d" % k, 1, 5000 + 10 * k, "60M40S") for k in range(50)])
    got, counts, _ = c.check()
    assert len(got) == 0 and counts["records"] == counts["eligible"] == 450 and counts["events"] == counts["beyond"] == 0
    c.close()


# ---- 2. sizes ----------------------------------------------------------------------------------------------------------------------------
def sized_recs(e, n_loci):
    """e events: one record with three, the others with one, over n_loci starts 40 bases apart"""
    recs = background(20) + [gc.read("three", 2, 50_000, "20M25D20M25I20M30D20M")]
    return recs + [gc.read("z%d" % k, 0, 10_000 + 40 * (k % n_loci), "30M25D30M") for k in range(e - 3)]


def size_cases():
    p = capi.prims_info()
    assert p["SCAN_TILE"] == p["RS_TILE"]  # (one list serves both; were they to differ, both lists would be needed)
    t = p["RS_TILE"]
    return [t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 301, p["SCAN_ONE_MAX"] + 2]


@pytest.mark.parametrize("which", range(8))
def test_event_counts_across_boundaries(which):
    e = size_cases()[which]
    c = Case(sized_recs(e, 700 if e < 10_000 else 500))
    got, counts, _ = c.check()
    assert counts["events"] == e and int(got["n_rows"].sum()) == e and counts["exact"] == len(got) >= 500
    c.close()


@pytest.mark.parametrize("n", [3 * gc.TILE - 1, 3 * gc.TILE, 3 * gc.TILE + 1])
def test_record_counts_around_a_tile(n):
    """the last record of the table carries the event"""
    recs = [gc.read("b%d" % k, 0, 1000 + 10 * k, "100M") for k in range(n - 1)] + [gc.read("last", 3, 1_900_000, "30M25D30M")]
    c = Case(recs)
    got, counts, _ = c.check()
    assert counts["records"] == n and len(got) == 1 and int(got[0]["tid"]) == 3 and int(c.cols["tid"][-1]) == 3
    c.close()


# ---- 3. the walk -------------------------------------------------------------------------------------------------------------------------
LONG = "2M1I" * 98 + "1M1X" + "30D" + "15M"  # 200 operations, the event last but one
WALK = [("5H5S12M3I2P4=6X30N20D15M5S", [(0, 52, 20)]),            # every operation once
        ("30M20D30M", [(0, 30, 20)]), ("30M19D30M", []),           # min_len and one below
        ("10M20D30M", [(0, 10, 20)]), ("9M20D30M", []), ("30M20D10M", [(0, 30, 20)]), ("30M20D9M", []),  # the anchors
        ("5=5X20I10=", [(1, 10, 20)]),                             # an anchor of = and X alone
        ("5M3I5M40N20D10M", [(0, 50, 20)]),                        # an anchor interrupted by a short I and by an N
        ("20D30M", []), ("30M20I", []), ("5S20D30M", []), ("5H20I30M", []), ("30M20D5S", []),  # first, last, behind a clip
        ("30M25D25I30M", [(0, 30, 25), (1, 55, 25)]),              # adjacent
        (LONG, [(0, 98 * 2 + 2, 30)]),
        ("30M45N30M", [])]


def test_walk():
    recs = background()
    for k, (cigar, _) in enumerate(WALK):
        recs.append(gc.read("w%d" % k, 0, 10_000 * (k + 1), cigar))
    recs.append(gc.read("zero", 1, 0, "30M25D30M"))  # pos = 0
    c = Case(recs)
    got, counts, info = c.check()
    want = sorted((kind, 0, 10_000 * (k + 1) + off, ln) for k, (_, ev) in enumerate(WALK) for kind, off, ln in ev) + [(0, 1, 30, 25)]
    assert info["exact_keys"] == sorted(want) and counts["events"] == len(want) == len(got)
    assert LONG.count("M") + LONG.count("I") + LONG.count("X") + LONG.count("D") == 200
    # min_len and anchor move the bounds with them
    got, counts, _ = c.check(min_len=19)
    assert counts["events"] == len(want) + 1
    got, counts, _ = c.check(anchor=9)
    assert counts["events"] == len(want) + 2
    got, counts, _ = c.check(anchor=31, min_len=26)
    assert counts["events"] == 0
    c.close()


# ---- 4. dropped records, each alone --------------------------------------------------------------------------------------------------------
def dropped_read(kind):
    if kind.startswith("flag"):
        return gc.read("drop", 2, 500_000, "30M25D30M", flag=int(kind[4:], 16))
    if kind == "unmapped":
        return gc.read("drop", -1, 100, "30M25D30M")
    if kind == "mapq":
        return gc.read("drop", 2, 500_000, "30M25D30M", mapq=QUAL - 1)
    if kind == "mapq_at":
        return gc.read("drop", 2, 500_000, "30M25D30M", mapq=QUAL)
    if kind == "no_cigar":
        return gc.read("drop", 2, 500_000, "*")
    # a deletion of 25 whose right end is start + 26: 2 000 001 is beyond the contig's 2 000 000 bases, 2 000 000 is kept
    return gc.read("drop", 2, (2_000_001 if kind == "beyond" else 2_000_000) - 26 - 30, "30M25D30M")


@pytest.mark.parametrize("kind", ["flag4", "flag100", "flag200", "flag400", "flag800", "unmapped", "mapq", "mapq_at", "no_cigar", "beyond", "beyond_at"])
def test_dropped_records_each_alone(kind):
    c = Case(background() + [gc.read("good%d" % k, 0, 300_000, "30M25D30M") for k in range(3)] + [dropped_read(kind)])
    reasons = [r for r in c.reasons() if r not in (None, "short")]
    kept = kind.endswith("_at")
    assert reasons == ([] if kept else [kind[:4] if kind.startswith("flag") else kind]), reasons
    got, counts, _ = c.check()
    assert len(got) == (2 if kept else 1) and int(got[0]["n_reads"]) == 3 and counts["events"] == (4 if kept else 3)
    assert counts["beyond"] == (kind == "beyond") and counts["eligible"] == 80 + 3 + (kind in ("mapq_at", "no_cigar", "beyond", "beyond_at"))
    if kind == "mapq":
        got, counts, _ = c.check(mapq_min=QUAL - 1)
        assert len(got) == 2 and counts["events"] == 4
    c.close()


# ---- 5. linkage ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def linkage():
    """pairs of starts, and of lengths, 0 1 2 3 25 26 apart; chains of 70 starts 2 and 25 apart; a deletion and an insertion at one start;
    one start on two contigs; two starts 4 apart with equal length and a third length between them"""
    recs = background()
    for k, d in enumerate((0, 1, 2, 3, 25, 26)):
        recs += [gc.read("sa%d" % k, 0, 100_000 + 1000 * k, "30M40D30M"), gc.read("sb%d" % k, 0, 100_000 + 1000 * k + d, "30M40D30M")]
        recs += [gc.read("la%d" % k, 1, 100_000 + 1000 * k, "30M40D30M"), gc.read("lb%d" % k, 1, 100_000 + 1000 * k, "30M%dD30M" % (40 + d))]
    for k in range(70):
        recs += [gc.read("c2_%d" % k, 2, 100_000 + 2 * k, "30M50D30M"), gc.read("c25_%d" % k, 2, 300_000 + 25 * k, "30M50D30M")]
    recs += [gc.read("kd", 3, 100_000, "30M40D30M"), gc.read("ki", 3, 100_000, "30M40I30M")]
    recs += [gc.read("t%d" % t, t, 700_000, "30M33D30M") for t in range(4)]
    recs += [gc.read("br_a", 3, 400_000, "30M40D30M"), gc.read("br_b", 3, 400_004, "30M40D30M"), gc.read("br_c", 3, 400_002, "30M60D30M")]
    c = Case(recs)
    yield c
    c.close()


@pytest.mark.parametrize("tol", [0, 2, 25])
def test_linkage(linkage, tol):
    got, counts, _ = linkage.check(tol=tol)
    on = lambda tid, lo, hi: got[(got["tid"] == tid) & (got["start"] >= lo) & (got["start"] < hi)]  # noqa: E731
    # two events d apart are one call exactly when d <= tol; d == 0 is one exact event
    assert len(on(0, 100_000, 110_000)) == sum(1 if d <= tol else 2 for d in (0, 1, 2, 3, 25, 26))
    assert len(on(1, 100_000, 110_000)) == sum(1 if d <= tol else 2 for d in (0, 1, 2, 3, 25, 26))
    c2, c25 = on(2, 100_000, 200_000), on(2, 300_000, 400_000)
    assert len(c2) == (70 if tol < 2 else 1) and len(c25) == (70 if tol < 25 else 1)
    if tol >= 2:
        assert (int(c2[0]["n_exact"]), int(c2[0]["lo_start"]), int(c2[0]["hi_start"]), int(c2[0]["start"])) == (70, 100_030, 100_030 + 138, 100_030)
    kinds = got[(got["tid"] == 3) & (got["start"] == 100_030)]
    assert [int(k) for k in kinds["kind"]] == [0, 1] and len(got[got["start"] == 700_030]) == 4
    # the bridge: at tol 2 the starts 400 030 and 400 034 share a locus through 400 032, and their equal lengths make them one call
    bridge = on(3, 400_000, 401_000)
    assert len(bridge) == {0: 3, 2: 2, 25: 1}[tol]
    if tol == 2:
        assert (int(bridge[0]["len"]), int(bridge[0]["n_exact"]), int(bridge[0]["lo_start"]), int(bridge[0]["hi_start"])) == (40, 2, 400_030, 400_034)
    if tol == 25:  # (the lengths 40 and 60 chain too)
        assert (int(bridge[0]["n_exact"]), int(bridge[0]["lo_len"]), int(bridge[0]["hi_len"])) == (3, 40, 60)
    assert counts["calls"] >= counts["loci"]


# ---- 6. distinct reads ---------------------------------------------------------------------------------------------------------------------
def test_distinct_reads_tie_and_strands():
    recs = background()
    # both mates across one gap: one read, two rows
    recs += gap_pair("mates", 0, 200_000, "70M45D80M", mate_cigar="40M45D110M", mate_off=30)
    # one read name in two calls
    recs += [gc.read("twice", 1, 200_000, "30M40D30M"), gc.read("twice", 1, 900_000, "30M40D30M"), gc.read("other", 1, 900_000, "30M40D30M")]
    # ties: (start, len) = (300 031, 40) and (300 030, 41) with two reads each; (500 030, 41) and (500 030, 40) with two reads each
    recs += [gc.read("t%d" % k, 2, 300_001, "30M40D30M") for k in range(2)] + [gc.read("u%d" % k, 2, 300_000, "30M41D30M", flag=0x10) for k in range(2)]
    recs += [gc.read("v%d" % k, 2, 500_000, "30M41D30M") for k in range(2)] + [gc.read("w%d" % k, 2, 500_000, "30M40D30M") for k in range(2)]
    recs += [gc.read("x", 2, 500_001, "30M40D30M", flag=0x10, mapq=33)]
    c = Case(recs)
    got, counts, _ = c.check()
    by = {(int(r["tid"]), int(r["lo_start"])): r for r in got}
    m = by[(0, 200_070)]
    assert (int(m["n_reads"]), int(m["n_rows"]), int(m["n_fwd"]), int(m["n_rev"])) == (1, 2, 1, 1)
    assert int(by[(1, 200_030)]["n_reads"]) == 1 and int(by[(1, 900_030)]["n_reads"]) == 2
    t = by[(2, 300_030)]
    assert (int(t["start"]), int(t["len"]), int(t["top_reads"]), int(t["n_reads"]), int(t["n_fwd"]), int(t["n_rev"])) == (300_030, 41, 2, 4, 2, 2)
    t = by[(2, 500_030)]
    assert (int(t["start"]), int(t["len"]), int(t["top_reads"]), int(t["n_reads"]), int(t["n_exact"]), int(t["n_rev"]), int(t["mapq_sum"])) == (500_030, 40, 2, 5, 3, 1, 4 * 60 + 33)
    c.close()


# ---- 7. min_reads --------------------------------------------------------------------------------------------------------------------------
def test_min_reads_keeps_order_and_bytes():
    recs = background()
    sizes = [1, 4, 2, 3, 1, 5, 3]
    for k, n in enumerate(sizes):
        recs += [gc.read("mr%d_%d" % (k, j), 0, 200_000 + 1000 * k, "30M40D30M") for j in range(n)]
    c = Case(recs)
    all_rows, _, _ = c.check(min_reads=1)
    assert list(all_rows["n_reads"]) == sizes
    got, counts, _ = c.check(min_reads=3)
    assert list(got["n_reads"]) == [4, 3, 5, 3] and [int(p) for p in got["start"]] == [201_030, 203_030, 205_030, 206_030] and counts["calls"] == 7
    assert all(got[i].tobytes() == all_rows[j].tobytes() for i, j in enumerate((1, 3, 5, 6)))
    got, _, _ = c.check(min_reads=6)
    assert len(got) == 0
    c.close()


# ---- 8. table forms ------------------------------------------------------------------------------------------------------------------------
def gap_reads():
    """a 45-base deletion in 5 reads (two of them the mates of one pair), a 30-base insertion in 3, a deletion in 2 reads inside a gene"""
    recs = []
    for k in range(3):
        recs += gap_pair("del%d" % k, 1, 1_700_000 - 70 - 10 * k, "%dM45D%dM" % (70 + 10 * k, 80 - 10 * k))
    recs += gap_pair("delm", 1, 1_700_000 - 70, "70M45D80M", mate_cigar="40M45D110M", mate_off=30)
    for k in range(3):
        recs += gap_pair("ins%d" % k, 2, 200_000 - 50 - k, "%dM30I%dM" % (50 + k, 70 - k))
    for k in range(2):
        recs += gap_pair("two%d" % k, 0, 305_000 - 60, "60M25D90M")
    return recs


@pytest.fixture(scope="module")
def designed():
    ds = cc.designed_tumor(mix=False, n_proper=3000, loci=cc.LOCI[:1])
    ds.recs += gap_reads()
    ds.sort()
    cols = ds.to_soa()
    ref = capi.Context(CONTIGS)  # a context that never makes the call
    ref.upload(cols)
    ref.run(qual=QUAL, fast=True)
    fetched = {st: ref.fetch(st)[0].tobytes() for st in (abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)}
    ref.close()
    return dict(ds=ds, cols=cols, fetched=fetched)


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
            tid, beg, end = np.asarray([1, 0], np.int32), np.asarray([1_699_000, 0], np.int32), np.asarray([1_701_000, 5_000], np.int32)
            assert t.exclude_regions(tid, beg, end) > 8
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, tid, beg, end))
    for tol, min_reads in ((2, 1), (0, 3)):
        exp, counts = gc.both(cols, TLEN, QUAL, 20, 10, tol, min_reads)
        got = t.cigar_gaps(QUAL, 20, 10, tol, min_reads)
        assert_rows(got, exp)
        assert t.cigar_gap_counts() == counts
        assert t.cigar_gaps(QUAL, 20, 10, tol, min_reads).tobytes() == got.tobytes()  # two runs, the same bytes
    assert len(got) == (1 if form.startswith("exclude") else 2)
    if form.startswith("exclude"):
        assert not np.any((got["tid"] == 1) & (got["start"] == 1_700_000))  # the deletion lies in the excluded interval
    else:
        assert [(int(r["tid"]), int(r["start"]), int(r["len"]), int(r["kind"]), int(r["n_reads"]), int(r["n_rows"])) for r in got] == [(1, 1_700_000, 45, 0, 4, 5), (2, 200_000, 30, 1, 3, 3)]
    if form == "host":  # a later bk_run and bk_fetch return what they return without the call
        t.run(qual=QUAL, fast=True)
        for st, want in designed["fetched"].items():
            assert t.fetch(st)[0].tobytes() == want
        assert t.cigar_gaps(QUAL, 20, 10, 0, 3).tobytes() == got.tobytes()
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


# ---- 9. refusals and timing ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_timing(designed):
    import ctypes as C
    t = capi.Context(CONTIGS)
    with pytest.raises(capi.BreakIDError) as e:
        t.cigar_gaps()
    assert e.value.code == abi.BK_ERR_ARG and "holds no record table" in str(e.value)
    t.upload(designed["cols"])
    for kw, word in ((dict(mapq_min=-1), "mapq_min below 0"), (dict(min_len=0), "min_len must be at least 1"), (dict(min_len=1_000_001), "min_len above 1000000"),
                     (dict(anchor=0), "anchor must be at least 1"), (dict(tol=101), "tol above 100"), (dict(min_reads=0), "min_reads must be at least 1")):
        with pytest.raises(capi.BreakIDError) as e:
            t.cigar_gaps(**kw)
        assert e.value.code == abi.BK_ERR_ARG and word in str(e.value), kw
    L = capi.lib()
    out, n = C.c_void_p(), C.c_uint64()
    assert L.bk_cigar_gaps(t.h, QUAL, 20, 10, 2, 3, None, C.byref(n)) == abi.BK_ERR_ARG and b"null output" in L.bk_last_error(t.h)
    assert L.bk_cigar_gaps(t.h, QUAL, 20, 10, 2, 3, C.byref(out), None) == abi.BK_ERR_ARG and b"null output" in L.bk_last_error(t.h)
    assert L.bk_cigar_gap_counts(t.h, None) == abi.BK_ERR_ARG and b"null out" in L.bk_last_error(t.h)
    assert len(t.cigar_gaps(tol=100, min_reads=1)) == 3 and len(t.cigar_gaps(min_len=1_000_000)) == 0  # the largest values are accepted
    # timing: the scope and its byte model, recomputed from the counts
    t.timing_enable(True)
    got = t.cigar_gaps(QUAL, 20, 10, 2, 1)
    cnt = t.cigar_gap_counts()
    names = [name for name, *_ in t.timing()]
    touched = dict(zip(names, t.timing_touched()))
    bits = lambda v: int(v).bit_length()  # noqa: E731
    tiles = (cnt["records"] + 255) // 256
    records = 11 * cnt["records"] + 56 * tiles + 1792 * min(cnt["events"], tiles) + 48 * cnt["events"]
    p1 = 8 + 4 + (bits(2_000_000) + bits(3) + 1 + 7) // 8
    p2, p3 = (bits(cnt["loci"]) + 28 + 7) // 8, (bits(cnt["calls"]) + bits(cnt["events"]) + 7) // 8
    calls = cnt["events"] * (36 * (p1 + p2 + p3) + 400) + 144 * cnt["calls"] + 128 * len(got)
    assert cnt["events"] == 10 and len(got) == 3
    assert (touched["cigar_gaps_records"], touched["cigar_gaps_calls"], touched["cigar_gaps"]) == (records, calls, records + calls)
    t.timing_enable(False)
    t.close()
    # a sharded context is refused
    s = capi.Context(CONTIGS)
    s.upload(designed["cols"])
    s.shard_begin(0, QUAL)
    with pytest.raises(capi.BreakIDError) as e:
        s.cigar_gaps()
    assert e.value.code == abi.BK_ERR_ARG and "sharded" in str(e.value)
    s.close()


# ---- 10. the command line ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(designed):
    with tempfile.TemporaryDirectory() as tmp:
        ds = designed["ds"]
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        base = [BIN, "-i", bam, "-n", side["nib"], "-fast", "-all"]
        runs = {}
        for name, extra in (("a", ["-bedpe"]), ("b", ["-gaps", "-bedpe"]), ("c", ["-gaps", "-gapsupport", "2", "-gaptol", "0", "-mingap", "21", "-gapanchor", "11"])):
            r = subprocess.run(base + ["-o", os.path.join(tmp, name)] + extra, env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name] = r
        yield dict(tmp=tmp, cols=designed["cols"], runs=runs, base=base, env=env)


def expected_files(run, sample, **kw):
    cols = run["cols"]
    rows, counts = gc.both(cols, TLEN, QUAL, **kw)
    endpos = cc.rec_endpos(cols)
    lines, bed = ["\t".join(gc.COLUMNS)], []
    for i, r in enumerate(rows):
        tid, ends = int(r["tid"]), (int(r["start"]), gc.gap_end(r))
        depth = [cc.single_base_depth(cols, endpos, tid, p) for p in ends]
        gene = "GA_LR_x" if tid == 0 and 290_000 <= ends[0] <= 310_000 else "intergenic"
        lines.append("\t".join(gc.row_fields(i, r, NAMES, depth[0], depth[1], gene, gene)))
        bed.append(gc.bedpe_line(i, r, NAMES, sample))
    return "\n".join(lines) + "\n", "".join(l + "\n" for l in bed), gc.stdout_line(counts)


def test_cli_gap_files(cli):
    tmp = cli["tmp"]
    table, bed, stdout = expected_files(cli, "b", min_len=20, anchor=10, tol=2, min_reads=3)
    got = open(os.path.join(tmp, "b_gaps.txt")).read()
    assert got == table, (got, table)
    rows = [l.split("\t") for l in got.split("\n")[1:-1]]
    assert [f[:12] for f in rows] == [["gp0", "chr2", "1700000", "1700046", "deletion", "45", "4", "5", "1", "4", "4", "1"],
                                      ["gp1", "chr3", "200000", "200001", "insertion", "30", "3", "3", "1", "3", "3", "0"]]
    assert all(f[12] == "60.0" and f[17] == f[18] == "intergenic" and int(f[15]) > 0 for f in rows)
    assert stdout in cli["runs"]["b"].stdout.split("\n") and stdout.endswith("10 events, 0 beyond a contig's end, 3 exact, 3 calls, 2 written")
    assert open(os.path.join(tmp, "b_gaps.bedpe")).read() == bed and bed.count("\n") == 2
    assert "gaps:" not in cli["runs"]["a"].stdout and not os.path.exists(os.path.join(tmp, "a_gaps.txt"))
    # -gapsupport 2 adds the third call, with its gene; the other dials change nothing here; no -bedpe, no BEDPE file
    table, _, stdout = expected_files(cli, "c", min_len=21, anchor=11, tol=0, min_reads=2)
    got = open(os.path.join(tmp, "c_gaps.txt")).read()
    assert got == table and got.count("\n") == 4 and "gp0\tchr1\t305000\t305026\tdeletion\t25\t2\t2\t1\t2\t2\t0\t60.0\t305000-305000\t25-25\t" in got
    assert "\tGA_LR_x\tGA_LR_x\n" in got and stdout in cli["runs"]["c"].stdout.split("\n")
    assert not os.path.exists(os.path.join(tmp, "c_gaps.bedpe"))


def test_cli_every_other_file_is_unchanged(cli):
    tmp = cli["tmp"]
    files = sorted(f[2:] for f in os.listdir(tmp) if f.startswith("a_"))
    assert "fusion.txt" in files and "fusion_all.txt" in files and "fusion_all.bedpe" in files and "params.txt" in files
    assert sorted(f[2:] for f in os.listdir(tmp) if f.startswith("b_")) == sorted(files + ["gaps.txt", "gaps.bedpe"])
    a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    for f in files:
        ta, tb = open(os.path.join(tmp, "a_" + f), "rb").read(), open(os.path.join(tmp, "b_" + f), "rb").read()
        if f == "params.txt":
            assert tb.decode() == ta.decode().replace("out_file\t" + a, "out_file\t" + b) + "gap_min_length\t20\ngap_anchor\t10\ngap_tol\t2\ngap_min_support\t3\n"
        elif f == "performance.txt":  # (the last four columns are times)
            assert [l.split("\t")[:5] for l in ta.decode().split("\n")] == [l.split("\t")[:5] for l in tb.decode().split("\n")]
        elif f.endswith(".bedpe"):  # (the name column is the prefix's base name)
            assert ta.replace(b"\ta\t", b"\tb\t") == tb and ta.count(b"\ta\t") == ta.count(b"\n") > 0, f
        else:
            assert ta.replace(a.encode(), b.encode()) == tb, f
    quiet = lambda out: [l for l in out.split("\n") if "costs time" not in l and not l.startswith("gaps:")]  # noqa: E731
    assert quiet(cli["runs"]["a"].stdout) == quiet(cli["runs"]["b"].stdout.replace(b, a))
    assert open(os.path.join(tmp, "c_params.txt")).read().endswith("gap_min_length\t21\ngap_anchor\t11\ngap_tol\t0\ngap_min_support\t2\n")


def test_cli_gap_bedpe_is_a_known_panel(cli):
    tmp = cli["tmp"]
    panel = os.path.join(tmp, "b_gaps.bedpe")
    r = subprocess.run(cli["base"] + ["-o", os.path.join(tmp, "d"), "-known", panel, "-knownslop", "0"], env=cli["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "known: 2 entries, 0 on contigs the input lacks, 0 calls with a hit\n" in r.stdout and "Warning" not in r.stderr


def test_cli_refusals(cli):
    tmp = cli["tmp"]
    base = cli["base"] + ["-o", os.path.join(tmp, "z")]
    need = "-mingap, -gapanchor, -gaptol and -gapsupport need -gaps."
    for args, word in ((["-mingap", "5"], need), (["-gapanchor", "5"], need), (["-gaptol", "1"], need), (["-gapsupport", "5"], need),
                       (["-gaps", "-gpus", "2"], "-gaps cannot be combined with -gpus."),
                       (["-gaps", "-mingap", "0"], "-mingap must be a number from 1 to 1000000."), (["-gaps", "-mingap", "1000001"], "-mingap must be a number from 1 to 1000000."),
                       (["-gaps", "-gapanchor", "0"], "-gapanchor must be a number from 1 to 2147483647."),
                       (["-gaps", "-gaptol", "101"], "-gaptol must be a number from 0 to 100."), (["-gaps", "-gaptol", "-1"], "-gaptol must be a number from 0 to 100."),
                       (["-gaps", "-gapsupport", "0"], "-gapsupport must be a number from 1 to 1000000."),
                       (["-gaps", "-gapsupport", "1000001"], "-gapsupport must be a number from 1 to 1000000.")):
        r = subprocess.run(base + args, env=cli["env"], capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-500:])
    assert not any(f.startswith("z_") for f in os.listdir(tmp))

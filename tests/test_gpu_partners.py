"""Partner loci (`bk_locus_partners`, `-partners`): the kernels against the definition in tests/partnercases.py byte for byte, the
expectations taken from the fetched BK_STAGE_SCAN table.  Windows that hold exactly 0, 1, 63 ... 257 ends, and as many elsewhere ends (a
ballot, a chunk, four ballots and one more); window and partner bounds on an end and one off it; max_gap at a real gap, one below it,
0 and 0xFFFFFFFF; ties for the top run; site lists of 0 to 257 sites with empty sites between full ones; a seeded table whose rows span
many radix tiles; every table form; every refusal; timing; and the command line's files against the definition."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import partnercases as pc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = [("c0", 2_000_000), ("c1", 2_000_000), ("c2", 2_000_000)]
COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 256, 257]
DENSE = 330  # pairs of the dense locus


def assert_rows(got, exp):
    assert got.dtype == abi.LOCUS_PARTNERS and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def joined_context(ds):
    """a context after bk_discordant_pairs and nothing later: (context, w)"""
    t = capi.Context(ds.contigs)
    t.upload(ds.to_soa())
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    return t, w


def designed_sample():
    """background, and a dense locus on c0 from 500 000 on: DENSE pairs three bases apart.  A third of the mates go to one partner locus
    on c1, a third to 40 small loci on c2 (some mates on equal positions), a third far along c0 itself, in stacks of equal positions"""
    rng = np.random.default_rng(8)
    ds = synth.Dataset(list(CONTIGS))
    for i in range(3000):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, 3)), 1000, 400_000, 100, 350, 40)
    for k in range(DENSE):
        own = 500_000 + 3 * k
        if k % 3 == 0:
            mate = (1, 800_000 + 2 * k)
        elif k % 3 == 1:
            mate = (2, 100_000 + 5000 * (k % 40) + k // 80)
        else:
            mate = (0, 1_500_000 + 700 * (k % 7) + (k % 2))
        ds.recs += synth._discordant_pair("dense_%d" % k, 0, own, mate[0], mate[1], 100)
    ds.sort()
    return ds


@pytest.fixture(scope="module")
def dense():
    t, w = joined_context(designed_sample())
    scan = t.fetch(abi.STAGE_SCAN)[0]
    tid, pos, mtid, mpos = pc.ends_of(scan)
    at = np.flatnonzero((tid == 0) & (pos >= 400_000) & (pos < 1_000_000))
    own = np.sort(pos[at])
    assert len(scan) == DENSE and len(own) == DENSE and len(np.unique(own)) == DENSE  # the ends of the locus, each on a position of its own
    yield {"ctx": t, "w": w, "scan": scan, "own": own}
    t.close()


def check(run, sites, gap, brute=True):
    """the kernels against the run-based statement, and on small lists against the brute-force one too"""
    exp = pc.expected_runs(run["scan"], sites, gap, len(CONTIGS))
    if brute:
        assert exp.tobytes() == pc.expected(run["scan"], sites, gap, len(CONTIGS)).tobytes()
    got = run["ctx"].locus_partners(sites, gap)
    assert_rows(got, exp)
    return got


# ---- 1. windows by the number of ends they hold ------------------------------------------------------------------------------------------
def window(own, first, m):
    """the window that holds exactly ends first .. first + m - 1 of the locus (m = 0: the gap in front of `first`)"""
    return (int(own[first]) + 1, int(own[first]) + 1) if m == 0 else (int(own[first]), int(own[first + m - 1]))


@pytest.mark.parametrize("gap", [0, 4, 5000])
def test_windows_by_their_number_of_ends(dense, gap):
    own = dense["own"]
    rows = []
    for m in COUNTS:
        for first in (0, 7, DENSE - m - 1):
            a, b = window(own, first, m)
            rows.append((0, a, b, -1, 1, 0))                    # every end goes elsewhere
            rows.append((0, a, b, 1, 1, pc.U32))                # the third on c1 goes to the partner
            rows.append((0, a, b, 0, 1, pc.U32))                # the partner is the site's own contig
            rows.append((0, a, b, 2, 100_000, 160_000))         # part of the loci on c2
    got = check(dense, pc.as_sites(rows), gap)
    ends = got["ends"].reshape(len(COUNTS), -1)
    assert all(np.all(ends[k] == m) for k, m in enumerate(COUNTS))
    elsewhere = set((got["ends"] - got["to_partner"]).tolist())
    assert set(COUNTS) <= elsewhere and set(got["to_partner"].tolist()) >= {0, 1, 21, 22, 43, 86}
    # the elsewhere counts around the edges of a ballot, a chunk and four ballots, with a partner that takes some ends away
    rows = []
    for first in range(0, 12):
        for m in (94, 95, 96, 97, 190, 191, 192, 193, 194, 300):
            a, b = window(own, first, m)
            rows.append((0, a, b, 1, 1, pc.U32))
    got = check(dense, pc.as_sites(rows), gap)
    assert {63, 64, 65, 127, 128, 129, 200} <= set((got["ends"] - got["to_partner"]).tolist())


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------------------
def test_bounds_on_an_end_and_one_off(dense):
    own, scan = dense["own"], dense["scan"]
    a, b = int(own[10]), int(own[50])
    tid, pos, mtid, mpos = pc.ends_of(scan)
    inside = (tid == 0) & (pos >= a) & (pos <= b) & (mtid == 1)
    ma, mb = int(mpos[inside].min()), int(mpos[inside].max())
    rows = []
    for da, db in ((0, 0), (1, 0), (0, -1), (1, -1), (-1, 1)):
        rows.append((0, a + da, b + db, 1, ma, mb))
        rows.append((0, a, b, 1, ma + da, mb + db))
        rows.append((1, ma + da, mb + db, 0, a, b))  # from the other side
    rows += [(0, a, a, 1, ma, mb), (0, a + 1, a + 2, 1, ma, mb), (0, a, b, 1, ma, ma), (0, a, b, 1, mb + 1, mb + 1), (0, 1, pc.U32, 1, 1, pc.U32), (0, 0, 0, 1, 0, 0),
             (0, pc.U32, pc.U32, 1, pc.U32, pc.U32)]
    got = check(dense, pc.as_sites(rows), 100)
    n_to = int(inside.sum())
    assert [int(got[k]["ends"]) for k in (0, 3, 6, 9, 12)] == [41, 40, 40, 39, 41]
    assert [int(got[k]["to_partner"]) for k in (1, 4, 7, 10, 13)] == [n_to, n_to - 1, n_to - 1, n_to - 2, n_to]
    assert [int(got[15 + k]["ends"]) for k in range(7)] == [1, 0, 41, 41, DENSE + (DENSE + 2) // 3, 0, 0]
    assert int(got[17]["to_partner"]) == 1 and int(got[18]["to_partner"]) == 0


def real_gap(dense):
    """a site whose elsewhere mates include two neighbours on one contig a real gap g > 1 apart: (site row, g)"""
    own, scan = dense["own"], dense["scan"]
    site = (0, int(own[0]), int(own[200]), 1, 1, pc.U32)
    _, _, mates = pc.elsewhere_of(scan, pc.as_sites([site])[0], len(CONTIGS))
    gaps = sorted({b[1] - a[1] for a, b in zip(mates, mates[1:]) if a[0] == b[0] and b[1] - a[1] > 1})
    return site, gaps


def test_max_gap_at_a_real_gap(dense):
    site, gaps = real_gap(dense)
    assert len(gaps) >= 3
    loci = []
    for g in gaps[:3] + gaps[-1:]:
        at_g, below, zero = (check(dense, pc.as_sites([site]), x)[0] for x in (g, g - 1, 0))
        assert int(at_g["loci"]) < int(below["loci"]) <= int(zero["loci"])  # the gap joins at g and splits at g - 1
        loci.append(int(at_g["loci"]))
    # no wrap: 0xFFFFFFFF joins every contig's mates into one run, and a gap of 2^32 - 2 behaves like it here
    top = check(dense, pc.as_sites([site]), pc.U32)[0]
    assert int(top["loci"]) == 2 and int(top["top_n"]) == 67 and check(dense, pc.as_sites([site]), pc.U32 - 1)[0].tobytes() == top.tobytes()
    # equal mate positions: at gap 0 the stacks on c0 are the runs of more than one mate
    zero = check(dense, pc.as_sites([site]), 0)[0]
    assert int(zero["top_n"]) >= 2 and int(zero["top_tid"]) == 0 and int(zero["top_beg"]) == int(zero["top_end"])


def ties(scan, site, gap):
    """the contigs of the runs that share the largest length, in sorted order"""
    _, _, mates = pc.elsewhere_of(scan, pc.as_sites([site])[0], len(CONTIGS))
    runs = pc.runs_of(mates, gap)
    longest = max(l for _, l in runs)
    return [mates[f][0] for f, l in runs if l == longest]


def test_ties_for_the_top_run(dense):
    own, scan = dense["own"], dense["scan"]
    # one contig: of the first twelve ends that go far along c0, ten land in stacks of two
    one = (0, int(own[0]), int(own[35]), 1, 1, pc.U32)
    assert set(ties(scan, one, 100)) == {0} and len(ties(scan, one, 100)) >= 3
    # two contigs: without a partner the six ends' mates stand alone on c0, c1 and c2
    two = (0, int(own[0]), int(own[5]), -1, 1, 0)
    assert len(set(ties(scan, two, 0))) == 3
    got = check(dense, pc.as_sites([one, two, one]), 100)
    assert int(got[0]["top_n"]) == 2 and int(got[0]["top_tid"]) == 0 and int(got[0]["top_end"]) - int(got[0]["top_beg"]) == 1 and got[0].tobytes() == got[2].tobytes()
    got = check(dense, pc.as_sites([two]), 0)
    assert int(got[0]["top_n"]) == 1 and int(got[0]["top_tid"]) == 0 and int(got[0]["loci"]) == 6


# ---- 3. site lists --------------------------------------------------------------------------------------------------------------------------
def mixed_sites(dense, n, seed):
    """n sites over the dense locus: full ones, empty ones between them, zero rows, and the same site more than once"""
    rng = np.random.default_rng(seed)
    own = dense["own"]
    rows = []
    for k in range(n):
        kind = int(rng.integers(0, 8))
        first = int(rng.integers(0, DENSE - 1))
        m = int(rng.integers(1, DENSE - first))
        a, b = window(own, first, m)
        if kind == 0:
            rows.append((0, int(own[first]) + 1, int(own[first]) + 2, 1, 1, pc.U32))  # between two ends
        elif kind == 1:
            rows.append([(-1, a, b, 1, 1, pc.U32), (3, a, b, 1, 1, pc.U32), (0, b, a - 1, 1, 1, pc.U32), (0x7FFFFFFF, a, b, 1, 1, pc.U32)][k % 4])  # the zero rows
        elif kind == 2 and rows:
            rows.append(rows[int(rng.integers(0, len(rows)))])
        elif kind == 3:
            rows.append((0, a, b, [-1, 3, 0x7FFFFFFF, 1][k % 4], 900_000, 800_000 + (k % 2) * 200_000))  # no partner, or an empty one
        else:
            rows.append((0, a, b, int(rng.integers(0, 3)), int(rng.integers(1, 1_600_000)), int(rng.integers(1, 2_000_000))))
    return pc.as_sites(rows)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 257])
def test_site_lists(dense, n):
    sites = mixed_sites(dense, n, 100 + n)
    first = check(dense, sites, 3000)
    if n == 0:
        return
    if n == 257:
        empty = first["ends"] == first["to_partner"]
        assert int(empty.sum()) >= 30 and int((~empty).sum()) >= 100 and int((first["ends"] == 0).sum()) >= 30
        assert np.any(empty[1:-1] & ~empty[:-2] & ~empty[2:])  # an empty segment between two full ones
    # another call in between, then the same bytes again; a permuted list gives the permuted rows
    dense["ctx"].locus_partners(pc.as_sites([(0, 1, pc.U32, -1, 1, 0)]), 1)
    assert dense["ctx"].locus_partners(sites, 3000).tobytes() == first.tobytes()
    order = np.random.default_rng(n).permutation(n)
    assert dense["ctx"].locus_partners(sites[order], 3000).tobytes() == first[order].tobytes()
    twice = np.concatenate([sites, sites])
    both = dense["ctx"].locus_partners(twice, 3000)
    assert both[:n].tobytes() == first.tobytes() == both[n:].tobytes()


# ---- 4. a seeded table ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    """30 000 pairs drawn on 3 contigs of 50 000 bases, a fifth of them around twelve hot spots"""
    rng = np.random.default_rng(77)
    contigs = [("s0", 50_000), ("s1", 50_000), ("s2", 50_000)]
    ds = synth.Dataset(list(contigs))
    for i in range(2000):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, 3)), 100, 49_000, 100, 350, 40)
    hot = [(int(rng.integers(0, 3)), int(rng.integers(2000, 47_000))) for _ in range(12)]
    for k in range(30_000):
        ends = []
        for _ in range(2):
            if rng.random() < 0.2:
                t, p = hot[int(rng.integers(0, 12))]
                ends.append((t, p + int(rng.integers(-200, 201))))
            else:
                ends.append((int(rng.integers(0, 3)), int(rng.integers(1, 49_800))))
        ds.recs += synth._discordant_pair("r%d" % k, ends[0][0], ends[0][1], ends[1][0], ends[1][1], 100)
    ds.sort()
    t, w = joined_context(ds)
    scan = t.fetch(abi.STAGE_SCAN)[0]
    assert 20_000 <= len(scan) <= 50_000
    sites = []
    for _ in range(3000):
        c, wd = int(rng.integers(1, 50_000)), int(rng.choice([0, 20, 100, 300, 1000]))
        mc, mw = int(rng.integers(1, 50_000)), int(rng.choice([0, 100, 1000, 50_000]))
        sites.append((int(rng.integers(-1, 4)), max(1, c - wd), c + wd, int(rng.integers(-1, 4)), max(1, mc - mw), mc + mw))
    yield {"ctx": t, "scan": scan, "sites": pc.as_sites(sites), "hot": hot}
    t.close()


@pytest.mark.parametrize("gap", [0, 25, pc.U32])
def test_seeded_table(seeded, gap):
    sites = seeded["sites"]
    exp, n_rows = pc.expected_runs(seeded["scan"], sites, gap, 3, with_rows=True)
    assert n_rows > 100_000 and int(exp["ends"].max()) > 500 and int((exp["ends"] == 0).sum()) > 300  # many radix tiles; windows of hundreds of ends
    assert int((exp["to_partner"] > 0).sum()) > 300 and int(exp["loci"].max()) > (100 if gap == 0 else 2)
    assert_rows(seeded["ctx"].locus_partners(sites, gap), exp)


# ---- 5. forms and side effects -----------------------------------------------------------------------------------------------------------------
G1_SITES = [(0, 49_000, 51_000, 1, 79_000, 81_000), (1, 79_000, 81_000, 0, 49_000, 51_000), (0, 1, 200_000, -1, 1, 0), (5, 1, 200_000, 0, 1, 200_000)]


@pytest.mark.parametrize("where", ["host", "device"])
def test_table_forms_and_every_stage_unchanged(where):
    """host upload and BK_MEM_DEVICE; after bk_discordant_pairs only and after the whole run; every stage's bytes before and after"""
    ds = synth.make_g1()
    cols = ds.to_soa()
    sites = pc.as_sites(G1_SITES)
    t, keep = cc.make_ctx(ds.contigs, cols, where)
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    scan = t.fetch(abi.STAGE_SCAN)[0]
    exp = pc.expected(scan, sites, int(w), 24)
    assert exp.tobytes() == pc.expected_runs(scan, sites, int(w), 24).tobytes()
    assert (int(exp[0]["ends"]), int(exp[0]["to_partner"]), int(exp[0]["loci"])) == (12, 12, 0) and int(exp[2]["ends"]) == 12 == int(exp[2]["top_n"])
    early = t.locus_partners(sites, int(w))
    assert_rows(early, exp)
    assert t.run(qual=QUAL, fast=True)[1] == 1
    stages = (abi.STAGE_SCAN, abi.STAGE_ISO, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)
    before = [t.fetch(st)[0].tobytes() for st in stages]
    assert before[0] == scan.tobytes()
    assert t.locus_partners(sites, int(w)).tobytes() == early.tobytes()
    assert [t.fetch(st)[0].tobytes() for st in stages] == before
    # the call's own windows, by the shared rule: all twelve pairs of the locus, each end with its mate at the partner (the call itself
    # reports the eight that clustering kept)
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    own = t.locus_partners(capi.call_partner_sites(cl[0], w), int(w))
    assert [(int(r["ends"]), int(r["to_partner"]), int(r["top_n"])) for r in own] == [(12, 12, 0)] * 2 and int(cl[0]["n_drp"]) == 8
    t.close()
    u = capi.Context(ds.contigs)  # a context that never made the call
    u.upload(cols)
    u.run(qual=QUAL, fast=True)
    assert [u.fetch(st)[0].tobytes() for st in stages] == before
    u.close()
    del keep


def test_a_context_without_pairs():
    t, w = joined_context(cc.quiet_tumor())
    assert len(t.fetch(abi.STAGE_SCAN)[0]) == 0
    sites = pc.as_sites([(0, 1, 2_000_000, 1, 1, 2_000_000), (-1, 1, 5, 0, 1, 5)])
    got = t.locus_partners(sites, 1000)
    assert_rows(got, pc.expected(pc.as_pairs([]), sites, 1000, 4))
    assert got[0].tobytes() == pc.none_row().tobytes() == got[1].tobytes()
    assert len(t.locus_partners(sites[:0], 1000)) == 0
    t.close()


def test_partners_are_timed(dense):
    t, scan, own = dense["ctx"], dense["scan"], dense["own"]
    sites = pc.as_sites([(0, int(own[0]), int(own[99]), 1, 1, pc.U32), (0, int(own[100]), int(own[299]), -1, 1, 0), (1, 1, 5, 0, 1, 5)])
    exp, n_rows = pc.expected_runs(scan, sites, 10, 3, with_rows=True)
    assert n_rows == 100 - 34 + 200
    t.timing_enable(True)
    got = t.locus_partners(sites, 10)
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    t.timing_enable(False)
    assert_rows(got, exp)
    assert names[-3:] == ["locus_partners", "locus_partners_index", "locus_partners_sites"]
    model = pc.touched(len(scan), 3, 3, n_rows)
    assert model == 56 * DENSE + 24 * DENSE + 3 * 64 + 12 * n_rows * 6
    assert touched["locus_partners"] == model == tm["locus_partners"][1]
    assert touched["locus_partners_index"] == pc.touched_index(len(scan)) and touched["locus_partners_sites"] == pc.touched_sites(3, 3, n_rows)
    assert tm["locus_partners"][0] >= tm["locus_partners_index"][0] > 0 and tm["locus_partners"][0] >= tm["locus_partners_sites"][0] > 0


def raw_call(ctx, sites, n, gap, out=True):
    C = capi.C
    res = C.c_void_p()
    rc = ctx.L.bk_locus_partners(ctx.h, sites.ctypes.data if sites is not None else None, n, gap, C.byref(res) if out else None)
    return rc, (ctx.L.bk_last_error(ctx.h) or b"").decode()


def test_argument_refusals(dense):
    ctx = dense["ctx"]
    good = pc.as_sites([(0, 500_000, 500_100, 1, 1, pc.U32), (0, 500_000, 500_400, -1, 1, 0)])
    want = pc.expected(dense["scan"], good, 50, 3)
    rc, msg = raw_call(ctx, good, 2, 50, out=False)
    assert rc == abi.BK_ERR_ARG and "null out" in msg
    rc, msg = raw_call(ctx, None, 2, 50)
    assert rc == abi.BK_ERR_ARG and "null sites" in msg
    assert raw_call(ctx, None, 0, 50)[0] == abi.BK_OK
    for k in (0, 1):
        bad = good.copy()
        bad[1]["reserved"][k] = 1
        rc, msg = raw_call(ctx, bad, 2, 50)
        assert rc == abi.BK_ERR_ARG and "site 1 has a non-zero reserved field" in msg
    rc, msg = raw_call(ctx, good, (1 << 30) + 1, 50)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg
    # wrong call order: records, statistics, but no pairs yet
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s.isize_stats()
    with pytest.raises(capi.BreakIDError, match="call bk_discordant_pairs first") as e:
        s.locus_partners(good, 50)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.locus_partners(good, 50)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.locus_partners(good, 50), want)  # the context still works


# ---- 6. command line ---------------------------------------------------------------------------------------------------------------------------
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=Integer," % k for k in ("PTN", "PTP", "PTL"))


def promiscuous_tumor():
    """the designed tumour, and at its first locus forty more ends on chr1 whose mates scatter over chr3 and chr4"""
    ds = cc.designed_tumor()
    rng = np.random.default_rng(31)
    for j in range(40):
        ds.recs += synth._discordant_pair("spray_%d" % j, 0, 300_000 - int(rng.integers(100, 400)), 2 + j % 2, 100_000 + 40_000 * (j % 5) + int(rng.integers(0, 300)), 100)
    ds.sort()
    return ds


@pytest.fixture(scope="module")
def cli_run():
    with tempfile.TemporaryDirectory() as tmp:
        ds, nor = promiscuous_tumor(), cc.designed_normal()
        bam, nbam = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        cc.write_indexed(ds, bam)
        nor.write_bam(nbam, aligned=True)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        t = capi.Context(ds.contigs)
        t.upload(ds.to_soa())
        w, _ = t.run(qual=QUAL, fast=True)
        cl, scan = t.fetch(abi.STAGE_CLUSTERS)[0], t.fetch(abi.STAGE_SCAN)[0]
        n = capi.Context(nor.contigs)
        n.upload(nor.to_soa())
        n.isize_stats()
        n.discordant_pairs(QUAL, w)
        nscan = n.fetch(abi.STAGE_SCAN)[0]
        # the kernels on both tables, at the sites and the gap the command line uses
        sites = np.concatenate([pc.call_sites(c, w) for c in cl])
        for ctx, table in ((t, scan), (n, nscan)):
            assert_rows(ctx.locus_partners(sites, int(w)), pc.expected_runs(table, sites, int(w), 4))
        t.close()
        n.close()
        yield {"tmp": tmp, "bam": bam, "nbam": nbam, "nib": side["nib"], "env": env, "cl": cl, "w": w, "scan": scan, "nscan": nscan}


@pytest.mark.parametrize("variant", ["plain", "all_vcf", "normal"])
def test_cli_partners(cli_run, variant):
    run = cli_run
    tmp, cl, w = run["tmp"], run["cl"], run["w"]
    extra = {"plain": [], "all_vcf": ["-all", "-vcf"], "normal": ["-normal", run["nbam"]]}[variant]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-partners"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_partners.txt", "_fusion_partners.txt"] if "-all" in extra else ["_fusion_partners.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    for suffix in fa:
        if suffix not in {"_params.txt", "_performance.txt", "_fusion.vcf"}:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "partners\n", (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's columns on the sample's pairs and the normal's
    with_normal = variant == "normal"
    columns = pc.PARTNER_NAMES + (["Normal_" + c for c in pc.PARTNER_NAMES] if with_normal else [])
    rows_of_call, held = {}, {}
    for twin in twins:
        plain = twin.replace("_partners", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(columns)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) >= 4
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            sites = pc.call_sites(cl[i], w)
            two = pc.expected(run["scan"], sites, int(w), 4)
            exp = pc.call_fields(two, cc.NAMES)
            if with_normal:
                exp = exp + pc.call_fields(pc.expected(run["nscan"], sites, int(w), 4), cc.NAMES)
            assert line == s + "\t" + "\t".join(exp), (line, exp)
            rows_of_call[i] = two
        held[twin] = calls
    # the designed locus: its own pairs go to the partner, the forty sprayed ends to ten loci, the largest four strong
    (first, a_is_1), = cc.rows_of(cl, 0, 300_000, 1, 700_000)
    side = rows_of_call[first][0 if a_is_1 else 1]
    assert (int(side["ends"]), int(side["to_partner"]), int(side["loci"]), int(side["top_n"])) == (54, 14, 10, 4)
    if with_normal:
        line = [l for l in open(b + "_fusion_partners.txt").read().split("\n") if l.split("\t")[1:3] in (["chr1:300000", "chr2:700000"], ["chr2:700000", "chr1:300000"])]
        assert len(line) == 1 and line[0].split("\t")[-11:] == ["6", "6", "0", ".", "0", "6", "6", "0", ".", "0", "1.000"]
    # 3. stdout: one more line
    written = held[twins[0]]
    ends = sum(int(rows_of_call[i]["ends"].sum()) for i in written)
    to = sum(int(rows_of_call[i]["to_partner"].sum()) for i in written)
    said = "partners: %d calls, %d ends in their windows, %d of them to the partner" % (len(written), ends, to)
    keep = lambda text: [l for l in text.split("\n") if "costs time" not in l]
    assert [l for l in keep(r.stdout) if l != said] == keep(out_a.replace(a, b)) and r.stdout.count(said + "\n") == 1
    # 4. the VCF: PTN / PTP / PTL of the breakend's own side last in INFO, their header lines, nothing else touched
    if "-vcf" not in extra:
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    head_b = [l for l in vb if l.startswith("#")]
    assert [l for l in va if l.startswith("#")] == [l for l in head_b if not l.startswith(INFO_LINES)]
    at = [k for k, l in enumerate(head_b) if l.startswith(INFO_LINES)]
    assert at == [at[0], at[0] + 1, at[0] + 2] and not head_b[at[2] + 1].startswith("##INFO")  # behind every other key of the calls
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 2 * len(written)
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + pc.info_fields(rows_of_call[i][s]), lb


def test_cli_partners_refusals_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-partners", "-gpus", "2"], "-partners cannot be combined with -gpus."), (["-partners", "-gpus", "1", "-vcf"], "-vcf cannot be combined with -gpus."),
                           (["-partners", "-linkdist", "5"], "-linkdist needs -link.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-partners", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_partners.txt", "_fusion_all_partners.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(pc.PARTNER_NAMES) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\npartners\n")
        assert "partners: 0 calls, 0 ends in their windows, 0 of them to the partner\n" in r.stdout

"""Linked calls (`bk_link_calls`, `-link`): the kernels against the definition in tests/linkcases.py byte for byte.  Every combination of
sides and both mappings at the distance D and one beyond it; positions at both ends of the 32-bit range; more calls in one window than a
step of the neighbour loop takes; events as paths, a ring and joined paths in shuffled order; a seeded table that spans several sort
tiles; a permuted list and a second run; every refusal; timing; and the command line's files against the definition."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import linkcases as lc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = [("c0", 5_000_000), ("c1", 5_000_000), ("c2", 1_000_000)]


@pytest.fixture(scope="module")
def ctx():
    """a context that holds no records: bk_link_calls needs none"""
    t = capi.Context(CONTIGS)
    yield t
    t.close()


def assert_rows(got, exp):
    assert got.dtype == abi.CALL_LINK and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


# ---- 1. relations at the edges ---------------------------------------------------------------------------------------------------------
def edge_sites(D):
    """pairs of sites, each pair 20 (D + 1) bases from the next: all 16 combinations of the four rights, the partner straight or
    crossed, its two breakpoints D or D + 1 from the first site's on either side; then the special pairs"""
    rows, step = [], 20 * (D + 1)
    deltas = [(D, D), (D + 1, D), (D, -(D + 1)), (-(D + 1), D + 1), (-D, -D)]
    base = step
    for rights in range(16):
        ri0, ri1, rj0, rj1 = rights & 1, rights >> 1 & 1, rights >> 2 & 1, rights >> 3 & 1
        for crossed in (0, 1):
            for d0, d1 in deltas:
                rows.append((0, base, ri0, 1, base + 7, ri1))
                rows.append((1, base + 7 + d1, rj0, 0, base + d0, rj1) if crossed else (0, base + d0, rj0, 1, base + 7 + d1, rj1))
                base += step
    special = [
        [(2, base, 0, 3, base, 1), (4, base, 1, 5, base, 0)],                          # the same positions on other contigs: nothing
        [(2, base + step, 0, -1, base + step, 1), (2, base + step, 1, -1, base + step, 0)],  # a side without a contig is near nothing: adjacent
        [(-1, 5, 0, -1, 5, 1), (-1, 5, 0, -1, 5, 1)],                                  # no contig at all
        [(6, base, 0, 7, base, 1), (6, base, 0, 7, base, 0)],                          # both pairs near, one equal and one different: adjacent
        [(6, base + step, 0, 7, base + step, 1), (6, base + step, 1, 7, base + step, 1)],
        # two small events on one spot: both mappings hold.  Both opposite: the smaller sum wins (crossed here), then straight on a tie
        [(8, base, 0, 8, base + D, 0), (8, base + D, 1, 8, base, 1)],
        [(8, base + step, 1, 8, base + step, 1), (8, base + step + D, 0, 8, base + step + D, 0)],
        # straight same and crossed opposite: a duplicate, whatever the crossed mapping says
        [(9, base, 0, 9, base + D, 1), (9, base, 0, 9, base + D, 1)],
        # a site whose own sides are near each other is alone; beside a second one it is that one's partner only
        [(10, base, 0, 10, base + D, 1)],
        [(10, base + step, 0, 10, base + step + D, 1), (10, base + step + 2 * D, 1, 11, 9, 0)],
    ]
    for group in special:
        rows += group
    return lc.as_sites(rows)


@pytest.mark.parametrize("D", [0, 100, 1000])
def test_relations_at_the_edges(ctx, D):
    sites = edge_sites(D)
    exp = lc.expected(sites, D)
    # the cases are what they are meant to be: the first 320 rows are pairs that see nobody else, and every relation is among them
    pairs = exp[:320]
    assert np.all(pairs["n_dup"] + pairs["n_recip"] + pairs["n_adj"] <= 1) and np.all(pairs["event_size"] <= 2)
    if D:
        assert min(int(pairs[f].sum()) for f in ("n_dup", "n_recip", "n_adj")) >= 16 and int((pairs["event_size"] == 1).sum()) >= 16
        assert int(pairs["mate_crossed"].sum()) >= 8
    assert lc.relation(sites, 0, 1, D) == lc.DUPLICATE and lc.relation(sites, 2, 3, D) == lc.ADJACENT
    tail = exp[320:]
    assert list(tail["event_size"][:2]) == [1, 1] and list(tail["n_adj"][2:4]) == [1, 1] and list(tail["event_size"][4:6]) == [1, 1]
    assert list(tail["n_adj"][6:10]) == [1, 1, 1, 1] and list(tail["n_recip"][6:10]) == [0, 0, 0, 0]
    both = tail[10:14]
    assert list(both["n_recip"]) == [1, 1, 1, 1] and int(both[0]["mate_crossed"]) == (1 if D else 0) and int(both[2]["mate_crossed"]) == 0
    assert list(both[0]["off"]) == [0, 0] and list(both[2]["off"]) == [D, D]
    assert list(tail["n_dup"][14:16]) == [1, 1] and list(tail["n_recip"][14:16]) == [0, 0]
    assert int(tail[16]["event_size"]) == 1 and list(tail["n_adj"][17:19]) == [1, 1] and list(tail["event_size"][17:19]) == [2, 2]
    assert_rows(ctx.link_calls(sites, D), exp)


# ---- 2. positions at both ends of the range -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1000, 1_000_000])
def test_positions_that_would_wrap(ctx, D):
    ends = [1, 3] + list(range(0xFFFFFFF0, 0x100000000))
    rng = np.random.default_rng(4)
    rows = []
    for k, p in enumerate(ends):
        q = ends[(k * 7 + 3) % len(ends)]
        rows.append((0, p, int(rng.integers(0, 2)), 1, q, int(rng.integers(0, 2))))
        rows.append((1, q, int(rng.integers(0, 2)), 0, p, int(rng.integers(0, 2))))
    # on contigs of their own: X at both ends of the range, Y exactly D inside it, Z one base further, W the ends the other way round
    # (1 - 0xFFFFFFFF is 2 in 32 bits), and a row in the middle of the range
    rows += [(2, 1, 0, 3, 0xFFFFFFFF, 1), (2, 1 + D, 0, 3, 0xFFFFFFFF - D, 1), (2, 2 + D, 0, 3, 0xFFFFFFFE - D, 1), (2, 0xFFFFFFFF, 0, 3, 1, 1), (0, 0x80000000, 0, 1, 0x7FFFFFFF, 1)]
    sites = lc.as_sites(rows)
    exp = lc.expected(sites, D)
    n = len(sites)
    X, Y, Z, W = n - 5, n - 4, n - 3, n - 2
    assert [lc.relation(sites, i, j, D) for i, j in ((X, Y), (X, Z), (Y, Z), (X, W), (Y, W))] == [lc.DUPLICATE, lc.NONE, lc.DUPLICATE, lc.NONE, lc.NONE]
    assert int(exp[n - 1]["event_size"]) == 1 and int(exp[W]["event_size"]) == 1 and list(exp["event_size"][[X, Y, Z]]) == [3, 3, 3]
    assert int(exp["n_recip"][:36].sum()) > 0 and int(exp["n_adj"][:36].sum()) > 0 and int(exp["event_size"][:36].max()) >= 18
    assert_rows(ctx.link_calls(sites, D), exp)


# ---- 3. more calls in one window than a step takes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 65, 129])
def test_stacks_inside_one_window(ctx, k):
    rng = np.random.default_rng(k)
    dups = lc.as_sites([(0, 70_000 + int(rng.integers(0, 50)), 0, 1, 90_000 + int(rng.integers(0, 50)), 1) for _ in range(k)])
    exp = lc.expected(dups, 100)
    assert np.all(exp["n_dup"] == k - 1) and list(exp["dup_of"]) == [1] + [0] * (k - 1) and np.all(exp["event_size"] == k) and np.all(exp["event"] == 0)
    assert_rows(ctx.link_calls(dups, 100), exp)
    rows = []
    for _ in range(k):
        a, b = (0, 70_000 + int(rng.integers(0, 150)), int(rng.integers(0, 2))), (1, 90_000 + int(rng.integers(0, 150)), int(rng.integers(0, 2)))
        if rng.random() < 0.2:
            b = (0, 70_000 + int(rng.integers(0, 150)), int(rng.integers(0, 2)))
        rows.append(a + b if rng.random() < 0.5 else b + a)
    mixed = lc.as_sites(rows)
    exp = lc.expected(mixed, 100)
    assert min(int(exp[f].sum()) for f in ("n_dup", "n_recip", "n_adj")) >= k and int(exp["mate_crossed"].sum()) >= 5
    assert_rows(ctx.link_calls(mixed, 100), exp)


# ---- 4. events -----------------------------------------------------------------------------------------------------------------------------
def chain(spots, rng, tid=0, closed=False):
    """sites k = 0 .. len(spots): side 2 of site k and side 1 of site k + 1 lie 5 bases apart at spots[k], and near nothing else; the
    free ends get spots of their own (closed: they share one, a ring)"""
    rows, free = [], [int(spots[-1]) + 1_000_000, int(spots[-1]) + 2_000_000]
    if closed:
        free[1] = free[0] + 5
    for k in range(len(spots) + 1):
        a = free[0] if k == 0 else int(spots[k - 1]) + 5
        b = free[1] if k == len(spots) else int(spots[k])
        rows.append((tid, a, int(rng.integers(0, 2)), tid, b, int(rng.integers(0, 2))))
    return rows


def test_events(ctx):
    """a path of 2000 sites whose joints lie in shuffled order along the contig, the rows shuffled too; a ring of 50; two paths of 40 and
    60 that one site, given last, joins; 300 sites alone between them"""
    rng = np.random.default_rng(11)
    spots = rng.permutation(4000)[:2300] * 10_000 + 10_000
    path = chain(spots[:1999], rng)
    ring = chain(spots[1999:2048], rng, tid=1, closed=True)
    p1, p2 = chain(spots[2048:2087], rng, tid=2), chain(spots[2087:2146], rng, tid=2)
    alone = [(3, int(s), 0, 4, int(s), 1) for s in spots[2146:2146 + 300]]
    rows = path + ring + p1 + p2 + alone
    order = rng.permutation(len(rows))
    rows = [rows[k] for k in order]
    where = np.empty(len(order), np.int64)
    where[order] = np.arange(len(order))  # where[k]: the row that holds the k-th site as built
    joint = (2, p1[-1][4] + 50, 0, 2, p2[0][1] - 50, 1)
    sites = lc.as_sites(rows + [joint])
    exp = lc.expected(sites, 100)
    at = lambda lo, hi: where[lo:hi]
    assert np.all(exp["event_size"][at(0, 2000)] == 2000) and np.all(exp["event"][at(0, 2000)] == at(0, 2000).min())
    assert np.all(exp["event_size"][at(2000, 2050)] == 50) and np.all(exp["n_dup"][at(2000, 2050)] + exp["n_recip"][at(2000, 2050)] + exp["n_adj"][at(2000, 2050)] == 2)
    assert np.all(exp["event_size"][at(2050, 2150)] == 101) and int(exp[-1]["event_size"]) == 101 and int(exp[-1]["event"]) == at(2050, 2150).min()
    assert np.all(exp["event_size"][at(2150, 2450)] == 1)
    got = ctx.link_calls(sites, 100)  # (more rounds than n + 1 would be BK_ERR_LIMIT)
    assert_rows(got, exp)
    assert_rows(ctx.link_calls(sites[:-1], 100), lc.expected_runs(sites[:-1], 100))  # without the joint: two events of 40 and 60


# ---- 5. seeded tables ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    sites = lc.random_sites(np.random.default_rng(50), 5000, D=100)
    return sites, lc.expected(sites, 100)


def test_seeded_table(ctx, seeded):
    """5000 sites on 3 contigs of 50 000 bases: a breakend every 15 bases, so a window holds dozens of calls and nearly all of them chain
    into one event"""
    sites, exp = seeded
    assert min(int(exp[f].sum()) for f in ("n_dup", "n_recip", "n_adj")) >= 500 and int((exp["event_size"] == 1).sum()) >= 10 and int(exp["event_size"].max()) >= 1000
    assert_rows(ctx.link_calls(sites, 100), exp)
    for n in (0, 1, 2):
        assert_rows(ctx.link_calls(sites[:n], 100), lc.expected(sites[:n], 100))
    assert_rows(ctx.link_calls(lc.as_sites([(-1, 7, 0, -1, 7, 1)] * 3), 100), lc.expected(lc.as_sites([(-1, 7, 0, -1, 7, 1)] * 3), 100))


def test_seeded_sparse_table(ctx):
    """the same on contigs of 5 000 000 bases: thousands of runs, and events of every small size"""
    sites = lc.random_sites(np.random.default_rng(51), 5000, length=5_000_000, D=100)
    exp = lc.expected(sites, 100)
    sizes = np.bincount(exp["event_size"])
    assert min(int(exp[f].sum()) for f in ("n_dup", "n_recip", "n_adj")) >= 500 and sizes[1] >= 500 and np.all(sizes[1:6] > 0) and len(np.unique(exp["event"])) >= 1000
    assert_rows(ctx.link_calls(sites, 100), exp)


# ---- 6. stability ------------------------------------------------------------------------------------------------------------------------------
def test_a_permuted_list_and_a_second_run(ctx, seeded):
    sites, exp = seeded
    first = ctx.link_calls(sites, 100)
    assert ctx.link_calls(lc.as_sites([(0, 5, 0, 1, 5, 1)]), 100).tobytes() != first.tobytes()  # (another call in between)
    assert ctx.link_calls(sites, 100).tobytes() == first.tobytes() == exp.tobytes()
    order = np.random.default_rng(6).permutation(len(sites))
    got = ctx.link_calls(sites[order], 100)
    assert_rows(got, lc.expected_runs(sites[order], 100))
    # row k of the permuted list is row order[k] of the first: the same counts, the same event, the same partner at the same offsets
    # wherever the choice does not hang on the index
    for f in ("n_dup", "n_recip", "n_adj", "event_size"):
        assert np.array_equal(got[f], exp[f][order]), f
    groups = lambda ev, name: sorted(sorted(int(name[i]) for i in np.flatnonzero(ev == e)) for e in np.unique(ev))
    assert groups(got["event"], order) == groups(exp["event"], np.arange(len(sites)))
    sums = lambda r: np.abs(r["off"]).sum(1)
    assert np.array_equal(sums(got), sums(exp)[order]) and np.array_equal(got["mate"] >= 0, exp["mate"][order] >= 0)
    single = np.flatnonzero(exp["n_recip"][order] == 1)
    assert len(single) >= 100 and np.array_equal(order[got["mate"][single]], exp["mate"][order][single]) and np.array_equal(got["off"][single], exp["off"][order][single])


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, sites, n, D, out=True):
    C = capi.C
    res = C.c_void_p()
    rc = ctx.L.bk_link_calls(ctx.h, sites.ctypes.data if sites is not None else None, n, D, C.byref(res) if out else None)
    return rc, (ctx.L.bk_last_error(ctx.h) or b"").decode()


def test_argument_refusals(ctx):
    good = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0)])
    rc, msg = raw_call(ctx, good, 2, 1000, out=False)
    assert rc == abi.BK_ERR_ARG and "null out" in msg
    rc, msg = raw_call(ctx, None, 2, 1000)
    assert rc == abi.BK_ERR_ARG and "null sites" in msg
    assert raw_call(ctx, None, 0, 1000)[0] == abi.BK_OK
    for field in ("right1", "right2"):
        bad = good.copy()
        bad[1][field] = 2
        rc, msg = raw_call(ctx, bad, 2, 1000)
        assert rc == abi.BK_ERR_ARG and "site 1 has a right above 1" in msg
    rc, msg = raw_call(ctx, good, 2, abi.LINK_MAX_DIST + 1)
    assert rc == abi.BK_ERR_ARG and "max_dist above 1000000" in msg
    assert raw_call(ctx, good, 2, abi.LINK_MAX_DIST)[0] == abi.BK_OK
    rc, msg = raw_call(ctx, good, (1 << 30) + 1, 1000)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.link_calls(good, 1000)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.link_calls(good, 1000), lc.expected(good, 1000))  # the context still works


# ---- 8. timing and side effects ---------------------------------------------------------------------------------------------------------------
def test_link_is_timed_and_changes_no_stage():
    ds = synth.make_g1()
    cols = ds.to_soa()
    sites = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0), (1, 700400, 0, 2, 5000, 1), (-1, 9, 0, 0, 77, 1)])
    t = capi.Context(ds.contigs)
    t.timing_enable(True)
    got = t.link_calls(sites, 1000)  # before any record is there
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    bytes_model = 4 * 64 + 7 * (24 + 24 * 5)
    assert bytes_model == lc.touched(sites)
    assert names[-1] == "link_calls" and tm["link_calls"][0] > 0 and tm["link_calls"][1] == bytes_model == touched["link_calls"]
    t.timing_enable(False)
    assert_rows(got, lc.expected(sites, 1000))
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=True)  # the stages behind it give the G1 call, as on a context that never made the call
    stages = [t.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)]
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    assert n_valid == 1 and (int(cl[0]["p1_exact"]), int(cl[0]["p2_exact"])) == (50099, 80200)
    assert t.link_calls(sites, 1000).tobytes() == got.tobytes()
    assert [t.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)] == stages
    t.close()
    u = capi.Context(ds.contigs)  # a context that never made the call
    u.upload(cols)
    assert u.run(qual=QUAL, fast=True) == (w, n_valid)
    assert [u.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)] == stages
    u.close()


# ---- 9. command line ---------------------------------------------------------------------------------------------------------------------------
# A junction (A), its reciprocal 3000 bases off on both contigs with both directions flipped (B; the CPU oracle keeps the two apart as
# voted calls of their own at this distance, so the runs take -linkdist 5000), a call that shares only the chr2 region with A (C) and a
# call alone (D).  B lies beside every gene: only -all writes it.
LINK_LOCI = [("A", 0, 300_000, "L", 1, 700_000, "R"), ("B", 0, 303_000, "R", 1, 697_000, "L"), ("C", 1, 704_000, "L", 2, 500_000, "R"), ("D", 2, 1_200_000, "L", 3, 400_000, "R")]
LINKDIST = 5000
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=String," % k for k in ("EVENT", "PARID"))


def link_refgene():
    rows = []
    for gene, chrom, s, e in (("GA1", "chr1", 295_000, 301_000), ("GA2", "chr2", 699_000, 702_000), ("GC1", "chr2", 703_000, 706_000), ("GC2", "chr3", 495_000, 505_000),
                              ("GD1", "chr3", 1_195_000, 1_205_000), ("GD2", "chr4", 395_000, 405_000)):
        rows.append("0\tNM_%s\t%s\t+\t%d\t%d\t%d\t%d\t1\t%d,\t%d,\t0\t%s\tcmpl\tcmpl\t0," % (gene, chrom, s, e, s + 50, e - 50, s, e, gene))
    return rows


@pytest.fixture(scope="module")
def link_run():
    with tempfile.TemporaryDirectory() as tmp:
        ds = cc.designed_tumor(mix=False, loci=LINK_LOCI, n_proper=3000)
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=link_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        t = capi.Context(ds.contigs)
        t.upload(ds.to_soa())
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        sides = [capi.junction_sides(j)[:2] for j in t.junctions()]
        # every voted call, in the order of the rows: what -all would write
        voted = [i for i, c in enumerate(cl) if c["flags"] & 2 and c["n_sr"] > 0 and int(c["p1_exact"]) != 0xFFFFFFFF and int(c["p2_exact"]) != -1]
        sites = lc.as_sites([(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), sides[i][0], int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"]), sides[i][1]) for i in voted])
        links = {}
        for D in (LINKDIST, 0):
            links[D] = t.link_calls(sites, D)
            assert_rows(links[D], lc.expected(sites, D))
        t.close()
        yield {"tmp": tmp, "bam": bam, "nib": side["nib"], "env": env, "cl": cl, "voted": voted, "links": links}


def row_of(cl, name):
    _, ta, bpa, _, tb, bpb, _ = [l for l in LINK_LOCI if l[0] == name][0]
    found = cc.rows_of(cl, ta, bpa, tb, bpb)
    assert len(found) == 1
    return found[0][0]


@pytest.mark.parametrize("variant", ["plain", "vcf", "all_vcf", "dist0"])
def test_cli_link(link_run, variant):
    run = link_run
    tmp, cl, voted = run["tmp"], run["cl"], run["voted"]
    D = 0 if variant == "dist0" else LINKDIST
    link = run["links"][D]
    extra = {"plain": [], "vcf": ["-vcf"], "all_vcf": ["-all", "-vcf"], "dist0": ["-all", "-vcf"]}[variant]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-link", "-linkdist", str(D)], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 0. the designed calls are there, each once, and relate as designed
    A, B, C, Dd = (voted.index(row_of(cl, name)) for name in "ABCD")
    assert len(voted) == 4
    if D:
        assert (int(link[A]["mate"]), int(link[B]["mate"]), int(link[A]["n_adj"]), int(link[C]["n_adj"]), int(link[C]["n_recip"])) == (B, A, 1, 1, 0)
        assert sorted(int(abs(o)) for o in link[A]["off"]) == [3000, 3000] and int(link[A]["event_size"]) == 3 and int(link[Dd]["event_size"]) == 1
        said = "link: 4 calls, 1 events of more than one call, 1 reciprocal pairs"
    else:
        assert np.all(link["event_size"] == 1) and np.all(link["mate"] == -1)
        said = "link: 4 calls, 0 events of more than one call, 0 reciprocal pairs"
    keep = lambda text: [l for l in text.split("\n") if "costs time" not in l]
    assert [l for l in keep(r.stdout) if l != said] == keep(out_a.replace(a, b)) and r.stdout.count(said + "\n") == 1
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_link.txt", "_fusion_link.txt"] if "-all" in extra else ["_fusion_link.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    for suffix in fa:
        if suffix not in {"_params.txt", "_performance.txt", "_fusion.vcf"}:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "link_max_dist\t%d\n" % D, (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's columns, named by rows of BK_STAGE_CLUSTERS
    held = {}
    for twin in twins:
        plain = twin.replace("_link", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(lc.LINK_COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            assert line == s + "\t" + "\t".join(lc.call_fields(link[voted.index(i)], voted)), line
        held[twin] = sorted(calls)
    # B lies beside every gene: the filtered table lacks it, and A names it as its mate all the same
    assert held["_fusion_link.txt"] == sorted(voted[k] for k in (A, C, Dd))
    if "-all" in extra:
        assert held["_fusion_all_link.txt"] == sorted(voted)
    if D:
        a_line = [l for l in open(b + "_fusion_link.txt").read().split("\n") if l.split("\t")[1:2] == ["chr1:300000"]]
        assert len(a_line) == 1 and a_line[0].split("\t")[-4] == "bk%d" % voted[B] and a_line[0].split("\t")[-10] == "ev%d" % min(voted[k] for k in (A, B, C))
    # 3. the VCF: EVENT / PARID last in INFO, their header lines, nothing else touched; no PARID names a record the file lacks
    if "-vcf" not in extra:
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 2 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    head_b = [l for l in vb if l.startswith("#")]
    assert [l for l in va if l.startswith("#")] == [l for l in head_b if not l.startswith(INFO_LINES)]
    at = [k for k, l in enumerate(head_b) if l.startswith(INFO_LINES)]
    assert at[1] == at[0] + 1 and not head_b[at[1] + 1].startswith("##INFO") or "ID=SC," in head_b[at[1] + 1]  # behind every other key of the calls
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    in_file = set(held["_fusion_all_link.txt" if "-all" in extra else "_fusion_link.txt"])
    assert len(body_a) == len(body_b) == 2 * len(in_file)
    ids = set(l.split("\t")[2] for l in body_b)
    tails = {}
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        tail = lc.info_fields(link[voted.index(i)], voted, s, lambda row: row in in_file)
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail, lb
        tails[y[2]] = tail
        for key in y[7].split(";"):
            if key.startswith("PARID="):
                assert key[6:] in ids, lb
    ev = ";EVENT=ev%d" % min(voted[k] for k in (A, B, C))
    if variant == "vcf":  # B's records are not here: A keeps its event and names no partner
        assert tails == {"bk%d_%d" % (voted[k], s): (ev if k != Dd else "") for k in (A, C, Dd) for s in (1, 2)}
    elif variant == "all_vcf":
        assert all(tails["bk%d_%d" % (voted[A], s)] == ev + ";PARID=bk%d_%d" % (voted[B], s) for s in (1, 2)) or \
            all(tails["bk%d_%d" % (voted[A], s)] == ev + ";PARID=bk%d_%d" % (voted[B], 3 - s) for s in (1, 2))
        assert all(tails["bk%d_%d" % (voted[B], s)].startswith(ev + ";PARID=bk%d_" % voted[A]) for s in (1, 2))
        assert all(tails["bk%d_%d" % (voted[C], s)] == ev and tails["bk%d_%d" % (voted[Dd], s)] == "" for s in (1, 2))
    else:
        assert set(tails.values()) == {""} and not any("EVENT=" in l or "PARID=" in l for l in body_b)


def test_cli_link_refusals_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp, refgene_lines=link_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-linkdist", "10"], "-linkdist needs -link."), (["-link", "-linkdist", "1000001"], "-linkdist must be a number from 0 to 1000000."),
                           (["-link", "-linkdist", "-1"], "-linkdist must be a number from 0 to 1000000."), (["-link", "-gpus", "2"], "-link cannot be combined with -gpus."),
                           (["-link", "-covflank", "5"], "-covflank needs -coverage.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-link", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_link.txt", "_fusion_all_link.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(lc.LINK_COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\nlink_max_dist\t1000\n")
        assert "link: 0 calls, 0 events of more than one call, 0 reciprocal pairs\n" in r.stdout

"""Known junctions (`bk_known_calls`, `-known`, `-bedpe`): the kernels against the definition in tests/knowncases.py byte for byte, at the
smallest shapes that can break them: the 64-lane step of the walk, the scan and sort boundaries, the running maximum, the contig
boundaries of the index, both ends of the 32-bit range, the slop to the base, entries on one contig, many hits with few names, missing
contigs, repeated and permuted runs, every refusal, timing; then the command line's files against the definition and the round trip
through -bedpe."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import knowncases as kc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = [("c0", 5_000_000), ("c1", 5_000_000), ("c2", 1_000_000)]
N = kc.NO_SCORE


@pytest.fixture(scope="module")
def ctx():
    """a context that holds no records: bk_known_calls needs none"""
    t = capi.Context(CONTIGS)
    yield t
    t.close()


def assert_rows(got, exp):
    assert got.dtype == abi.KNOWN_CALL and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def check(ctx, entries, sites, slop):
    exp = kc.expected(entries, sites, slop)
    assert_rows(ctx.known_calls(entries, sites, slop), exp)
    return exp


# ---- 1. the 64-lane step of the walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 128, 129])
def test_interval_ends_inside_one_walk(ctx, k):
    """k intervals hold breakend 0 of the one site (every third of their entries is a hit, through either mapping), between intervals
    that begin behind x + slop and intervals that end in front of x - slop"""
    slop, x0, x1 = 10, 100_000, 200_000
    rows = []
    for j in range(k):
        other = (1, x1 - 5, x1 + 5) if j % 3 == 0 else (1, x1 + 500, x1 + 600)
        own = (0, x0 - 3 * j - 1, x0 + 1 + j % 2)
        rows.append((own + other if j % 2 else other + own) + (j % 5, j % 7, 0, 0))
    rows += [(0, x0 + slop + 1 + j, x0 + 900, 1, x1, x1 + 1, 9, 50, 0, 0) for j in range(70)]     # begin one or more behind x + slop
    rows += [(0, x0 - 5000 - j, x0 - slop - j, 1, x1, x1 + 1, 9, 50, 0, 0) for j in range(70)]    # end - 1 is one or more in front of x - slop
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, x0 + 1, 0, 1, x1 + 1, 1)])
    exp = check(ctx, entries, sites, slop)
    assert int(exp[0]["n_side"][0]) == k and int(exp[0]["n_hits"]) == (k + 2) // 3 and int(exp[0]["n_side"][1]) == 140 + (k + 2) // 3


# ---- 2. the scan and sort boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sites", [255, 256, 257])
@pytest.mark.parametrize("n_entries", [0, 1, 300])
def test_site_and_entry_counts(ctx, n_sites, n_entries):
    rng = np.random.default_rng(1000 * n_sites + n_entries)
    entries, sites = kc.random_case(rng, n_sites, n_entries, 20)
    if n_entries == 1:  # the one entry holds the last site
        b = kc.breakends(sites[-1])
        entries = kc.as_entries([(b[0][0], max(b[0][1] - 3, 0), b[0][1] + 3, b[1][0], max(b[1][1] - 3, 0), b[1][1] + 3, 0, 4, 0, 0)])
    exp = check(ctx, entries, sites, 20)
    assert n_entries == 0 or int(exp["n_hits"].sum()) >= 1
    assert n_entries != 0 or (np.all(exp["best"] == -1) and np.all(exp["best_score"] == N) and not exp["n_side"].any())


# ---- 3. the running maximum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_end", [2_000_000, 1_400_000])
def test_a_long_interval_in_front_of_thousands_of_short_ones(ctx, long_end):
    """the site lies behind 5000 short intervals, none of which reaches it; the long interval in front of them does (the walk has to go
    all the way back) or ends 100 000 bases short (the walk stops at once)"""
    rows = [(0, 100, long_end, 1, 10, 20, 7, 1, 0, 0)] + [(0, 1000 + 100 * j, 1010 + 100 * j, 1, 10, 20, j % 3, 1, 0, 0) for j in range(5000)]
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, 1_500_000, 0, 1, 15, 1), (0, 1_500_000, 0, 2, 15, 1), (0, 700_000, 1, 1, 5015, 0)])
    exp = check(ctx, entries, sites, 100)
    reached = long_end > 1_500_000
    assert list(exp["n_side"][:, 0]) == [int(reached), int(reached), 1] and list(exp["n_hits"]) == [int(reached), 0, 0]
    assert int(exp[0]["n_side"][1]) == 5001 and int(exp[2]["n_side"][1]) == 0


# ---- 4. the contigs of the index -------------------------------------------------------------------------------------------------------------
def test_contig_boundaries_of_the_index(ctx):
    """the last interval of contig 0 stands next to the first of contig 2 in sorted order (contig 1 has none); sites on contig 1, on a
    contig beyond every entry, and at both of those intervals with a slop that reaches across the key's 32 bits"""
    rows = [(0, 0xFFFFFF00, 0xFFFFFFFF, 2, 0, 50, 0, 1, 0, 0), (2, 0, 40, 0, 0xFFFFFFF0, 0xFFFFFFFF, 1, 2, 0, 0), (0, 500, 600, 2, 700, 800, 2, 3, 0, 0)]
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(1, 10, 0, 1, 0xFFFFFFFF, 1), (7, 10, 0, 9, 20, 1), (0, 0xFFFFFFFF, 0, 2, 1, 1), (2, 1, 0, 0, 0xFFFFFFFF, 1), (2, 60, 0, 0, 0xFFFFFF00, 1),
                         (1, 1, 0, 2, 1, 0), (0, 550, 0, 1, 0xFFFFFFFF, 1), (2, 0, 0, 0, 0, 0)])
    for slop in (0, 30, 1_000_000):
        exp = check(ctx, entries, sites, slop)
        assert not exp[0]["n_side"].any() and not exp[1]["n_side"].any() and int(exp[2]["n_hits"]) == 2 and int(exp[3]["n_hits"]) == 2
    assert int(kc.expected(entries, sites, 30)[4]["n_hits"]) == 1 and int(kc.expected(entries, sites, 0)[4]["n_hits"]) == 0


# ---- 5. both ends of the 32-bit range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slop", [0, 1_000_000])
def test_positions_that_would_wrap(ctx, slop):
    top = 0xFFFFFFFF
    rows = [(0, 0, 1, 1, top - 1, top, 0, 1, 0, 0), (0, 0, top, 1, 0, top, 1, 2, 0, 0), (1, top - 1, top, 0, 0, 1, 2, 3, 0, 0), (0, top - 5, top, 1, 0, 3, 3, 4, 0, 0),
            (0, slop + 1, slop + 2, 1, top - slop - 2, top - slop - 1, 4, 5, 0, 0), (0, slop, slop + 1, 1, top - slop - 1, top - slop, 5, 6, 0, 0)]
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, 1, 0, 1, top, 1), (1, top, 0, 0, 1, 1), (0, top, 0, 1, 1, 1), (0, 0, 0, 1, top, 1), (0, 1, 0, 1, 0, 1), (1, 1, 1, 1, top, 0)])
    exp = check(ctx, entries, sites, slop)
    # site 0 = (x 0, x top - 1): e0, e1, e2 (crossed) and e5, whose two intervals lie exactly slop off, hold it; e4 at slop + 1 does not
    assert int(exp[0]["n_hits"]) == 4 and kc.hit_of(sites[0], entries[5], slop)[3] == 2 * slop and kc.hit_of(sites[0], entries[4], slop) is None
    assert (int(exp[1]["n_hits"]), int(exp[1]["best"]), int(exp[1]["best_crossed"])) == (4, 5, 1)  # the same junction the other way round
    assert int(exp[3]["n_side"][0]) == (3 if slop else 0)  # P = 0 is x = -1: one base in front of beg 0


# ---- 6. the slop to the base ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slop", [0, 1, 100, 1_000_000])
def test_dist_equal_to_the_slop_and_one_more(ctx, slop):
    x0, x1 = 2_000_000, 3_000_000
    rows = []
    for d0 in (slop, slop + 1, -slop, -slop - 1):      # the interval begins d0 behind x (d0 > 0) or its last base lies -d0 in front of it
        for d1 in (0, slop, slop + 1, -slop, -slop - 1):
            iv = [(t, x + d, x + d + 4) if d > 0 else (t, x + d - 3, x + d + 1) for t, x, d in ((0, x0, d0), (1, x1, d1))]
            rows.append(iv[0] + iv[1] + (len(rows), len(rows), 0, 0))
            rows.append(iv[1] + iv[0] + (len(rows), len(rows), 0, 0))
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, x0 + 1, 0, 1, x1 + 1, 1), (1, x1 + 1, 0, 0, x0 + 1, 1)])
    exp = check(ctx, entries, sites, slop)
    held = {e >> 1 for e in range(len(rows)) if kc.hit_of(sites[0], entries[e], slop) is not None}
    assert held == {5 * a + b for a in (0, 2) for b in (0, 1, 3)}  # exactly the slop on either side holds, one more does not
    assert int(exp[0]["n_hits"]) == 2 * len(held) and int(exp[0]["best_dist"]) <= 2 * slop


# ---- 7. entries on one contig ----------------------------------------------------------------------------------------------------------------
def test_same_contig_entries(ctx):
    rows = [(0, 1000, 1100, 0, 1050, 1200, 0, 5, 0, 0),                       # both intervals hold breakend 0 of site 0, none breakend 1: n_side once
            (0, 1000, 1100, 0, 1050, 1200, 1, 5, kc.LEFT, kc.RIGHT),           # site 1 lies in both with both breakends: both mappings hold, straight agrees
            (0, 1000, 1100, 0, 1050, 1200, 2, 5, kc.RIGHT, kc.LEFT),           # ... crossed agrees
            (0, 1000, 1100, 0, 1050, 1200, 3, 5, kc.LEFT, kc.LEFT),            # ... neither agrees: the smaller dist, here equal, so straight
            (0, 1060, 1070, 0, 1080, 1090, 4, 5, 0, 0),                        # ... unstated, straight is nearer (0 against 36)
            (0, 1080, 1090, 0, 1060, 1070, 4, 5, 0, 0)]                        # ... unstated, crossed is nearer
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, 1061, 0, 1, 5000, 1), (0, 1061, 0, 0, 1086, 1), (0, 1086, 0, 0, 1061, 1)])
    exp = check(ctx, entries, sites, 30)
    assert list(exp[0]["n_side"]) == [6, 0] and int(exp[0]["n_hits"]) == 0
    assert int(exp[1]["n_hits"]) == 6 and list(exp[1]["n_side"]) == [6, 6] and (int(exp[1]["n_oriented"]), int(exp[1]["n_opposed"])) == (2, 1)
    maps = [kc.hit_of(sites[1], e, 30)[0] for e in entries]
    assert maps == [0, 0, 1, 0, 0, 1] and [kc.hit_of(sites[2], e, 30)[0] for e in entries] == [0, 0, 1, 0, 1, 0]
    assert int(exp[1]["best"]) == 0 and int(exp[1]["best_dist"]) == 0


# ---- 8. many hits, few names -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 200])
def test_many_hits_with_few_names(ctx, k):
    rng = np.random.default_rng(k)
    names = [3, 70_000, 0x12345678, 0]
    rows = [(0, 1000 - j, 1001 + j, 1, 2000 - 2 * j, 2001, names[j % 3], int(rng.integers(0, 4)), 0, 0) for j in range(k)]
    rows += [(0, 900_000, 900_010, 1, 5, 6, names[3], 1, 0, 0), (2, 5, 50, 1, 2000, 2001, 0xFFFFFFFF, 9, 0, 0)]
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, 1001, 0, 1, 2001, 1), (2, 10, 0, 1, 2001, 1), (0, 900_001, 0, 1, 6, 0), (1, 2001, 1, 0, 1001, 0), (0, 1001, 0, 2, 10, 1)])
    exp = check(ctx, entries, sites, 5)
    assert list(exp["n_hits"]) == [k, 1, 1, k, 0] and list(exp["n_names"]) == [3, 1, 1, 3, 0] and int(exp[3]["best_crossed"]) == 1


# ---- 9. sides without a contig -----------------------------------------------------------------------------------------------------------------
def test_missing_contigs(ctx):
    rows = [(-1, 100, 50, 1, 2000, 2100, 0, 1, 0, 0), (0, 1000, 1100, -1, 0, 0, 1, 2, 0, 0), (-1, 0, 0, -5, 9, 3, 2, 3, 0, 0), (0, 1000, 1100, 1, 2000, 2100, 3, 4, 0, 0)]
    entries = kc.as_entries(rows)
    sites = kc.as_sites([(0, 1050, 0, 1, 2050, 1), (-1, 1050, 0, 1, 2050, 1), (0, 1050, 0, -1, 2050, 1), (-1, 1050, 0, -1, 2050, 1), (-1, 100, 0, -1, 100, 0)])
    exp = check(ctx, entries, sites, 0)
    assert [list(r) for r in exp["n_side"]] == [[2, 2], [0, 2], [2, 0], [0, 0], [0, 0]] and list(exp["n_hits"]) == [1, 0, 0, 0, 0]
    check(ctx, entries[:3], sites, 1000)
    check(ctx, entries[2:3], sites, 1000)  # no interval has a contig: the index is empty


# ---- 10. seeded tables, repeated and permuted runs -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    rng = np.random.default_rng(77)
    entries, sites = kc.random_case(rng, 300, 500, 100, n_contigs=3, length=200_000, n_names=5)
    return entries, sites, {slop: kc.expected(entries, sites, slop) for slop in (100, 3)}


def test_seeded_table(ctx, seeded):
    entries, sites, exp = seeded
    assert_rows(ctx.known_calls(entries, sites, 100), exp[100])
    e = exp[100]
    assert int((e["n_hits"] > 0).sum()) >= 50 and int(e["best_crossed"].sum()) >= 10 and int((e["n_names"] < e["n_hits"]).sum()) >= 5 and int((e["n_hits"] == 0).sum()) >= 100, \
        [int((e["n_hits"] > 0).sum()), int(e["best_crossed"].sum()), int((e["n_names"] < e["n_hits"]).sum()), int((e["n_hits"] == 0).sum())]


def test_two_runs_a_permuted_list_and_two_slops_in_alternation(ctx, seeded):
    entries, sites, exp = seeded
    first = ctx.known_calls(entries, sites, 100)
    for slop in (3, 100, 3, 100):
        got = ctx.known_calls(entries, sites, slop)
        assert_rows(got, exp[slop])
        assert slop != 100 or got.tobytes() == first.tobytes()
    perm = np.random.default_rng(5).permutation(len(sites))
    assert_rows(ctx.known_calls(entries, sites[perm], 100), exp[100][perm])
    # a smaller panel and a smaller list after a larger one: the buffers are reused
    assert_rows(ctx.known_calls(entries[:7], sites[:9], 100), kc.expected(entries[:7], sites[:9], 100))
    assert_rows(ctx.known_calls(entries, sites[:0], 100), exp[100][:0])


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, entries, n_entries, sites, n, slop, out=True):
    C = capi.C
    res = C.c_void_p()
    rc = ctx.L.bk_known_calls(ctx.h, entries.ctypes.data if entries is not None else None, n_entries, sites.ctypes.data if sites is not None else None, n, slop,
                              C.byref(res) if out else None)
    return rc, (ctx.L.bk_last_error(ctx.h) or b"").decode()


def test_argument_refusals(ctx):
    entries = kc.as_entries([(0, 299950, 300050, 1, 699900, 700100, 0, 12, kc.LEFT, kc.RIGHT), (1, 700050, 700060, 0, 299000, 299990, 1, 40, kc.RIGHT, kc.LEFT)])
    sites = kc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0)])
    assert raw_call(ctx, entries, 2, sites, 2, 100, out=False) == (abi.BK_ERR_ARG, "bk_known_calls: null out")
    rc, msg = raw_call(ctx, entries, 2, None, 2, 100)
    assert rc == abi.BK_ERR_ARG and "null sites" in msg
    rc, msg = raw_call(ctx, None, 2, sites, 2, 100)
    assert rc == abi.BK_ERR_ARG and "null entries" in msg
    assert raw_call(ctx, None, 0, None, 0, 100)[0] == abi.BK_OK and raw_call(ctx, None, 0, sites, 2, 100)[0] == abi.BK_OK
    for field in ("right1", "right2"):
        bad = sites.copy()
        bad[1][field] = 2
        rc, msg = raw_call(ctx, entries, 2, bad, 2, 100)
        assert rc == abi.BK_ERR_ARG and "site 1 has a right above 1" in msg
    for field in ("strand1", "strand2"):
        bad = entries.copy()
        bad[1][field] = 3
        rc, msg = raw_call(ctx, bad, 2, sites, 2, 100)
        assert rc == abi.BK_ERR_ARG and "entry 1 has a strand above 2" in msg
    for table, what in ((sites, "site"), (entries, "entry")):
        bad = table.copy()
        bad[1]["reserved"][5] = 1
        rc, msg = raw_call(ctx, bad if what == "entry" else entries, 2, bad if what == "site" else sites, 2, 100)
        assert rc == abi.BK_ERR_ARG and "%s 1 has a non-zero reserved field" % what in msg
    for beg, end in (("beg1", "end1"), ("beg2", "end2")):
        for value in (0, 1):
            bad = entries.copy()
            bad[0][end] = int(bad[0][beg]) + value - 1 if value == 0 else bad[0][beg]
            rc, msg = raw_call(ctx, bad, 2, sites, 2, 100)
            assert rc == abi.BK_ERR_ARG and "entry 0 has an interval with end <= beg" in msg
    rc, msg = raw_call(ctx, entries, 2, sites, 2, abi.KNOWN_MAX_SLOP + 1)
    assert rc == abi.BK_ERR_ARG and "slop above 1000000" in msg
    assert raw_call(ctx, entries, 2, sites, 2, abi.KNOWN_MAX_SLOP)[0] == abi.BK_OK
    rc, msg = raw_call(ctx, entries, 2, sites, (1 << 30) + 1, 100)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg
    rc, msg = raw_call(ctx, entries, (1 << 30) + 1, sites, 2, 100)
    assert rc == abi.BK_ERR_LIMIT and "2^30 entries" in msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.known_calls(entries, sites, 100)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.known_calls(entries, sites, 100), kc.expected(entries, sites, 100))  # the context still works


# ---- 12. timing and side effects ---------------------------------------------------------------------------------------------------------------
def hand_example():
    entries = kc.as_entries([(0, 299950, 300050, 1, 699900, 700100, 0, 12, kc.LEFT, kc.RIGHT), (1, 700050, 700060, 0, 299000, 299990, 1, 40, kc.RIGHT, kc.LEFT),
                             (0, 299990, 300010, 0, 100, 200, 0, N, 0, 0), (1, 699000, 701000, 1, 699500, 700500, 2, N, 0, 0)])
    return entries, kc.as_sites([(0, 300000, 0, 1, 700000, 1)])


def test_known_is_timed_and_changes_no_stage():
    ds = synth.make_g1()
    cols = ds.to_soa()
    entries, sites = hand_example()
    sites = np.concatenate([sites, kc.as_sites([(1, 700000, 1, 0, 300000, 0), (-1, 9, 0, 0, 5000, 1)])])
    t = capi.Context(ds.contigs)
    t.timing_enable(True)
    got = t.known_calls(entries, sites, 100)  # before any record is there
    timing = t.timing()
    names = [name for name, _, _ in timing]
    touched = t.timing_touched()
    assert names[-3:] == ["known_calls", "known_calls_index", "known_calls_sites"]
    # the byte model, restated: 4 entries on tids 0 and 1 (34 key bits: 5 passes) with 8 intervals; 3 sites (2 site bits: 1 pass), names up to 2
    # (1 pass), and 4 listed hits (two at each of the first two sites)
    index, at_sites = 4 * (40 + 24 + 48 * 5) + 16 * 8, 3 * 80 + 4 * (12 + 24 * 2)
    assert (index, at_sites, index + at_sites) == kc.touched(entries, sites, 4)
    assert list(touched[-3:]) == [index + at_sites, index, at_sites] and [by for _, _, by in timing[-3:]] == [index + at_sites, index, at_sites]
    assert all(ms > 0 for _, ms, _ in timing[-3:]) and timing[-3][1] >= timing[-2][1]
    t.timing_enable(False)
    exp = kc.expected(entries, sites, 100)
    assert_rows(got, exp)
    r = got[0]  # the header's hand example, field by field
    assert (int(r["n_hits"]), int(r["n_oriented"]), int(r["n_opposed"]), int(r["n_names"]), list(r["n_side"])) == (2, 2, 0, 2, [3, 3])
    assert (int(r["best"]), int(r["best_score"]), int(r["best_dist"]), int(r["best_crossed"]), int(r["best_oriented"])) == (1, 40, 61, 1, 1)
    assert (int(got[1]["best"]), int(got[1]["best_crossed"]), int(got[1]["n_hits"])) == (1, 0, 2) and int(got[2]["n_side"][1]) == 0
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=True)  # the stages behind it give the G1 call, as on a context that never made the call
    stages = [t.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)]
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    assert n_valid == 1 and (int(cl[0]["p1_exact"]), int(cl[0]["p2_exact"])) == (50099, 80200)
    assert t.known_calls(entries, sites, 100).tobytes() == got.tobytes()
    assert [t.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)] == stages
    t.close()
    u = capi.Context(ds.contigs)  # a context that never made the call
    u.upload(cols)
    assert u.run(qual=QUAL, fast=True) == (w, n_valid)
    assert [u.fetch(st)[0].tobytes() for st in (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)] == stages
    u.close()


# ---- 13. command line ------------------------------------------------------------------------------------------------------------------------
# The panel against the first four loci of tests/callcases.py (LR_x chr1:300000 L / chr2:700000 R, LL_x chr1:600000 L / chr3:500000 L,
# RR_x chr2:300000 R / chr4:900000 R, RL_x chr3:900000 R / chr4:400000 L), written with chr1's interval first.
PANEL = "\n".join([
    "# a panel for the designed tumour", "track name=panel", "",
    "chr1\t299900\t300100\tchr2\t699900\t700100\tfusA\t10\t+\t-",        # LR_x, straight when side 1 is chr1, agreeing
    "chr1 299990 300001 chr2 699999 700050 fusA",                           # LR_x again under the same name, no score, unstated
    "chr3 499950 500050 chr1 599950 600050 fusB 5 + +",                     # LL_x the other way round, agreeing
    "chr2 299990 300010 chr4 899990 900010 pon 3.7 + +",                    # RR_x with the opposite strands: opposed
    "chr3 899900 900100 chr1 1 2 lone 1",                                   # one partner of RL_x only
    "chrZ 1 2 chr4 399900 400100 ghost 9 + -",                              # a contig the input lacks; the other partner of RL_x
    ". -1 -1 . -1 -1",
    "chr4 1999990 2000500 chr4 2000000 2000010 edge 2",                     # clamped to the contig's length; the second lies behind its end
]) + "\n"
KNOWN_INFO = tuple("##INFO=<ID=%s,Number=1,Type=%s," % k for k in (("KNOWN", "Integer"), ("KNAMES", "Integer"), ("KBEST", "String")))
SLOP = 100


def outputs(tmp, prefix):
    return sorted(f[len(prefix):] for f in os.listdir(tmp) if f.startswith(prefix + "_"))


def call_sites(cl, jn, calls):
    rows = []
    for i in calls:
        r1, r2, source = capi.junction_sides(jn[i])
        rows.append((int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), r1 if source else 0, int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"]), r2 if source else 0))
    return kc.as_sites(rows)


@pytest.fixture(scope="module")
def known_run():
    with tempfile.TemporaryDirectory() as tmp:
        ds = cc.designed_tumor(mix=False, n_proper=3000)
        bam, nbam, panel = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "panel.bedpe")
        cc.write_indexed(ds, bam)
        cc.write_indexed(cc.designed_normal(), nbam)
        open(panel, "w").write(PANEL)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        t = capi.Context(ds.contigs)
        t.upload(ds.to_soa())
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        jn = t.junctions()
        entries, names, unknown = kc.read_bedpe(PANEL, cc.CONTIGS)
        assert unknown == 2 and len(entries) == 8 and names == ["fusA", "fusB", "pon", "lone", "ghost", ".", "edge"]
        yield {"tmp": tmp, "bam": bam, "nbam": nbam, "panel": panel, "nib": side["nib"], "env": env, "cl": cl, "jn": jn, "ctx": t, "entries": entries, "names": names}
        t.close()


@pytest.mark.parametrize("variant", ["plain", "all", "vcf_normal_genotype_link"])
def test_cli_known(known_run, variant):
    run = known_run
    tmp, cl, jn, entries, names = run["tmp"], run["cl"], run["jn"], run["entries"], run["names"]
    extra = {"plain": [], "all": ["-all", "-vcf"], "vcf_normal_genotype_link": ["-vcf", "-normal", run["nbam"], "-genotype", "-link"]}[variant]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    ra = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert ra.returncode == 0, ra.stderr[-2000:]
    rb = subprocess.run(base + ["-o", b, "-known", run["panel"], "-bedpe"], env=run["env"], capture_output=True, text=True)
    assert rb.returncode == 0, rb.stderr[-2000:]
    last = "_fusion_all.txt" if "-all" in extra else "_fusion.txt"
    calls = written_calls(cl, b + last)
    sites = call_sites(cl, jn, calls)
    rows = dict(zip(calls, kc.expected(entries, sites, SLOP)))
    assert_rows(run["ctx"].known_calls(entries, sites, SLOP), np.array([rows[i] for i in calls], abi.KNOWN_CALL))
    # 0. the designed calls meet the panel as designed
    at = {}
    for name, ta, bpa, da, tb, bpb, db in cc.LOCI[:4]:
        found = cc.rows_of(cl, ta, bpa, tb, bpb)
        assert len(found) == 1 and found[0][0] in calls
        at[name] = (rows[found[0][0]], found[0][1])
    r, a_first = at["LR_x"]
    assert (int(r["n_hits"]), int(r["n_names"]), int(r["n_oriented"]), int(r["n_opposed"]), int(r["best"]), int(r["best_score"]), int(r["best_crossed"])) == (2, 1, 1, 0, 0, 10, int(not a_first))
    r, a_first = at["LL_x"]
    assert (int(r["n_hits"]), int(r["n_oriented"]), int(r["best"]), int(r["best_score"]), int(r["best_crossed"])) == (1, 1, 2, 5, int(a_first))
    r, _ = at["RR_x"]
    assert (int(r["n_hits"]), int(r["n_oriented"]), int(r["n_opposed"]), int(r["best_score"])) == (1, 0, 1, 3)
    r, _ = at["RL_x"]
    assert int(r["n_hits"]) == 0 and list(r["n_side"]) == [1, 1] and int(r["best"]) == -1
    with_hit = sum(int(r["n_hits"]) > 0 for r in rows.values())
    # 1. the files: the twins and the BEDPE files are new, params / performance (and the VCF) change, every other file is byte-identical
    twins = ["_fusion_known.txt"] + (["_fusion_all_known.txt"] if "-all" in extra else [])
    beds = ["_fusion.bedpe"] + (["_fusion_all.bedpe"] if "-all" in extra else [])
    fa, fb = outputs(tmp, os.path.basename(a)), outputs(tmp, os.path.basename(b))
    assert fb == sorted(fa + twins + beds), (fa, fb)
    changed = {"_params.txt", "_performance.txt"} | ({"_fusion.vcf"} if "-vcf" in extra else set())
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "known_file\t%s\nknown_slop\t100\nbedpe\n" % run["panel"], (pa, pb)
    said = "known: 8 entries, 2 on contigs the input lacks, %d calls with a hit" % with_hit
    keep = lambda text: [l for l in text.split("\n") if "costs time" not in l]
    assert [l for l in keep(rb.stdout) if l != said] == keep(ra.stdout.replace(a, b)) and rb.stdout.count(said + "\n") == 1
    assert "Warning: 2 lines of the known file %s name contigs that are not in the BAM header" % run["panel"] in rb.stderr
    # 2. the twins: the rows of their fusion table in its order, then the definition's columns; the BEDPE files: the same rows
    for twin, bed in zip(twins, beds):
        plain = twin.replace("_known", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(kc.KNOWN_COLUMNS)
        here = written_calls(cl, b + plain)
        assert len(here) == len(lines) - 2 and len(here) >= 4
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in here}
        bed_lines = open(b + bed).read().split("\n")
        assert len(bed_lines) == len(src) - 1 and bed_lines[-1] == ""
        for text, s, bl in zip(lines[1:-1], src[1:-1], bed_lines[:-1]):
            f = text.split("\t")
            i = by_key[(f[1], f[2])]
            assert text == s + "\t" + "\t".join(kc.call_fields(rows[i], entries, names)), text
            r1, r2, source = capi.junction_sides(jn[i])
            assert bl == kc.bedpe_line(cc.NAMES[cl[i]["p1_tid"]], int(cl[i]["p1_exact"]), cc.NAMES[cl[i]["p2_tid"]], int(cl[i]["p2_exact"]), os.path.basename(b), int(cl[i]["n_drp"]),
                                       int(cl[i]["n_sr"]), kc.strand_text(r1, source), kc.strand_text(r2, source), i, f[0]), bl
    if "-vcf" not in extra:
        return
    # 3. the VCF: KNOWN / KNAMES (and KBEST where there is a hit) last in INFO on both breakends, their header lines behind every older key
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in KNOWN_INFO)
    head_b = [l for l in vb if l.startswith("#")]
    assert [l for l in va if l.startswith("#")] == [l for l in head_b if not l.startswith(KNOWN_INFO)]
    where = [k for k, l in enumerate(head_b) if l.startswith(KNOWN_INFO)]
    assert where == list(range(where[0], where[0] + 3)) and not head_b[where[2] + 1].startswith("##INFO")
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 2 * len(calls)
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        u = rows[int(y[2][2:].split("_")[0])]
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + kc.info_fields(u, entries, names), lb
    assert sum(";KBEST=fusA" in l for l in body_b) == 2 and any(l.split("\t")[7].endswith(";KNOWN=0;KNAMES=0") for l in body_b)


def test_cli_round_trip_through_bedpe(known_run):
    """a run with -bedpe -all, then the same input with -known <its own out_fusion_all.bedpe> -knownslop 0 -all: every row is a hit of its
    own line at distance 0, nothing opposes, and the best name is the first run's prefix"""
    run = known_run
    tmp = run["tmp"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-fast", "-all"]
    first, second = os.path.join(tmp, "first"), os.path.join(tmp, "second")
    r = subprocess.run(base + ["-o", first, "-bedpe"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(first + "_params.txt").read().endswith("bedpe\n") and "known" not in r.stdout
    bed = [l.split("\t") for l in open(first + "_fusion_all.bedpe").read().split("\n")[:-1]]
    n_rows = len(open(first + "_fusion_all.txt").read().split("\n")) - 2
    assert len(bed) == n_rows >= 8 and all(len(f) == 14 and f[6] == "first" and int(f[7]) == int(f[12]) + int(f[13]) for f in bed)
    r = subprocess.run(base + ["-o", second, "-known", first + "_fusion_all.bedpe", "-knownslop", "0"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "known: %d entries, 0 on contigs the input lacks, %d calls with a hit\n" % (n_rows, n_rows) in r.stdout and "Warning" not in r.stderr
    assert open(second + "_params.txt").read().endswith("known_file\t%s\nknown_slop\t0\n" % (first + "_fusion_all.bedpe"))
    for twin in ("_fusion_all_known.txt", "_fusion_known.txt"):
        lines = open(second + twin).read().split("\n")
        head = lines[0].split("\t")
        col = {name: head.index(name) for name in kc.KNOWN_COLUMNS}
        assert len(lines) - 2 == (n_rows if "all" in twin else len(open(first + "_fusion.txt").read().split("\n")) - 2)
        for text in lines[1:-1]:
            f = text.split("\t")
            assert int(f[col["Kn_Hits"]]) >= 1 and f[col["Kn_BestDist"]] == "0" and f[col["Kn_Opposed"]] == "0" and f[col["Kn_Best"]] == "first", text
            assert int(f[col["Kn_Oriented"]]) >= 1 and f[col["Kn_BestMap"]] == "straight" and int(f[col["Kn_Score"]]) == int(f[7]) + int(f[8]), text
    assert not os.path.exists(second + "_fusion_all.bedpe")


def test_cli_known_limits_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb, panel = os.path.join(tmp, "t.bam"), os.path.join(tmp, "p.bedpe")
        cc.write_indexed(tum, tb)
        open(panel, "w").write(PANEL)
        side = synth.write_side_files(tum, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        missing = os.path.join(tmp, "missing.bedpe")
        for args, word in ((["-knownslop", "10"], " Error: -knownslop needs -known."), (["-known", panel, "-knownslop", "1000001"], " Error: -knownslop must be a number from 0 to 1000000."),
                           (["-known", panel, "-knownslop", "-1"], " Error: -knownslop must be a number from 0 to 1000000."),
                           (["-known", panel, "-gpus", "2"], " Error: -known cannot be combined with -gpus."), (["-bedpe", "-gpus", "2"], " Error: -bedpe cannot be combined with -gpus."),
                           (["-known", panel, "-linkdist", "5"], " Error: -linkdist needs -link."), (["-known", missing], "Error: can not open known file: " + missing),
                           (["-known", missing, "-bedpe", "-knownslop", "7"], "Error: can not open known file: " + missing),
                           (["-known", missing, "-bedpe", "-gpus", "2"], " Error: -known cannot be combined with -gpus.")):  # (an earlier row of the table)
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [word], (args, r.stderr[-2000:])
        # a line that ends the run does so with its number, before anything is written
        for text, line, why in (("chr1 1 2 chr2 3\n", 1, "fewer than six fields"), ("#\n\nchr1 1 2 chr2 3 x\n", 3, "not a number: x"), ("chr1 -1 2 chr2 3 4\n", 1, "negative coordinate: -1"),
                                ("chr1 1 2 chr2 4 4\n", 1, "end <= start")):
            bad = os.path.join(tmp, "bad.bedpe")
            open(bad, "w").write(text)
            r = subprocess.run(base + ["-known", bad], env=env, capture_output=True, text=True)
            assert r.returncode == 1 and "Error: known file %s, line %d: %s" % (bad, line, why) in r.stderr, r.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-known", panel, "-knownslop", "1000000", "-bedpe", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_known.txt", "_fusion_all_known.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(kc.KNOWN_COLUMNS) + "\n"
        assert open(prefix + "_fusion.bedpe").read() == "" and open(prefix + "_fusion_all.bedpe").read() == ""
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in KNOWN_INFO)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\nknown_file\t%s\nknown_slop\t1000000\nbedpe\n" % panel)
        assert "known: 8 entries, 2 on contigs the input lacks, 0 calls with a hit\n" in r.stdout

"""Soft-clip evidence (`bk_clip_support`, `bk_base_depth`, `bk_clip_rescue`, `-clip`): the counts of every cluster against a numpy
evaluation of their definition (include/breakid_hip.h) over the record table, exact and with no row left out; one call with
hand-placed records on either side of every clause of the definition; windows wider than a tile and a pile deeper than a byte; the
synthetic truth of designed loci; the depth at arbitrary positions; every table form a context can hold; the command line."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import clipcases as kc
from tests.callcases import BIN, QUAL, EXCLUDE, designed_refgene, filtered, make_ctx, rec_endpos, single_base_depth, to_device, write_indexed
from tests.clipcases import CLIP_TILE, LEFT, RIGHT, expected_clip_support

pytestmark = pytest.mark.gpu


def assert_rows_equal(got, exp, cl):
    assert got.dtype == abi.CLIP_SUPPORT and len(got) == len(exp) == len(cl)
    bad = [i for i in range(len(cl)) if got[i] != exp[i]]
    assert not bad, [(cl[i], got[i], exp[i]) for i in bad[:3]]


_SHARED = {}


def dataset(name):
    if name not in _SHARED:
        if name == "tumor":
            _SHARED[name] = cc.tumor()
        elif name == "edge":
            _SHARED[name] = cc.call_dataset("edge")
        else:
            ds = {"clipped": kc.clipped_tumor, "designed": kc.clip_tumor}[name]()
            _SHARED[name] = (ds, ds.to_soa())
    return _SHARED[name]


# ---- 1. the definition on seeded data -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", ["tumor", "edge", "clipped"])
def test_clip_support_equals_its_definition(name, fast):
    ds, cols = dataset(name)
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=fast)
    before, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert len(before) > 0
    for min_clip in (1, 10, 25):
        for mapq_min in (0, 20):
            got = t.clip_support(t, mapq_min, min_clip, w)
            cl, _ = t.fetch(abi.STAGE_CLUSTERS)
            assert np.array_equal(cl, before)  # the call changes nothing a fetch returns
            assert_rows_equal(got, expected_clip_support(cl, cols, mapq_min, min_clip, w), cl)
            assert not got["at"][(cl["flags"] & 2) == 0].any()
    if name == "clipped":
        voted = (before["flags"] & 2) != 0
        got = t.clip_support(t, QUAL, 10, w)
        assert voted.any() and (~voted).any() and got["events"][voted].any() and got["events"][~voted].any()
        assert int(got["events"].sum()) > 100 and int(got["peak_n"].max()) >= 2
    t.close()


# ---- 2. one call, hand-placed records; 3. wide and deep windows -----------------------------------------------------------------
HAND_CONTIGS = [("chr1", 2_000_000), ("chr2", 6_000), ("chr3", 2_000_000), ("chr4", 2_000_000)]
E1, E2 = 5_530, 700_030   # the main call: chr3:E1 (side 1) and chr4:E2 (side 2)
HAND_W = 1000.5           # W = 1000
WIDE_W = 20000.5          # W = 20 000: every window spans many tiles
P1_MIN = P1_MAX = E1 - 229                      # side 1 of the main call: its pairs' reads on chr3 all start here (1-based), whichever of them the clustering keeps
LO, HI = P1_MIN - 1000, P1_MAX + 1000           # its window at HAND_W
WIDE_LO, WIDE_HI = 1, P1_MAX + 20000            # ... at WIDE_W (clamped at 1); tile k of the kernel's walk begins at 1 + k * CLIP_TILE
TILE3, TILE8 = WIDE_LO + 3 * CLIP_TILE, WIDE_LO + 8 * CLIP_TILE
DEEP_P, DEEP_N = E2 + 100, 20_000               # 20 000 reads clipped at one position on side 2
F_LEFT, F_RIGHT = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80


def hand_records():
    """name -> (records, (events LEFT, events RIGHT, at LEFT, at RIGHT) they add to side 1 of the main call at min_clip 10, mapq_min 20,
    W 1000).  trail(p) is a read whose aligned bases end at 1-based p, lead(p) one whose aligned bases begin there."""
    R = synth.Rec
    h = {}

    def add(name, contrib, pos, cigar, flag=F_LEFT, mapq=60, tid=2, sa="", n=1):
        h[name] = ([R("H_%s_%d" % (name, k), flag, tid, pos, mapq, cigar, tid, pos + 200, 300, sa=sa) for k in range(n)], contrib)

    def trail(name, contrib, p, cigar="60M40S", reflen=60, **kw):
        add(name, contrib, p - reflen, cigar, **kw)

    def lead(name, contrib, p, cigar="40S60M", **kw):
        add(name, contrib, p - 1, cigar, **kw)

    trail("clip_min", (1, 0, 0, 0), E1 - 500, "90M10S", 90)
    trail("clip_min_less", (0, 0, 0, 0), E1 - 501, "91M9S", 91)
    lead("lead_min", (0, 1, 0, 0), E1 - 502, "10S90M")
    lead("lead_min_less", (0, 0, 0, 0), E1 - 503, "9S91M")
    lead("lead_at_lo", (0, 1, 0, 0), LO)
    lead("lead_before_lo", (0, 0, 0, 0), LO - 1)
    lead("lead_at_hi", (0, 1, 0, 0), HI)
    lead("lead_behind_hi", (0, 0, 0, 0), HI + 1)
    trail("trail_at_lo", (1, 0, 0, 0), LO)             # the record starts 60 bases left of the window
    trail("trail_before_lo", (0, 0, 0, 0), LO - 1)
    trail("trail_at_hi", (1, 0, 0, 0), HI)
    trail("trail_behind_hi", (0, 0, 0, 0), HI + 1)     # the record starts inside the window, its end lies beyond it
    trail("trail_exact_p2", (1, 0, 1, 0), E1 + 2)
    trail("trail_exact_m2", (1, 0, 1, 0), E1 - 2)
    trail("trail_exact_p3", (1, 0, 0, 0), E1 + 3)
    trail("trail_exact_m3", (1, 0, 0, 0), E1 - 3)
    lead("lead_exact_p2", (0, 1, 0, 1), E1 + 2)
    lead("lead_exact_m2", (0, 1, 0, 1), E1 - 2)
    lead("lead_exact_p3", (0, 1, 0, 0), E1 + 3)
    lead("lead_exact_m3", (0, 1, 0, 0), E1 - 3)
    lead("hard_lead", (0, 1, 0, 0), E1 - 400, "5H20S75M")
    trail("hard_trail", (1, 0, 0, 0), E1 - 401, "75M20S5H", 75)
    add("both_ends", (1, 1, 0, 0), E1 - 701, "20S60M20S")   # leading at E1 - 700, trailing at E1 - 641
    add("only_clip", (0, 0, 0, 0), E1 - 300, "100S")
    add("no_cigar", (0, 0, 0, 0), E1 - 300, "*")
    for bit in (0x4, 0x100, 0x200, 0x400, 0x800):
        trail("flag_%x" % bit, (0, 0, 0, 0), E1 - 200, flag=F_LEFT | bit)
    trail("unpaired", (1, 0, 0, 0), E1 - 210, flag=0)
    trail("mapq_19", (0, 0, 0, 0), E1 - 220, mapq=19)
    trail("mapq_20", (1, 0, 0, 0), E1 - 221, mapq=20)
    trail("with_sa", (0, 0, 0, 0), E1 - 230, sa="chr1,100,+,60S40M,60,0;")
    trail("skip", (1, 0, 0, 0), E1 - 100, "30M200N30M20S", 260)
    trail("deletion", (1, 0, 0, 0), E1 - 90, "40M5D40M20S", 85)
    trail("other_contig", (0, 0, 0, 0), E1, tid=1)     # the same numbers on the contig before
    lead("other_contig_b", (0, 0, 0, 0), E1, tid=1)
    trail("tie_low", (3, 0, 0, 0), E1 - 800, n=3)      # LEFT: three reads each at two positions - the smaller one is the peak
    trail("tie_high", (3, 0, 0, 0), E1 - 750, n=3)
    lead("right_pile", (0, 5, 0, 0), E1 - 799, n=5)    # RIGHT: a larger pile one base further on - the directions are kept apart
    # outside the window at W 1000, inside at W 20 000: either side of a tile boundary of the wide walk and exactly on it, and a pile
    # whose records begin in the tile before
    lead("tile_last", (0, 0, 0, 0), TILE3 - 1)
    lead("tile_first", (0, 0, 0, 0), TILE3, n=2)
    lead("tile_second", (0, 0, 0, 0), TILE3 + 1)
    trail("tile_last_t", (0, 0, 0, 0), TILE3 - 1)
    trail("tile_first_t", (0, 0, 0, 0), TILE3)
    trail("tile_pile", (0, 0, 0, 0), TILE8 + 10, n=4)
    lead("clamp", (0, 0, 0, 0), 1, tid=3)              # chr4:1, inside the window of the second call, whose lower bound is clamped
    return h


def hand_dataset(seed=5):
    """Background (no clipped read) on the three long contigs; the main call chr3:E1 / chr4:E2 with the hand-placed records around E1
    and DEEP_N unpaired reads clipped at DEEP_P on its other side; a second call chr1:900 030 / chr4:5, whose side 2 has
    p2_min - W < 1."""
    rng = np.random.default_rng(seed)
    names = [n for n, _ in HAND_CONTIGS]
    ds = synth.Dataset(list(HAND_CONTIGS))
    for i in range(6000):
        t = (0, 2, 3)[int(rng.integers(0, 3))]
        ds.recs += synth._proper_pair(rng, i, t, 30_000, 1_999_000, 100, 350, 40)
    for j in range(14):
        ds.recs += synth._discordant_pair("mD_%d" % j, 2, E1 - 230, 3, E2 - 30 + int(rng.integers(40, 300)), 100, False, True)
        ds.recs += synth._discordant_pair("zD_%d" % j, 0, 900_000 - int(rng.integers(80, 300)), 3, 5 + int(rng.integers(40, 300)), 100, False, True)
    for j in range(6):
        ds.recs += synth._split_pair("mS_%d" % j, names, 2, E1, 3, E2, 60, 40)
        ds.recs += synth._split_pair("zS_%d" % j, names, 0, 900_030, 3, 5, 60, 40)
    ds.recs += [synth.Rec("deep%d" % j, 0, 3, DEEP_P - 60, 60, "60M40S", -1, -1, 0) for j in range(DEEP_N)]
    for recs, _ in hand_records().values():
        ds.recs += recs
    ds.sort()
    return ds


def hand():
    if "hand" not in _SHARED:
        ds = hand_dataset()
        _SHARED["hand"] = (ds, ds.to_soa())
    return _SHARED["hand"]


def hand_context(fast):
    ds, cols = hand()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    main = [i for i, c in enumerate(cl) if c["flags"] & 2 and (c["p1_tid"], int(c["p1_exact"]), c["p2_tid"], int(c["p2_exact"])) == (2, E1, 3, E2)]
    low = [i for i, c in enumerate(cl) if c["flags"] & 2 and (c["p1_tid"], int(c["p1_exact"]), c["p2_tid"], int(c["p2_exact"])) == (0, 900_030, 3, 5)]
    assert len(main) == 1 and len(low) == 1, cl
    assert (int(cl[main[0]]["p1_min"]), int(cl[main[0]]["p1_max"])) == (P1_MIN, P1_MAX)  # what LO and HI were worked out from
    return t, cols, w, cl, main[0], low[0]


@pytest.mark.parametrize("fast", [True, False])
def test_clip_support_hand_placed_records(fast):
    t, cols, w, cl, main, low = hand_context(fast)
    table = hand_records()
    # the numpy definition itself against the hand-written truth of every placed record
    ds = hand()[0]
    idx = {}
    for i, r in enumerate(ds.recs):
        idx.setdefault(r.qname, []).append(i)
    one = cl[main:main + 1]
    for name, (recs, contrib) in table.items():
        rows = sorted(i for r in recs for i in idx[r.qname])
        sub = filtered(cols, np.isin(np.arange(len(cols["tid"])), rows))
        v = expected_clip_support(one, sub, QUAL, 10, HAND_W)[0]
        assert (int(v["events"][0][LEFT]), int(v["events"][0][RIGHT]), int(v["at"][0][LEFT]), int(v["at"][0][RIGHT])) == contrib, name
    for min_clip in (9, 10, 41):
        for mapq_min in (0, 20):
            for ww in (HAND_W, w):
                got = t.clip_support(t, mapq_min, min_clip, ww)
                assert_rows_equal(got, expected_clip_support(cl, cols, mapq_min, min_clip, ww), cl)
    got = t.clip_support(t, QUAL, 10, HAND_W)
    m = got[main]
    total = [sum(v[1][k] for v in table.values()) for k in range(4)]
    assert [int(m["events"][0][LEFT]), int(m["events"][0][RIGHT]), int(m["at"][0][LEFT]), int(m["at"][0][RIGHT])] == total  # the background has no clipped read
    assert (int(m["peak_pos"][0][LEFT]), int(m["peak_n"][0][LEFT])) == (E1 - 800, 3)    # the tie: the smaller position
    assert (int(m["peak_pos"][0][RIGHT]), int(m["peak_n"][0][RIGHT])) == (E1 - 799, 5)  # kept apart from the LEFT pile beside it
    z = got[low]
    assert int(cl[low]["p2_min"]) < 1000 and int(z["events"][1][RIGHT]) == 1 and int(z["peak_pos"][1][RIGHT]) == 1  # the clamp: chr4:1 is in
    t.close()


@pytest.mark.parametrize("fast", [True, False])
def test_clip_support_wide_and_deep_windows(fast):
    t, cols, w, cl, main, low = hand_context(fast)
    assert (WIDE_HI - WIDE_LO) // CLIP_TILE >= 20 and LO > TILE3 + 1 and TILE8 + 10 > HI
    for mapq_min in (0, 20):
        got = t.clip_support(t, mapq_min, 10, WIDE_W)
        assert_rows_equal(got, expected_clip_support(cl, cols, mapq_min, 10, WIDE_W), cl)
    narrow = t.clip_support(t, QUAL, 10, HAND_W)[main]
    m = got[main]
    # the six reads around the tile boundary, the pile of four behind it, and the four just outside the narrow window
    assert int(m["events"][0][RIGHT]) == int(narrow["events"][0][RIGHT]) + 4 + 2
    assert int(m["events"][0][LEFT]) == int(narrow["events"][0][LEFT]) + 2 + 4 + 2
    assert (int(m["peak_pos"][0][LEFT]), int(m["peak_n"][0][LEFT])) == (TILE8 + 10, 4)
    assert np.array_equal(m["at"], narrow["at"])
    # the deep pile: far more than 255 reads at one position, several steps of the record loop
    for row in (m, narrow):
        assert (int(row["peak_pos"][1][LEFT]), int(row["peak_n"][1][LEFT]), int(row["events"][1][LEFT])) == (DEEP_P, DEEP_N, DEEP_N)
    t.close()


# ---- 4. designed truth ----------------------------------------------------------------------------------------------------------
DIR = {"L": LEFT, "R": RIGHT}


@pytest.mark.parametrize("fast", [True, False])
def test_designed_loci_counted_and_rescued(fast):
    ds, cols = dataset("designed")
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    sup = t.clip_support(t, QUAL, 10, w)
    jn = t.junctions()
    assert_rows_equal(sup, expected_clip_support(cl, cols, QUAL, 10, w), cl)
    seen = {}
    for c, j, s in zip(cl, jn, sup):
        L, a_first = kc.locus_of(c)
        if L is None:
            continue
        name, ta, bpa, da, tb, bpb, db = L
        assert name not in seen, name
        bp = (bpa, bpb) if a_first else (bpb, bpa)
        d = (DIR[da], DIR[db]) if a_first else (DIR[db], DIR[da])
        assert capi.junction_sides(j)[:2] == d, (name, j)
        n = kc.CLIP_READS[name][:2] if a_first else kc.CLIP_READS[name][1::-1]
        along = kc.CLIP_READS[name][2]
        r3, r2 = capi.clip_rescue(c, j, s, 3), capi.clip_rescue(c, j, s, 2)
        assert r3 == kc.expected_rescue(c, j, s, 3) and r2 == kc.expected_rescue(c, j, s, 2)
        seen[name] = (bool(c["flags"] & 2), r3, r2)
        for side in (0, 1):
            dd = d[side] if along else 1 - d[side]
            assert int(s["peak_n"][side][dd]) == n[side], (name, side, s)
            assert int(s["peak_pos"][side][dd]) == (bp[side] if n[side] else 0), (name, side, s)
            assert int(s["peak_n"][side][1 - dd]) == 0, (name, side, s)  # the background has no clipped read
        if name == "a":
            assert (int(c["p1_exact"]), int(c["p2_exact"])) == bp and int(c["n_sr"]) == 8
            assert [int(s["at"][side][d[side]]) for side in (0, 1)] == [5, 5]
        if name in ("b", "f"):
            assert (r2[0], r2[1]) == bp
    assert set(seen) == {L[0] for L in kc.CLIP_LOCI}, seen
    assert seen["a"] == (True, None, None)
    assert seen["b"] == (False, seen["b"][1], seen["b"][1]) and seen["b"][1][2:] == (6, 6)
    assert seen["c"] == (False, None, None) and seen["d"] == (False, None, None) and seen["e"] == (False, None, None)
    assert seen["f"][:2] == (False, None) and seen["f"][2][2:] == (2, 2)
    t.close()


# ---- 5. bk_base_depth -----------------------------------------------------------------------------------------------------------
def test_base_depth_at_calls_and_at_arbitrary_positions():
    ds, cols = dataset("clipped")
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_isize_stats"):
        t.base_depth([0], [1000])
    w, n_valid = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    v = cl[(cl["flags"] & 2) != 0]
    assert len(v) >= 3
    assert np.array_equal(t.base_depth(v["p1_tid"], v["p1_exact"]), v["depth1"]) and v["depth1"].any()
    assert np.array_equal(t.base_depth(v["p2_tid"], v["p2_exact"].astype(np.uint32)), v["depth2"])
    rng = np.random.default_rng(77)
    n = 300
    tid = rng.integers(-1, 4, n).astype(np.int32)
    pos = rng.integers(1, 2_000_000, n).astype(np.uint32)
    hot = rng.integers(0, len(kc.CLIPPED_LOCI), n // 2)  # half of them around the loci, where reads pile up
    tid[:n // 2] = [kc.CLIPPED_LOCI[k][0] for k in hot]
    pos[:n // 2] = [kc.CLIPPED_LOCI[k][1] + int(d) for k, d in zip(hot, rng.integers(-500, 500, n // 2))]
    tid[-4:], pos[-4:] = (0, 0, 3, 3), (0, 1, 2_000_000, 2 ** 32 - 1)
    endpos = rec_endpos(cols)
    exp = np.asarray([single_base_depth(cols, endpos, int(a), int(b)) for a, b in zip(tid, pos)], np.uint32)
    got = t.base_depth(tid, pos)
    assert got.dtype == np.uint32 and np.array_equal(got, exp), np.nonzero(got != exp)[0][:5]
    assert exp.max() > 10 and not got[tid < 0].any()
    assert len(t.base_depth([], [])) == 0
    assert np.array_equal(cl, t.fetch(abi.STAGE_CLUSTERS)[0])
    t.close()


# ---- 6. table forms and the normal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "exclude_host", "exclude_device", "feed_ctx"])
def test_clip_support_table_forms(form):
    ds, cols = dataset("clipped")
    if form == "feed_ctx":
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "t.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        t, hold = make_ctx(ds.contigs, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            assert t.exclude_regions(*EXCLUDE) > 0
            cols = filtered(cols, ~cc.excluded_mask(cols, *EXCLUDE))
    w, n_valid = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert n_valid > 0
    for min_clip, mapq_min in ((10, 20), (1, 0)):
        got = t.clip_support(t, mapq_min, min_clip, w)
        assert_rows_equal(got, expected_clip_support(cl, cols, mapq_min, min_clip, w), cl)
    assert got["events"].any()
    t.close()
    if form == "feed_ctx":
        hold.close()
    del hold


def test_clip_support_device_table_with_side_rows():
    """BK_MEM_DEVICE: a table generated in HBM with bk_side rows"""
    import torch
    from breakid_amd import synth_gpu
    contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
    cols = synth_gpu.to_numpy_cols(dcols)
    assert "side" in dcols
    t = capi.Context(contigs)
    t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
    w, n_valid = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert n_valid > 0
    for min_clip, mapq_min in ((10, 20), (1, 0)):
        got = t.clip_support(t, mapq_min, min_clip, w)
        assert_rows_equal(got, expected_clip_support(cl, cols, mapq_min, min_clip, w), cl)
    t.close()
    del dcols


def test_clip_support_of_the_normal_and_errors():
    ds, cols = dataset("clipped")
    nor = kc.clipped_tumor(seed=31, n_background=6000, n_local=150)
    ncols = nor.to_soa()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints") as e:
        t.clip_support(t, QUAL, 10, 1000.0)
    assert e.value.code == abi.BK_ERR_ARG
    w, _ = t.run(qual=QUAL, fast=True)
    n = capi.Context(nor.contigs)
    n.upload(ncols)
    with pytest.raises(capi.BreakIDError, match="bk_isize_stats on the records context"):
        t.clip_support(n, QUAL, 10, w)
    n.isize_stats()
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    for min_clip, mapq_min in ((10, 20), (1, 0), (25, 20)):
        got = t.clip_support(n, mapq_min, min_clip, w)
        assert_rows_equal(got, expected_clip_support(cl, ncols, mapq_min, min_clip, w), cl)
    assert got["events"].any()
    own = t.clip_support(t, QUAL, 10, w)  # the rows of the call before are gone; these are the tumour's own again
    assert_rows_equal(own, expected_clip_support(cl, cols, QUAL, 10, w), cl)
    for bad, msg in (((QUAL, 0, w), "min_clip must be at least 1"), ((-1, 10, w), "mapq_min must not be negative"), ((QUAL, 10, -1.0), "w is out of range")):
        with pytest.raises(capi.BreakIDError, match=msg) as e:
            t.clip_support(n, *bad)
        assert e.value.code == abi.BK_ERR_ARG
    o = capi.Context([(name, ln + 1) for name, ln in ds.contigs])
    o.upload(cols)
    o.isize_stats()
    with pytest.raises(capi.BreakIDError, match="reference lists differ"):
        t.clip_support(o, QUAL, 10, w)
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts"):
        t.clip_support(s, QUAL, 10, w)
    with pytest.raises(capi.BreakIDError, match="sharded contexts"):
        s.clip_support(t, QUAL, 10, w)
    assert np.array_equal(cl, t.fetch(abi.STAGE_CLUSTERS)[0])
    for c in (t, n, o, s):
        c.close()


# ---- 7. command line ------------------------------------------------------------------------------------------------------------
C_COLS = ["Clip1", "Clip2", "ClipPeak1", "ClipPeakN1", "ClipPeak2", "ClipPeakN2", "ClipBg1", "ClipBg2"]


def clip_fields(j, s, normal=None):
    d = capi.junction_sides(j)[:2]
    f = [s["at"][0][d[0]], s["at"][1][d[1]], s["peak_pos"][0][d[0]], s["peak_n"][0][d[0]], s["peak_pos"][1][d[1]], s["peak_n"][1][d[1]], s["events"][0][d[0]],
         s["events"][1][d[1]]]
    if normal is not None:
        f += [normal["at"][0][d[0]], normal["at"][1][d[1]]]
    return [str(int(x)) for x in f]


def run_cli(args, env):
    r = subprocess.run([BIN] + args, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.mark.parametrize("with_normal", [False, True])
def test_cli_clip_files(with_normal):
    ds, cols = dataset("designed")
    names = [nm for nm, _ in ds.contigs]
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        write_indexed(ds, tb)
        side = synth.write_side_files(ds, tmp, refgene_lines=designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        extra = ["-all", "-fast", "-vcf", "-evidence"]
        ncols = None
        if with_normal:
            nor = kc.clipped_tumor(seed=31, n_background=4000, n_local=100)
            ncols = nor.to_soa()
            nor.write_bam(nb, aligned=True)
            extra += ["-normal", nb]
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b, b2, c = (os.path.join(tmp, x) for x in "abdc")
        run_cli(base[1:] + ["-o", a], env)
        r = run_cli(base[1:] + ["-o", b, "-clip"], env)
        run_cli(base[1:] + ["-o", b2, "-clip"], env)
        # every file that a run without -clip writes is byte-identical
        same = ["_fusion.txt", "_fusion_all.txt", "_fusion.vcf", "_evidence.txt", "_evidence.bam"] + (["_fusion_normal.txt", "_fusion_all_normal.txt"] if with_normal else [])
        for suffix in same:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
        pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
        assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "clip_min_length\t10\nclip_min_support\t3\n", (pa, pb)
        fa, fb = open(a + "_performance.txt").read().split("\n"), open(b + "_performance.txt").read().split("\n")
        assert fa[0] == fb[0] and fa[1].split("\t")[:5] == fb[1].split("\t")[:5]
        new = ["_fusion_clip.txt", "_fusion_all_clip.txt", "_fusion_rescued.txt"]
        assert not any(os.path.exists(a + s) for s in new)
        for suffix in new + same:  # two runs: the same bytes
            assert open(b + suffix, "rb").read() == open(b2 + suffix, "rb").read(), suffix
        # the same values through the C ABI
        t = capi.Context(ds.contigs)
        t.upload(cols)
        w, _ = t.run(qual=QUAL, fast=True)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        sup, jn = t.clip_support(t, QUAL, 10, w), t.junctions()
        nsup = [None] * len(cl)
        if with_normal:
            n = capi.Context(ds.contigs)
            n.upload(ncols)
            n.isize_stats()
            nsup = t.clip_support(n, QUAL, 10, w)
            n.close()
        by_call, rescued3, rescued2 = {}, {}, {}
        q_tid, q_pos = [], []
        for i, cr in enumerate(cl):
            f = clip_fields(jn[i], sup[i], nsup[i])
            if cr["flags"] & 2:
                key = (names[cr["p1_tid"]] + ":%d" % cr["p1_exact"], names[cr["p2_tid"]] + ":%d" % cr["p2_exact"], str(cr["n_drp"]), str(cr["n_sr"]))
                by_call.setdefault(key, []).append(f)
            for support, out in ((3, rescued3), (2, rescued2)):
                res = capi.clip_rescue(cr, jn[i], sup[i], support)
                if res:
                    out[(names[cr["p1_tid"]] + ":%d" % res[0], names[cr["p2_tid"]] + ":%d" % res[1])] = (f, int(cr["n_drp"]), int(cr["p1_tid"]), res[0], int(cr["p2_tid"]), res[1])
        header_tail = C_COLS + (["Normal_Clip1", "Normal_Clip2"] if with_normal else [])
        n_rows = 0
        for suffix in ("_fusion", "_fusion_all"):
            plain = open(b + suffix + ".txt").read().split("\n")
            twin = open(b + suffix + "_clip.txt").read().split("\n")
            assert len(plain) == len(twin) and twin[0] == plain[0] + "\t" + "\t".join(header_tail)
            for p, q in zip(plain[1:], twin[1:]):
                f = q.split("\t")
                assert "\t".join(f[:15]) == p
                if not p:
                    continue
                n_rows += 1
                cand = by_call[(f[1], f[2], f[7], f[8])]
                assert all(x == cand[0] for x in cand) and f[15:] == cand[0], (f, cand)
        assert n_rows >= 2  # locus a, in both files

        def check_rescued(path, want):
            lines = open(path).read().split("\n")
            assert lines[0] == plain[0] + "\t" + "\t".join(header_tail) and lines[-1] == ""
            rows = [l.split("\t") for l in lines[1:-1]]
            assert sorted((f[1], f[2]) for f in rows) == sorted(want), (rows, want)
            assert [int(f[7]) for f in rows] == sorted((int(f[7]) for f in rows), reverse=True)
            for f in rows:
                fields, n_drp, t1, p1, t2, p2 = want[(f[1], f[2])]
                d = t.base_depth([t1, t2], [p1, p2])
                assert f[7:13] == [str(n_drp), "0", "%g" % float(d[0]), "%g" % float(d[1]), "0", "0"] and f[15:] == fields, f
            return rows

        b_locus = ("chr1:600000", "chr3:500000")
        f_locus = ("chr2:300000", "chr4:900000")
        assert set(rescued3) == {b_locus} and set(rescued2) == {b_locus, f_locus}  # the designed positions
        check_rescued(b + "_fusion_rescued.txt", rescued3)
        assert "rescued cluster count: 1\n" in r.stdout
        # -clipsupport 2, and without -all: both loci have a gene on either side and pass the filters of _fusion.txt
        r = run_cli([x for x in base[1:] if x not in ("-all", "-vcf", "-evidence")] + ["-o", c, "-clip", "-clipsupport", "2", "-minclip", "12"], env)
        check_rescued(c + "_fusion_rescued.txt", rescued2)
        assert "rescued cluster count: 2\n" in r.stdout and not os.path.exists(c + "_fusion_all_clip.txt")
        assert open(c + "_params.txt").read().endswith("clip_min_length\t12\nclip_min_support\t2\n")
        t.close()
        # the options are checked before anything is read
        z = os.path.join(tmp, "z")
        for more, msg in ((["-clip", "-gpus", "2"], "-clip cannot be combined with -gpus"), (["-minclip", "12"], "need -clip"), (["-clipsupport", "2"], "need -clip"),
                          (["-clip", "-minclip", "0"], "must be numbers from 1"), (["-clip", "-clipsupport", "0"], "must be numbers from 1")):
            rr = subprocess.run([BIN, "-i", tb, "-n", side["nib"], "-o", z] + more, env=env, capture_output=True, text=True)
            assert rr.returncode == 1 and msg in rr.stderr, rr.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))


def test_cli_clip_quiet_sample():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "q")
        r = run_cli(["-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast", "-clip"], env)
        assert "rescued cluster count: 0\n" in r.stdout
        plain = open(prefix + "_fusion.txt").read()
        assert plain.count("\n") == 1
        for suffix in ("_fusion_clip.txt", "_fusion_all_clip.txt", "_fusion_rescued.txt"):
            assert open(prefix + suffix).read() == plain[:-1] + "\t" + "\t".join(C_COLS) + "\n", suffix

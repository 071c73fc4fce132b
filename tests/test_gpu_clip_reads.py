"""The clipped reads at a site (`bk_clip_reads`) and the rescued clusters downstream of `-clip` (`_fusion_rescued_normal.txt`,
`_fusion_rescued.vcf`, `_evidence_rescued.txt` / `.bam`): counts, rows and offsets byte for byte against the numpy definition
(tests/clipreadcases.py) at every site; the two identities with bk_clip_support on the device result; hand-placed records on either
side of every clause and of every path of the kernels; every table form a context can hold; the errors; the command line."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import clipcases as kc
from tests import clipreadcases as rc
from tests.callcases import BIN, QUAL, EXCLUDE, designed_refgene, filtered, make_ctx, write_indexed
from tests.clipcases import LEFT, RIGHT
from tests.clipreadcases import as_sites, assert_clip_reads_equal, expected_clip_reads

pytestmark = pytest.mark.gpu

_SHARED = {}


def dataset(name):
    if name not in _SHARED:
        ds = {"clipped": kc.clipped_tumor, "designed": kc.clip_tumor}[name]()
        _SHARED[name] = (ds, ds.to_soa())
    return _SHARED[name]


def check(t, cols, sites, mapq_min, min_clip):
    """the listing call against the definition, and the counts-only call against the listing"""
    got = t.clip_reads(sites, mapq_min, min_clip)
    assert_clip_reads_equal(got, expected_clip_reads(cols, sites, mapq_min, min_clip))
    only = t.clip_reads(sites, mapq_min, min_clip, listing=False)
    assert only.dtype == np.uint32 and np.array_equal(only, got[0])
    return got


# ---- 1. the definition and the two identities on seeded data ----------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("name", ["designed", "clipped"])
def test_clip_reads_equal_their_definition_and_clip_support(name, fast):
    ds, cols = dataset(name)
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    voted = (cl["flags"] & 2) != 0
    assert voted.any() and (~voted).any()
    for mapq_min, min_clip in ((QUAL, 10), (0, 1), (QUAL, 25)):
        sup = t.clip_support(t, mapq_min, min_clip, w)
        sites, want = rc.identity_sites(cl, sup)
        assert len(sites) == 4 * len(cl) + 4 * int(voted.sum())
        counts, rows, off = check(t, cols, sites, mapq_min, min_clip)
        assert np.array_equal(counts, want), np.nonzero(counts != want)[0][:5]  # both identities, on the device result
        assert counts.any() and int(off[-1]) == len(rows) == int(counts.sum())
        assert np.array_equal(cl, t.fetch(abi.STAGE_CLUSTERS)[0])
    t.close()


# ---- 2. hand-placed records -----------------------------------------------------------------------------------------------------
HAND_CONTIGS = [("chrA", 2_000_000), ("chrB", 6_000), ("chrC", 100_000)]
P0 = 500_000       # the pile
Q0 = 520_000       # the tolerance site, tol 3
B0 = 540_000       # the record with a clip on both ends
LONG = 560_000     # where the spliced read's trailing clip lies, maxspan bases behind its start
MAXSPAN = 5100     # 50M5000N50M: the longest alignment of the table
F1, F2 = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80
CLIP_STEPS = 4     # breakid_amd/csrc/clip.hip: 64-record steps in flight per trip of the record loop


def hand_dataset():
    R = synth.Rec
    rng = np.random.default_rng(9)
    ds = synth.Dataset(list(HAND_CONTIGS))
    for i in range(3000):  # unclipped background: the ranges the kernels walk are long and of every length
        ds.recs += synth._proper_pair(rng, i, 0, 440_000, 600_000, 100, 350, 40)

    def add(name, tid, pos, cigar, flag=F1, mapq=60, sa="", n=1):
        ds.recs.extend(R("H_%s_%d" % (name, k), flag, tid, pos, mapq, cigar, tid, pos + 200, 300, sa=sa) for k in range(n))

    def trail(name, p, cigar="60M40S", reflen=60, tid=0, **kw):  # aligned bases end at 1-based p
        add(name, tid, p - reflen, cigar, **kw)

    def lead(name, p, cigar="40S60M", tid=0, **kw):              # aligned bases begin at 1-based p
        add(name, tid, p - 1, cigar, **kw)

    trail("pile", P0, n=150)                       # more than two 64-record steps at one position
    lead("pile_right", P0, n=3)                    # the other direction at the same position
    trail("hard_trail", P0, "80M12S5H", 80)
    lead("hard_lead", P0, "5H12S80M")
    trail("short", P0, "91M9S", 91)                # min_clip - 1 bases
    trail("with_sa", P0, sa="chr1,100,+,60S40M,60,0;")
    trail("dup", P0, flag=F1 | 0x400)
    trail("mapq_19", P0, mapq=19)
    lead("no_ref", P0, "40S60I")                   # a leading clip on a record without reference length
    add("only_clip", 0, P0 - 1, "100S")
    for d in (-4, -3, 3, 4):                       # pos +- tol exactly, and one further
        trail("tol_t%+d" % d, Q0 + d)
        lead("tol_l%+d" % d, Q0 + d)
    add("both", 0, B0 - 1, "20S60M20S")            # leading at B0 (clip 20), trailing at B0 + 59 (clip 20)
    add("both_uneven", 0, B0 - 1, "15S60M25S")     # the same two events with clips of 15 and 25
    trail("long", LONG, "50M5000N50M20S", MAXSPAN)  # starts maxspan before the site
    lead("first_base", 1)                          # chrA:1
    lead("sixth_base", 6)
    lead("seventh_base", 7)
    trail("other_contig", P0, tid=1)
    trail("last", 50_000, tid=2, n=2)              # the last records of the last contig
    lead("last_lead", 49_990, tid=2)
    ds.sort()
    return ds


def hand():
    if "hand" not in _SHARED:
        ds = hand_dataset()
        _SHARED["hand"] = (ds, ds.to_soa())
    return _SHARED["hand"]


HAND_SITES = [
    # descending positions on chrA
    (0, LONG, 0, LEFT), (0, B0 + 59, 0, LEFT), (0, B0, 0, RIGHT), (0, B0, 0, LEFT), (0, Q0, 3, LEFT), (0, Q0, 3, RIGHT), (0, Q0, 4, LEFT), (0, Q0, 2, RIGHT),
    (0, P0, 0, LEFT), (0, P0, 0, RIGHT), (0, P0, 0, LEFT),  # two identical sites
    (0, P0 + 1, 2, LEFT), (0, P0 - 2, 2, LEFT), (0, P0 - 3, 2, LEFT),  # overlapping ones, and one that just misses
    (0, 1, 5, RIGHT), (0, 1, 0, RIGHT), (0, 1, 5, LEFT),
    (-1, P0, 0, LEFT), (7, P0, 0, LEFT), (1, P0, 0, LEFT), (1, P0, 0, RIGHT),
    (2, 50_000, 0, LEFT), (2, 90_000, 10, LEFT), (2, 90_000, 2 ** 32 - 1, LEFT), (2, 2 ** 32 - 1, 2 ** 32 - 1, RIGHT), (2, 49_990, 0, RIGHT),
    (0, P0, 2 ** 31, LEFT), (0, 0, 0, RIGHT),
]
# what they count at mapq_min 20, min_clip 10, by hand: the pile is 150 + hard_trail; short, with_sa, dup, mapq_19 and no_ref give nothing
HAND_COUNTS = [1, 2, 2, 0, 2, 2, 4, 0,
               151, 4, 151,
               151, 151, 0,
               2, 1, 0,
               0, 0, 1, 0,
               2, 0, 2, 1, 1,
               None, 0]


def hand_context():
    ds, cols = hand()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.isize_stats()
    return t, ds, cols


def test_clip_reads_hand_placed_records():
    t, ds, cols = hand_context()
    sites = as_sites(HAND_SITES)
    # the numpy definition itself against the hand-written counts
    exp = expected_clip_reads(cols, sites, QUAL, 10)
    for k, n in enumerate(HAND_COUNTS):
        assert n is None or int(exp[0][k]) == n, (k, HAND_SITES[k], int(exp[0][k]), n)
    all_left = kc.clip_events(cols, QUAL, 10)
    assert int(exp[0][26]) == int(((all_left[0] == 0) & (all_left[2] == LEFT)).sum())  # tol 2^31: the whole contig
    names = lambda rows: sorted(ds.recs[int(r["rec"])].qname for r in rows)
    rows = lambda k: exp[1][int(exp[2][k]):int(exp[2][k + 1])]
    assert names(rows(8)) == sorted(["H_pile_%d" % j for j in range(150)] + ["H_hard_trail_0"])
    assert names(rows(9)) == sorted(["H_pile_right_%d" % j for j in range(3)] + ["H_hard_lead_0"])
    assert sorted(rows(2)["clip_len"].tolist()) == [15, 20] and sorted(rows(1)["clip_len"].tolist()) == [20, 25]  # one record, two sites, two lengths
    assert set(rows(2)["rec"].tolist()) == set(rows(1)["rec"].tolist())
    assert names(rows(0)) == ["H_long_0"] and int(cols["pos"][int(rows(0)["rec"][0])]) == LONG - MAXSPAN
    assert 12 in rows(8)["clip_len"].tolist() and 12 in rows(9)["clip_len"].tolist()  # the S op behind and before the H
    # the ranges the kernels walk: longer than two steps of 64 at the pile, no multiple of a trip, and one shorter than 64
    pos, tid = cols["pos"].astype(np.int64), cols["tid"]
    rng_len = lambda T, p, tol: int(((tid == T) & (pos >= p - tol - 1 - MAXSPAN) & (pos < p + tol)).sum())
    assert rng_len(0, P0, 0) > 64 * CLIP_STEPS and rng_len(0, P0, 0) % (64 * CLIP_STEPS) != 0 and 0 < rng_len(2, 50_000, 0) < 64
    assert int(np.count_nonzero(pos[tid == 0] == P0 - 60)) >= 150 + 3  # one position: the pile spans more than two steps of 64 lanes
    # the device
    for mapq_min, min_clip in ((QUAL, 10), (QUAL, 9), (19, 10), (0, 1), (QUAL, 13), (QUAL, 41)):
        got = check(t, cols, sites, mapq_min, min_clip)
    got = check(t, cols, sites, QUAL, 10)
    assert [int(x) for x in got[0][:26]] == HAND_COUNTS[:26]
    assert int(check(t, cols, sites, QUAL, 9)[0][8]) == 152 and int(check(t, cols, sites, 19, 10)[0][8]) == 152  # the short clip, the low mapq
    # every site on its own, and all of them reversed: a site's rows do not depend on its neighbours
    for k in (0, 8, 14, 23):
        one = t.clip_reads(sites[k:k + 1], QUAL, 10)
        assert one[2].tolist() == [0, int(got[0][k])] and np.array_equal(one[1]["rec"], got[1][int(got[2][k]):int(got[2][k + 1])]["rec"])
    check(t, cols, sites[::-1].copy(), QUAL, 10)
    # many sites: more than one workgroup, waves without a site in the last one
    many = as_sites([(0, P0 - 300 + j, j % 4, j % 2) for j in range(601)] + [(2, 49_000 + 7 * j, 3, j % 2) for j in range(201)])
    assert check(t, cols, many, QUAL, 10)[0].any()
    t.close()


# ---- 4. two calls, no site, no record --------------------------------------------------------------------------------------------
def test_clip_reads_twice_and_empty():
    t, ds, cols = hand_context()
    sites = as_sites(HAND_SITES)
    a = t.clip_reads(sites, QUAL, 10)
    b = t.clip_reads(sites, QUAL, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[1]) > 300
    counts, rows, off = t.clip_reads(as_sites([]), QUAL, 10)
    assert len(counts) == 0 and len(rows) == 0 and off.tolist() == [0] and rows.dtype == abi.CLIP_READ
    assert len(t.clip_reads(as_sites([]), QUAL, 10, listing=False)) == 0
    none = as_sites([(0, 10, 0, LEFT), (-1, 5, 5, RIGHT)])  # sites without an event: an empty listing
    counts, rows, off = t.clip_reads(none, QUAL, 10)
    assert counts.tolist() == [0, 0] and len(rows) == 0 and off.tolist() == [0, 0, 0]
    t.close()
    e = capi.Context(ds.contigs)
    empty = filtered(cols, np.zeros(len(cols["tid"]), bool))
    e.upload(empty)
    e.isize_stats()
    counts, rows, off = e.clip_reads(sites, QUAL, 10)
    assert not counts.any() and len(counts) == len(sites) and len(rows) == 0 and not off.any() and len(off) == len(sites) + 1
    assert not e.clip_reads(sites, QUAL, 10, listing=False).any()
    e.close()


# ---- 5. table forms --------------------------------------------------------------------------------------------------------------
def form_sites(t, w, cl):
    sup = t.clip_support(t, QUAL, 10, w)
    sites, want = rc.identity_sites(cl, sup)
    wide = sites.copy()
    wide["tol"] = 150
    return np.concatenate([sites, wide]), want


@pytest.mark.parametrize("form", ["host", "device", "host_no_qcheck", "device_no_qcheck", "exclude_host", "exclude_device", "feed_ctx"])
def test_clip_reads_table_forms(form):
    ds, cols = dataset("clipped")
    qcheck = not form.endswith("no_qcheck")
    if form == "feed_ctx":
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "t.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        t, hold = make_ctx(ds.contigs, cols, "device" if "device" in form else "host", qcheck=qcheck)
        if form.startswith("exclude"):
            assert t.exclude_regions(*EXCLUDE) > 0
            cols = filtered(cols, ~cc.excluded_mask(cols, *EXCLUDE))
    if not qcheck:
        cols = {k: v for k, v in cols.items() if k != "qcheck"}
    w, n_valid = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert n_valid > 0
    sites, want = form_sites(t, w, cl)
    counts, rows, off = check(t, cols, sites, QUAL, 10)
    assert np.array_equal(counts[:len(want)], want) and len(rows) > 100
    assert np.array_equal(rows["qhash"], cols["qhash"][rows["rec"]])
    if qcheck:
        assert np.array_equal(rows["qcheck"], cols["qcheck"][rows["rec"]]) and rows["qcheck"].all()
    else:
        assert not rows["qcheck"].any()
    t.close()
    if form == "feed_ctx":
        hold.close()
    del hold


def test_clip_reads_device_table_with_side_rows():
    """BK_MEM_DEVICE with bk_side rows: a listed row takes its hashes from the row, not from the columns (which hold zeros here)"""
    import torch
    from breakid_amd import synth_gpu
    ds, cols = dataset("clipped")
    dcols, ptrs = cc.to_device(cols)
    dcols["side"] = synth_gpu.side_rows(dcols)
    for k in ("qhash", "qcheck"):
        dcols[k] = torch.zeros_like(dcols[k])
    ptrs = abi.device_ptrs(dcols)
    assert ptrs["side"]
    t = capi.Context(ds.contigs)
    t.attach_device(ptrs, len(cols["tid"]), int(cols["cigar_off"][-1]), int(cols["aux_off"][-1]))
    t.isize_stats()
    tid, p, d = kc.clip_events(cols, QUAL, 10)  # sites at events all over the table
    pick = np.arange(0, len(tid), max(1, len(tid) // 300))
    sites = as_sites([(int(tid[i]), int(p[i]), 3, int(d[i])) for i in pick])
    counts, rows, off = check(t, cols, sites, QUAL, 10)
    assert counts.all() and len(rows) >= len(pick)
    assert np.array_equal(rows["qhash"], cols["qhash"][rows["rec"]]) and np.array_equal(rows["qcheck"], cols["qcheck"][rows["rec"]]) and rows["qhash"].all()
    t.close()
    del dcols


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_clip_reads_errors():
    import ctypes as C
    ds, cols = dataset("designed")
    sites = as_sites([(0, 600_000, 0, LEFT)])
    t = capi.Context(ds.contigs)
    t.upload(cols)

    def refused(ctx, msg, *args, **kw):
        with pytest.raises(capi.BreakIDError, match=msg) as e:
            ctx.clip_reads(*args, **kw)
        assert e.value.code == abi.BK_ERR_ARG

    refused(t, "bk_clip_reads: call bk_isize_stats first", sites, QUAL, 10)
    refused(t, "bk_clip_reads: call bk_isize_stats first", sites, QUAL, 10, listing=False)
    w, _ = t.run(qual=QUAL, fast=True)
    before = t.fetch(abi.STAGE_CLUSTERS)[0]
    refused(t, "min_clip must be at least 1", sites, QUAL, 0)
    refused(t, "mapq_min must not be negative", sites, -1, 10)
    refused(t, "site 1 has a dir above 1", as_sites([(0, 600_000, 0, LEFT), (0, 600_000, 0, 2)]), QUAL, 10)
    refused(t, "site 0 has a dir above 1", as_sites([(0, 600_000, 0, 2 ** 32 - 1)]), QUAL, 10, listing=False)
    counts, rows, off = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for kw in ((C.byref(rows), None), (None, C.byref(off))):
        with pytest.raises(capi.BreakIDError, match="rows and site_off go together") as e:
            t._check(t.L.bk_clip_reads(t.h, sites.ctypes.data, 1, QUAL, 10, C.byref(counts), *kw))
        assert e.value.code == abi.BK_ERR_ARG
    with pytest.raises(capi.BreakIDError, match="null counts") as e:
        t._check(t.L.bk_clip_reads(t.h, sites.ctypes.data, 1, QUAL, 10, None, C.byref(rows), C.byref(off)))
    assert e.value.code == abi.BK_ERR_ARG
    with pytest.raises(capi.BreakIDError, match="null sites") as e:
        t._check(t.L.bk_clip_reads(t.h, None, 1, QUAL, 10, C.byref(counts), C.byref(rows), C.byref(off)))
    assert e.value.code == abi.BK_ERR_ARG
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    refused(s, "sharded contexts", sites, QUAL, 10)
    assert np.array_equal(before, t.fetch(abi.STAGE_CLUSTERS)[0])
    assert t.clip_reads(sites, QUAL, 10)[0].tolist() == [6]  # and the context still answers
    assert np.array_equal(before, t.fetch(abi.STAGE_CLUSTERS)[0])
    t.close()
    s.close()


# ---- 7. a normal context ----------------------------------------------------------------------------------------------------------
def test_clip_reads_on_a_normal_context():
    ds, cols = dataset("clipped")
    nor = kc.clipped_tumor(seed=31, n_background=6000, n_local=150)
    ncols = nor.to_soa()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    sup, jn = t.clip_support(t, QUAL, 10, w), t.junctions()
    sites = []
    for c, j, s in zip(cl, jn, sup):
        res = capi.clip_rescue(c, j, s, 1)  # every unvoted cluster with a clip peak on both sides
        if res:
            d = capi.junction_sides(j)
            for tol in (2, 300):
                sites += [(int(c["p1_tid"]), res[0], tol, d[0]), (int(c["p2_tid"]), res[1], tol, d[1])]
    assert len(sites) >= 4
    sites = as_sites(sites)
    n = capi.Context(nor.contigs)
    n.upload(ncols)
    n.isize_stats()
    got = n.clip_reads(sites, QUAL, 10, listing=False)
    exp = expected_clip_reads(ncols, sites, QUAL, 10)
    assert got.dtype == np.uint32 and np.array_equal(got, exp[0]) and got.any()
    check(n, ncols, sites, QUAL, 10)
    assert not np.array_equal(got, t.clip_reads(sites, QUAL, 10, listing=False))  # the tumour's own reads are another matter
    t.close()
    n.close()


# ---- 8. command line --------------------------------------------------------------------------------------------------------------
def run_cli(args, env):
    r = subprocess.run([BIN] + args, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


EV_HEADER = "Call\tKind\tRead\tChr1\tPos1\tChr2\tPos2\tSides\tFlag1\tFlag2\tMapq1\tMapq2\tRecord\tClip"
B_LOCUS = ("chr1:600000", "chr3:500000")
F_LOCUS = ("chr2:300000", "chr4:900000")


def vcf_records(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = [l for l in lines[:-1] if l.startswith("#")]
    recs = [l.split("\t") for l in lines[:-1] if not l.startswith("#")]
    return head, recs


def info_of(f):
    return dict(x.split("=", 1) for x in f[7].split(";"))


@pytest.mark.parametrize("with_normal", [False, True])
def test_cli_rescued_files(with_normal):
    ds, cols = dataset("designed")
    names = [nm for nm, _ in ds.contigs]
    qnames = [r.qname for r in ds.recs]
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
        base = ["-i", tb, "-n", side["nib"]] + extra
        a, b, b2, c = (os.path.join(tmp, x) for x in "abdc")
        run_cli(base + ["-o", a], env)
        run_cli(base + ["-o", b, "-clip"], env)
        run_cli(base + ["-o", b2, "-clip"], env)
        # every file that a run without -clip writes is byte-identical, the new files are written only with -clip, twice the same
        same = ["_fusion.txt", "_fusion_all.txt", "_fusion.vcf", "_evidence.txt", "_evidence.bam"] + (["_fusion_normal.txt", "_fusion_all_normal.txt"] if with_normal else [])
        for suffix in same:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
        new = ["_fusion_rescued.vcf", "_evidence_rescued.txt", "_evidence_rescued.bam"] + (["_fusion_rescued_normal.txt"] if with_normal else [])
        assert not any(os.path.exists(a + s) for s in new + ["_fusion_rescued_normal.txt"])
        assert with_normal or not os.path.exists(b + "_fusion_rescued_normal.txt")
        for suffix in new + same + ["_fusion_rescued.txt", "_fusion_clip.txt", "_fusion_all_clip.txt"]:
            assert open(b + suffix, "rb").read() == open(b2 + suffix, "rb").read(), suffix
        assert open(b + "_params.txt").read() == open(a + "_params.txt").read().replace("out_file\t" + a, "out_file\t" + b) + "clip_min_length\t10\nclip_min_support\t3\n"
        # the same values through the C ABI
        t = capi.Context(ds.contigs)
        t.upload(cols)
        w, _ = t.run(qual=QUAL, fast=True)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        sup, jn = t.clip_support(t, QUAL, 10, w), t.junctions()
        ev, ev_off = t.evidence()
        n = nsup = None
        if with_normal:
            n = capi.Context(ds.contigs)
            n.upload(ncols)
            n.isize_stats()
            n.discordant_pairs(QUAL, w)
            n.split_evidence()
            nsup = t.normal_support(n, w)

        def rescued_calls(support):
            out = {}
            for i, cr in enumerate(cl):
                res = capi.clip_rescue(cr, jn[i], sup[i], support)
                if res:
                    out[(names[cr["p1_tid"]] + ":%d" % res[0], names[cr["p2_tid"]] + ":%d" % res[1])] = (i, res, capi.junction_sides(jn[i])[:2])
            return out

        def check_files(prefix, calls):
            rescued_rows = [l.split("\t") for l in open(prefix + "_fusion_rescued.txt").read().split("\n")[1:-1]]
            assert sorted((f[1], f[2]) for f in rescued_rows) == sorted(calls)
            # -- _fusion_rescued_normal.txt
            if with_normal:
                plain = open(prefix + "_fusion_rescued.txt").read().split("\n")
                twin = open(prefix + "_fusion_rescued_normal.txt").read().split("\n")
                assert len(twin) == len(plain) and twin[0] == plain[0] + "\tNormal_DRP\tNormal_ClipAt1\tNormal_ClipAt2\tNormal_Depth1\tNormal_Depth2" and twin[-1] == ""
                for p, q in zip(plain[1:-1], twin[1:-1]):
                    f = q.split("\t")
                    assert "\t".join(f[:-5]) == p
                    i, res, d = calls[(f[1], f[2])]
                    tids = [int(cl[i]["p1_tid"]), int(cl[i]["p2_tid"])]
                    at = n.clip_reads(as_sites([(tids[0], res[0], 2, d[0]), (tids[1], res[1], 2, d[1])]), QUAL, 10, listing=False)
                    depth = n.base_depth(tids, [res[0], res[1]])
                    assert f[-5:] == [str(int(nsup[i]["n_drp"])), str(int(at[0])), str(int(at[1])), str(int(depth[0])), str(int(depth[1]))], f
            # -- _fusion_rescued.vcf
            head, recs = vcf_records(prefix + "_fusion_rescued.vcf")
            assert head[0] == "##fileformat=VCFv4.2" and head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tTUMOR" + ("\tNORMAL" if with_normal else "")
            assert sum(l.startswith("##INFO=<ID=SC,") for l in head) == 1 and sum(l.startswith("##FORMAT=<ID=CV,") for l in head) == 1
            plain_head, _ = vcf_records(prefix + "_fusion.vcf")
            assert [l for l in head if "ID=SC," not in l and "ID=CV," not in l] == plain_head
            assert len(recs) == 2 * len(calls)
            key = [(names.index(f[0]), int(f[1]), f[2]) for f in recs]
            assert key == sorted(key)
            by_id = {f[2]: f for f in recs}
            for (bp1, bp2), (i, res, d) in calls.items():
                for s in (0, 1):
                    f = by_id["bk%d_%d" % (i, s + 1)]
                    own, mate = (bp1, bp2)[s].split(":"), (bp1, bp2)[1 - s].split(":")
                    info = info_of(f)
                    assert (f[0], f[1]) == tuple(own) and info["MATEID"] == "bk%d_%d" % (i, 2 - s) and info["SVTYPE"] == "BND"
                    assert f[4] == capi.vcf_breakend_alt(f[3], d[s], mate[0], int(mate[1]), d[1 - s])
                    peak_n = int(sup[i]["peak_n"][s][d[s]])
                    assert info["SC"] == str(peak_n) == str(res[2 + s]) and info["SR"] == "0" and info["PE"] == str(int(cl[i]["n_drp"])) and info["SIDES"] == "PE"
                    depth = t.base_depth([int(cl[i]["p%d_tid" % (s + 1)])], [res[s]])
                    assert info["DP"] == str(int(depth[0]))
                    assert f[8] == "DV:RV:CV" and f[9] == "%d:0:%d" % (int(cl[i]["n_drp"]), peak_n)
                    if with_normal:
                        at = n.clip_reads(as_sites([(int(cl[i]["p%d_tid" % (s + 1)]), res[s], 2, d[s])]), QUAL, 10, listing=False)
                        assert f[10] == "%d:0:%d" % (int(nsup[i]["n_drp"]), int(at[0]))
                    assert f[6] in ("PASS", "NoGenePair", "Repeat", "NoGenePair;Repeat")
            # -- _evidence_rescued.txt
            lines = open(prefix + "_evidence_rescued.txt").read().split("\n")
            assert lines[0] == EV_HEADER and lines[-1] == ""
            exp, listed = [], set()
            for i, res, d in sorted(calls.values()):
                tids = [int(cl[i]["p1_tid"]), int(cl[i]["p2_tid"])]
                for r in ev[int(ev_off[i]):int(ev_off[i + 1])]:
                    assert r["kind"] == abi.EV_PAIR
                    sides = "LR"[int(r["sides"]) >> 1] + "LR"[int(r["sides"]) & 1]
                    exp.append(["bk%d" % i, "PE", qnames[int(r["rec"])], names[r["tid1"]], str(r["pos1"]), names[r["tid2"]], str(r["pos2"]), sides, str(r["flag1"]),
                                str(r["flag2"]), str(r["mapq1"]), str(r["mapq2"]), str(r["rec"]), "."])
                _, rows, off = t.clip_reads(as_sites([(tids[0], res[0], 0, d[0]), (tids[1], res[1], 0, d[1])]), QUAL, 10)
                assert len(rows) == res[2] + res[3]  # ClipPeakN1 + ClipPeakN2
                for r in rows:
                    s = int(r["site"])
                    exp.append(["bk%d" % i, "SC", qnames[int(r["rec"])], names[r["tid"]], str(r["p"]), names[tids[1 - s]], str(res[1 - s]), "%d%s" % (s + 1, "LR"[d[s]]),
                                str(r["flag"]), "0", str(r["mapq"]), "0", str(r["rec"]), str(r["clip_len"])])
                listed |= {e[2] for e in exp if e[0] == "bk%d" % i}
            assert [l.split("\t") for l in lines[1:-1]] == exp
            # -- _evidence_rescued.bam: every record of every listed read, in file order
            sel = np.asarray([k for k, q in enumerate(qnames) if q in listed], np.int64)
            contigs, host = capi.decode_bam(prefix + "_evidence_rescued.bam")[:2]
            assert contigs == ds.contigs
            for k in cc.FIXED:
                assert np.array_equal(host[k], cols[k][sel]), k
            return exp

        r3, r2 = rescued_calls(3), rescued_calls(2)
        assert set(r3) == {B_LOCUS} and set(r2) == {B_LOCUS, F_LOCUS}
        exp = check_files(b, r3)
        # the designed locus b: six clipped reads on either side, named; its member pairs
        i = r3[B_LOCUS][0]
        _, vrecs = vcf_records(b + "_fusion_rescued.vcf")
        assert sorted((f[0], f[1], info_of(f)["SC"], f[9].split(":")[2]) for f in vrecs) == [("chr1", "600000", "6", "6"), ("chr3", "500000", "6", "6")]
        sc = [e for e in exp if e[1] == "SC"]
        assert sorted(e[2] for e in sc) == sorted(["bCa_%d" % j for j in range(6)] + ["bCb_%d" % j for j in range(6)])
        assert [e[7] for e in sc] == ["1L"] * 6 + ["2L"] * 6 and all(e[13] == "40" for e in sc)
        assert sum(e[1] == "PE" for e in exp) == int(cl[i]["n_drp"]) > 0
        # -clipsupport 2 adds locus f
        run_cli(base + ["-o", c, "-clip", "-clipsupport", "2"], env)
        exp2 = check_files(c, r2)
        assert {e[2] for e in exp2 if e[1] == "SC"} >= {"fCa_0", "fCa_1", "fCb_0", "fCb_1"} and len(exp2) > len(exp)
        # -genotype: the rescued VCF is the same
        g = os.path.join(tmp, "g")
        run_cli(base + ["-o", g, "-clip", "-genotype"], env)
        assert open(g + "_fusion_rescued.vcf", "rb").read() == open(b + "_fusion_rescued.vcf", "rb").read()
        t.close()
        if n is not None:
            n.close()


def test_cli_rescued_files_of_a_quiet_sample():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "q")
        r = run_cli(["-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast", "-clip", "-vcf", "-evidence"], env)
        assert "rescued cluster count: 0\n" in r.stdout
        head, recs = vcf_records(prefix + "_fusion_rescued.vcf")
        assert recs == [] and any("ID=SC," in l for l in head) and head[-1].endswith("\tTUMOR")
        assert open(prefix + "_evidence_rescued.txt").read() == EV_HEADER + "\n"
        contigs, host = capi.decode_bam(prefix + "_evidence_rescued.bam")[:2]
        assert contigs == tum.contigs and len(host["tid"]) == 0
        assert not os.path.exists(prefix + "_fusion_rescued_normal.txt")

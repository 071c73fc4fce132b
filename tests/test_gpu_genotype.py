"""Genotyping (`bk_ref_support`, `bk_genotype_call`, `-genotype`): the reference-allele counts of every call against a numpy
evaluation of their definition (include/breakid_hip.h) over the record table, exact and with no call left out; the synthetic
truth of designed heterozygous / homozygous / sub-clonal loci; one call with hand-placed records on either side of every clause
of the definition; every table form a context can hold; and the command line's twin files."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc
from tests.callcases import CONTIGS, GENOTYPE_LOCI as LOCI, expected_ref_support, genotype_tumor, side_masks, tumor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")
QUAL = 20


def assert_rows_equal(got, exp, cl):
    assert got.dtype == abi.REF_SUPPORT and len(got) == len(exp) == len(cl)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(cl[i], got[i], exp[i]) for i in bad[:5]]


def genotype_of(c, s):
    """the call's genotype on its junction reads, as the command line reports it"""
    return capi.genotype_call(int(c["n_sr"]), (int(s["ref_reads1"]) + int(s["ref_reads2"]) + 1) // 2)


# ---- a seeded synthetic tumour ----------------------------------------------------------------------------------------------
def locus_of(c, loci=LOCI, tol=5000):
    for L in loci:
        _, ta, pa, tb, pb = L[:5]
        if (c["p1_tid"], c["p2_tid"]) == (ta, tb) and abs(int(c["p1_mean"]) - pa) < tol and abs(int(c["p2_mean"]) - pb) < tol:
            return L
        if (c["p1_tid"], c["p2_tid"]) == (tb, ta) and abs(int(c["p1_mean"]) - pb) < tol and abs(int(c["p2_mean"]) - pa) < tol:
            return L
    return None


# ---- 1. the synthetic tumour ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False])
def test_ref_support_equals_its_definition(fast):
    ds, cols = tumor()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    before, _ = t.fetch(abi.STAGE_CLUSTERS)
    for anchor in (0, 10, 25):
        for mapq_min in (0, 20):
            got = t.ref_support(t, mapq_min, anchor, w)
            cl, _ = t.fetch(abi.STAGE_CLUSTERS)
            assert np.array_equal(cl, before)  # the call changes nothing a fetch returns
            assert_rows_equal(got, expected_ref_support(cl, cols, mapq_min, anchor, w), cl)
            unvoted = (cl["flags"] & 2) == 0
            assert not any(got[f][unvoted].any() for f in got.dtype.names)
    # the synthetic truth at anchor 10, mapq 20: every designed locus is voted and genotyped as designed
    got = t.ref_support(t, QUAL, 10, w)
    seen = {}
    for c, s in zip(cl, got):
        L = locus_of(c)
        if L is None or not c["flags"] & 2:
            continue
        assert L[0] not in seen, L[0]
        gt, gq, vaf = genotype_of(c, s)
        seen[L[0]] = (gt, gq, int(c["n_sr"]), s)
        assert gt == L[7], (L[0], gt, gq, c, s)
        assert int(c["n_sr"]) == L[5], (L[0], c)
    assert set(seen) == {L[0] for L in LOCI}, seen
    for name in ("het1", "het2"):  # ~10x of local reads on either side: some of them span the breakpoint
        assert all(int(seen[name][3][f]) >= 1 for f in ("ref_reads1", "ref_reads2", "ref_pairs1", "ref_pairs2")), (name, seen[name])
    assert seen["sub"][1] == 99 and min(int(seen["sub"][3]["ref_reads1"]), int(seen["sub"][3]["ref_reads2"])) >= 60
    assert min(int(seen["deep"][3]["ref_pairs1"]), int(seen["deep"][3]["ref_pairs2"])) >= 500  # several steps of the kernel's loop per window
    assert int(seen["hom"][3]["ref_reads1"]) + int(seen["hom"][3]["ref_reads2"]) == 0
    t.close()


# ---- 2. one call, hand-placed records ---------------------------------------------------------------------------------------
HAND_CONTIGS = [("chr1", 2_000_000), ("chr2", 6_000), ("chr3", 2_000_000), ("chr4", 2_000_000)]
E1, E2 = 5_530, 700_030  # the main call: chr3:E1 (side 1) and chr4:E2 (side 2)
HAND_W = 1000.5          # W = 1000
F_LEFT, F_RIGHT = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80


def hand_records():
    """name -> (record, counts as ref_reads1, counts as ref_pairs1) at anchor 10, mapq_min 20, W 1000: b = E1 - 1, so a record counts
    with pos <= E1 - 11 and bam_endpos (pos + isize for a pair) >= E1 + 10"""
    R = synth.Rec
    E = E1
    h = {}

    def add(name, reads, pairs, pos, cigar="100M", isize=300, flag=F_LEFT, mapq=60, tid=2):
        h[name] = (R("H_" + name, flag, tid, pos, mapq, cigar, tid, max(0, pos + isize - 100) if isize > 0 else max(0, pos + isize + 100), isize), reads, pairs)

    add("inside", 1, 1, E - 50)
    add("pos_at_bound", 1, 1, E - 11)               # pos == b - A
    add("pos_past_bound", 0, 0, E - 10)             # pos == b - A + 1
    add("end_at_bound", 1, 1, E - 90, isize=100)    # endpos == pos + isize == b + 1 + A
    add("end_before_bound", 0, 0, E - 91, isize=100)
    add("isize_w", 0, 1, E - 500, isize=1000)       # isize == W (the read itself ends far left of the breakpoint)
    add("isize_w1", 0, 0, E - 500, isize=1001)
    add("isize_negative", 1, 0, E - 50, isize=-300, flag=F_RIGHT)
    for bit in (0x4, 0x100, 0x200, 0x400, 0x800):
        add("flag_%x" % bit, 0, 0, E - 50, flag=F_LEFT | bit)
    add("flag_8", 1, 0, E - 50, flag=F_LEFT | 0x8)  # mate unmapped: a read, not a pair
    add("no_paired_bit", 0, 0, E - 50, flag=F_LEFT & ~0x1)
    add("no_proper_bit", 1, 0, E - 50, flag=F_LEFT & ~0x2)
    add("mapq_19", 0, 0, E - 50, mapq=19)
    add("mapq_20", 1, 1, E - 50, mapq=20)
    add("clip_at_bp", 0, 1, E - 60, cigar="60M40S")  # aligned bases end at the breakpoint: the soft clip covers nothing
    add("skip_across", 1, 1, E - 100, cigar="30M200N30M", isize=400)
    add("del_across", 1, 1, E - 50, cigar="40M5D60M")
    add("del_at_bound", 1, 0, E - 95, cigar="40M5D60M", isize=104)  # 105 reference bases with the D: endpos == E + 10; pos + isize == E + 9
    add("other_contig", 0, 0, E - 50, tid=1)        # the end of the contig before: same numbers, another chromosome
    add("other_contig_b", 0, 0, E - 11, tid=1)
    return h


def hand_dataset(seed=5):
    """Background on the three long contigs; the main call chr3:E1 / chr4:E2 with the hand-placed records around E1 and 22 000 proper
    pairs left of E2 (a window of more than 20 000 records); a second call chr1:900 030 / chr4:5, whose side 2 has b - A < 0 at
    anchor 10."""
    rng = np.random.default_rng(seed)
    names = [n for n, _ in HAND_CONTIGS]
    ds = synth.Dataset(list(HAND_CONTIGS))
    for i in range(9000):
        t = (0, 2, 3)[int(rng.integers(0, 3))]
        pr = synth._proper_pair(rng, i, t, 20_000, 1_999_000, 100, 350, 40)
        ds.recs += pr
    for j in range(14):
        ds.recs += synth._discordant_pair("mD_%d" % j, 2, E1 - 30 - int(rng.integers(80, 300)), 3, E2 - 30 + int(rng.integers(40, 300)), 100, False, True)
        ds.recs += synth._discordant_pair("zD_%d" % j, 0, 900_000 - int(rng.integers(80, 300)), 3, 5 + int(rng.integers(40, 300)), 100, False, True)
    for j in range(6):
        ds.recs += synth._split_pair("mS_%d" % j, names, 2, E1, 3, E2, 60, 40)
        ds.recs += synth._split_pair("zS_%d" % j, names, 0, 900_030, 3, 5, 60, 40)
    for j in range(22_000):
        p = E2 - 300 + int(rng.integers(0, 281))
        ds.recs += [synth.Rec("w%d" % j, F_LEFT, 3, p, 60, "100M", 3, p + 150, 250), synth.Rec("w%d" % j, F_RIGHT, 3, p + 150, 60, "100M", 3, p, -250)]
    ds.recs += [v[0] for v in hand_records().values()]
    ds.sort()
    return ds


@pytest.mark.parametrize("fast", [True, False])
def test_ref_support_hand_placed_records(fast):
    ds = hand_dataset()
    cols = ds.to_soa()
    hand = hand_records()
    # the numpy definition itself against the hand-written truth of every placed record
    reads, pairs = side_masks(cols, 2, E1, QUAL, 10, HAND_W)
    idx = {r.qname: i for i, r in enumerate(ds.recs)}
    for name, (rec, in_reads, in_pairs) in hand.items():
        i = idx[rec.qname]
        assert (bool(reads[i]), bool(pairs[i])) == (bool(in_reads), bool(in_pairs)), name
    # a read with an SA tag is never reference evidence: at anchor 0 the split reads' own primaries (60M40S ending at E1) cover the
    # breakpoint base and would count but for their aux blob
    r0, _ = side_masks(cols, 2, E1, QUAL, 0, HAND_W)
    r0_aux, _ = side_masks(cols, 2, E1, QUAL, 0, HAND_W, ignore_aux=True)
    assert int(r0_aux.sum()) - int(r0.sum()) == 6
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    voted = cl[(cl["flags"] & 2) != 0]
    main = [c for c in voted if (c["p1_tid"], int(c["p1_exact"]), c["p2_tid"], int(c["p2_exact"])) == (2, E1, 3, E2)]
    low = [c for c in voted if (c["p1_tid"], int(c["p1_exact"]), c["p2_tid"], int(c["p2_exact"])) == (0, 900_030, 3, 5)]
    assert len(main) == 1 and len(low) == 1, voted
    for anchor in (0, 10):
        for mapq_min in (0, 20):
            for ww in (HAND_W, w):
                got = t.ref_support(t, mapq_min, anchor, ww)
                assert_rows_equal(got, expected_ref_support(cl, cols, mapq_min, anchor, ww), cl)
    got = t.ref_support(t, QUAL, 10, HAND_W)
    m = got[[i for i, c in enumerate(cl) if c["flags"] & 2 and (c["p1_tid"], int(c["p1_exact"])) == (2, E1)][0]]
    assert int(m["ref_reads1"]) >= sum(v[1] for v in hand.values()) and int(m["ref_pairs1"]) >= sum(v[2] for v in hand.values())
    in_window = (cols["tid"] == 3) & (cols["pos"] >= E2 + 10 - int(HAND_W)) & (cols["pos"] <= E2 - 11)
    assert int(in_window.sum()) > 20_000 and int(m["ref_pairs2"]) > 10_000  # the long window: more than a hundred steps of the loop
    z = got[[i for i, c in enumerate(cl) if c["flags"] & 2 and (c["p2_tid"], int(c["p2_exact"])) == (3, 5)][0]]
    assert int(z["ref_reads2"]) == 0 and int(z["ref_pairs2"]) == 0  # b - A = 4 - 10 < 0: no record starts left of it
    t.close()


# ---- 3. the normal as `records`, and the table forms -------------------------------------------------------------------------
def normal_of_tumor():
    """the germline: het1 again (fresh reads), nothing at the other loci but background; sub's locus with deep reference coverage"""
    loci = [("het1", 0, 300_000, 1, 700_000, 5, 200, 1), ("sub", 0, 1_700_000, 2, 900_000, 0, 800, 0)]
    return genotype_tumor(seed=23, loci=loci, prefix="n")


def test_ref_support_of_the_normal():
    ds, cols = tumor()
    nor = normal_of_tumor()
    ncols = nor.to_soa()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, _ = t.run(qual=QUAL, fast=True)
    n = capi.Context(nor.contigs)
    n.upload(ncols)
    n.isize_stats()
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    for anchor, mapq_min in ((10, 20), (0, 0), (25, 20)):
        got = t.ref_support(n, mapq_min, anchor, w)
        assert_rows_equal(got, expected_ref_support(cl, ncols, mapq_min, anchor, w), cl)
    got = t.ref_support(n, QUAL, 10, w)
    own = t.ref_support(t, QUAL, 10, w)  # the rows of the call before are gone; these are the tumour's own again
    assert_rows_equal(own, expected_ref_support(cl, cols, QUAL, 10, w), cl)
    by = {locus_of(c)[0]: s for c, s in zip(cl, got) if c["flags"] & 2 and locus_of(c)}
    assert int(by["sub"]["ref_reads1"]) > 10 and int(by["het1"]["ref_reads1"]) + int(by["het1"]["ref_reads2"]) >= 1
    assert int(by["hom"]["ref_reads1"]) + int(by["hom"]["ref_reads2"]) <= 4  # background only: "no coverage" is visible as such
    t.close()
    n.close()


@pytest.mark.parametrize("fast", [True, False])
def test_ref_support_after_exclude_regions(fast):
    ds, cols = tumor()
    tid = np.asarray([0, 2, 3, 1], np.int32)
    beg = np.asarray([299_900, 899_000, 0, 1_499_990], np.int32)  # through het1's reference reads, next to sub, the head of chr4, a sliver of hom
    end = np.asarray([299_990, 899_800, 50_000, 1_500_000], np.int32)
    keep = ~cc.excluded_mask(cols, tid, beg, end)
    kept = cc.filtered(cols, keep)
    for where in ("host", "device"):
        t, hold = cc.make_ctx(ds.contigs, cols, where)
        assert t.exclude_regions(tid, beg, end) == int((~keep).sum()) > 0
        w, _ = t.run(qual=QUAL, fast=fast)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        assert (cl["flags"] & 2).sum() >= 4
        for anchor in (0, 10):
            got = t.ref_support(t, QUAL, anchor, w)
            assert_rows_equal(got, expected_ref_support(cl, kept, QUAL, anchor, w), cl)
        t.close()
        del hold


@pytest.mark.parametrize("side", [True, False])
def test_ref_support_device_table(side):
    """BK_MEM_DEVICE: a table generated in HBM with bk_side rows, and device copies of host columns without them"""
    import torch
    if side:
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
        cols = synth_gpu.to_numpy_cols(dcols)
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
    else:
        ds, cols = tumor()
        t, hold = cc.make_ctx(ds.contigs, cols, "device")
    w, n_valid = t.run(qual=QUAL, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert n_valid > 0
    for anchor, mapq_min in ((10, 20), (0, 0)):
        got = t.ref_support(t, mapq_min, anchor, w)
        assert_rows_equal(got, expected_ref_support(cl, cols, mapq_min, anchor, w), cl)
    t.close()
    del hold


def test_ref_support_errors():
    ds, cols = tumor()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.ref_support(t, QUAL, 10, 1000.0)
    w, _ = t.run(qual=QUAL, fast=True)
    n = capi.Context(ds.contigs)
    n.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_isize_stats on the records context"):
        t.ref_support(n, QUAL, 10, w)
    n.isize_stats()
    with pytest.raises(capi.BreakIDError, match="anchor must not be negative"):
        t.ref_support(n, QUAL, -1, w)
    with pytest.raises(capi.BreakIDError, match="mapq_min must not be negative"):
        t.ref_support(n, -1, 10, w)
    assert len(t.ref_support(n, QUAL, 10, w)) == len(t.fetch(abi.STAGE_CLUSTERS)[0])
    o = capi.Context([(name, ln + 1) for name, ln in ds.contigs])
    o.upload(cols)
    o.isize_stats()
    with pytest.raises(capi.BreakIDError, match="reference lists differ"):
        t.ref_support(o, QUAL, 10, w)
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts"):
        t.ref_support(s, QUAL, 10, w)
    with pytest.raises(capi.BreakIDError, match="sharded contexts"):
        s.ref_support(t, QUAL, 10, w)
    for c in (t, n, o, s):
        c.close()


# ---- 4. command line --------------------------------------------------------------------------------------------------------
GT_TEXT = {0: "0/0", 1: "0/1", 2: "1/1", 255: "./."}
G_COLS = ["Ref_Pairs1", "Ref_Pairs2", "Ref_Reads1", "Ref_Reads2", "VAF_Pairs", "VAF_Reads", "GT", "GQ"]
N_COLS = ["Normal_DRP", "Normal_SR", "Normal_Depth1", "Normal_Depth2"]


def genotype_fields(s, n_drp, n_sr):
    """the eight columns of one sample as the command line prints them (iostream's default float format is %g)"""
    def vaf_text(v):
        return "." if np.isnan(v) else "%g" % float(v)
    gt, gq, vaf = capi.genotype_call(n_sr, (int(s["ref_reads1"]) + int(s["ref_reads2"]) + 1) // 2)
    _, _, vaf_pairs = capi.genotype_call(n_drp, (int(s["ref_pairs1"]) + int(s["ref_pairs2"]) + 1) // 2)
    return [str(int(s[f])) for f in ("ref_pairs1", "ref_pairs2", "ref_reads1", "ref_reads2")] + [vaf_text(vaf_pairs), vaf_text(vaf), GT_TEXT[gt], str(gq)]


def _write(ds, path, aligned=True):
    ds.write_bam(path, aligned=aligned)
    bamio.write_bai(path)


def exclude_bed(path):
    with open(path, "w") as f:
        f.write("chr1\t299900\t299990\nchr3\t899000\t899800\n")
    return (np.asarray([0, 2], np.int32), np.asarray([299_900, 899_000], np.int32), np.asarray([299_990, 899_800], np.int32))


@pytest.mark.parametrize("variant", ["gpu_feed", "across_blocks", "host_decode", "exclude", "normal", "normal_exclude"])
@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_cli_genotype_twin_files(mode, variant):
    ds, cols = tumor()
    with_normal, with_x = variant.startswith("normal"), variant.endswith("exclude")
    refgene = synth.random_refgene(ds.contigs, 60, 5)
    anchor = 25 if variant == "across_blocks" else 10
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb, bed = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "x.bed")
        _write(ds, tb, aligned=variant != "across_blocks")
        side = synth.write_side_files(ds, tmp, refgene_lines=refgene)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        if variant == "host_decode":
            env["BREAKID_HOST_DECODE"] = "1"
        extra = ["-all"] + (["-fast"] if mode == "fast" else [])
        ncols = None
        if with_normal:
            nor = normal_of_tumor()
            ncols = nor.to_soa()
            nor.write_bam(nb, aligned=True)
            extra += ["-normal", nb]
        lst = None
        if with_x:
            lst = exclude_bed(bed)
            extra += ["-x", bed]
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        r = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-o", b, "-genotype"] + (["-anchor", "25"] if anchor == 25 else []), env=dict(env, BK_DEBUG="feed"), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        feeds = [l for l in r.stderr.split("\n") if l.startswith("[feed/gpu]") and "file -> device table" in l]
        if variant == "host_decode":
            assert not feeds, feeds
        elif not with_x:
            assert len(feeds) == 1 + with_normal and ("records across blocks" in feeds[0]) == (variant == "across_blocks"), feeds
        # every file without _genotype is byte-identical to the run without -genotype
        plain_files = ["_fusion.txt", "_fusion_all.txt"] + (["_fusion_normal.txt", "_fusion_all_normal.txt"] if with_normal else [])
        for suffix in plain_files:
            assert open(a + suffix).read() == open(b + suffix).read(), suffix
        pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
        assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "genotype_anchor\t%d\n" % anchor, (pa, pb)
        fa, fb = open(a + "_performance.txt").read().split("\n"), open(b + "_performance.txt").read().split("\n")
        assert fa[0] == fb[0] and fa[1].split("\t")[:5] == fb[1].split("\t")[:5]
        assert not os.path.exists(a + "_fusion_genotype.txt") and not os.path.exists(a + "_fusion_all_genotype.txt")
        # the same calls through the C ABI (the records of the BAM files)
        t = capi.Context(ds.contigs)
        t.upload(cols)
        if with_x:
            t.exclude_regions(*lst)
        w, _ = t.run(qual=QUAL, fast=mode == "fast")
        sup = t.ref_support(t, QUAL, anchor, w)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        nsup = rsup_n = None
        if with_normal:
            n = capi.Context(ds.contigs)
            n.upload(ncols)
            if with_x:
                n.exclude_regions(*lst)
            n.isize_stats()
            n.discordant_pairs(QUAL, w)
            n.split_evidence()
            nsup = t.normal_support(n, w)
            rsup_n = t.ref_support(n, QUAL, anchor, w)
            n.close()
        t.close()
        names = [nm for nm, _ in ds.contigs]
        by_call = {}
        for i, c in enumerate(cl):
            if c["flags"] & 2:
                key = (names[c["p1_tid"]] + ":%d" % c["p1_exact"], names[c["p2_tid"]] + ":%d" % c["p2_exact"], str(c["n_drp"]), str(c["n_sr"]))
                f = genotype_fields(sup[i], int(c["n_drp"]), int(c["n_sr"]))
                if with_normal:
                    f += [str(int(nsup[i][x])) for x in ("n_drp", "n_sr", "depth1", "depth2")]
                    f += genotype_fields(rsup_n[i], int(nsup[i]["n_drp"]), int(nsup[i]["n_sr"]))
                by_call.setdefault(key, []).append(f)
        header_tail = G_COLS + ((N_COLS + ["Normal_" + x for x in G_COLS]) if with_normal else [])
        n_rows = 0
        for suffix in ("_fusion", "_fusion_all"):
            plain = open(b + suffix + ".txt").read().split("\n")
            twin = open(b + suffix + "_genotype.txt").read().split("\n")
            assert len(plain) == len(twin)
            assert twin[0] == plain[0] + "\t" + "\t".join(header_tail)
            for p, q in zip(plain[1:], twin[1:]):
                f = q.split("\t")
                assert "\t".join(f[:15]) == p
                if not p:
                    continue
                n_rows += 1
                cand = by_call[(f[1], f[2], f[7], f[8])]
                assert all(x == cand[0] for x in cand) and f[15:] == cand[0], (f, cand)
        assert n_rows >= (4 if with_x else len(LOCI))


def test_cli_genotype_errors_and_a_sample_without_calls():
    """no cluster: the fusion files hold their header only, and so do their twins; the options are checked before anything is read"""
    tum = synth.Dataset(list(CONTIGS))
    rng = np.random.default_rng(3)
    for i in range(4000):
        tum.recs += synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)
    tum.sort()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        _write(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for extra, msg in ((["-anchor", "5"], "-anchor needs -genotype"), (["-genotype", "-gpus", "2"], "-genotype cannot be combined with -gpus"),
                           (["-genotype", "-anchor", "-1"], "-anchor must be a number from 0 to 2147483647")):
            r = subprocess.run(base + extra, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and msg in r.stderr, r.stderr[-2000:]
            assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-genotype", "-anchor", "0"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for suffix in ("_fusion", "_fusion_all"):
            plain = open(prefix + suffix + ".txt").read()
            assert plain.count("\n") == 1, plain
            assert open(prefix + suffix + "_genotype.txt").read() == plain[:-1] + "\t" + "\t".join(G_COLS) + "\n"
        assert open(prefix + "_params.txt").read().endswith("genotype_anchor\t0\n")

"""Matched-normal evidence (`bk_normal_support`, `-normal`): the four counts of every tumour call against a numpy evaluation of
their definition (include/breakid_hip.h) over the normal's own stage tables, the normal = tumour invariants, and the command
line's twin files."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests.callcases import DENSE, GERMLINE, SOMATIC, expected_support, tumor_normal
from tools import make_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")
QUAL = 20


# ---- a tumour / normal pair -----------------------------------------------------------------------------------------------
def locus_of(c, loci, tol=5000):
    for L in loci:
        ta, pa, tb, pb = L[:4]
        if (c["p1_tid"], c["p2_tid"]) == (ta, tb) and abs(int(c["p1_mean"]) - pa) < tol and abs(int(c["p2_mean"]) - pb) < tol:
            return L
        if (c["p1_tid"], c["p2_tid"]) == (tb, ta) and abs(int(c["p1_mean"]) - pb) < tol and abs(int(c["p2_mean"]) - pa) < tol:
            return L
    return None


def run_pair(contigs, tcols, ncols, fast):
    t = capi.Context(contigs)
    t.upload(tcols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    n = capi.Context(contigs)
    n.upload(ncols)
    n.isize_stats()
    n.discordant_pairs(QUAL, w)
    n.split_evidence()
    return t, n, w


# ---- 1. brute-force equality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", ["ordered", "wide", "swapped"])
@pytest.mark.parametrize("fast", [True, False])
def test_normal_support_equals_its_definition(fast, header):
    """wide: 70 000 extra contigs, (nt + 1)^2 no longer fits in 32 bits and the pair index ranks the chromosome pairs instead.
    swapped: the header lists chr2 before chr1, so a tuple's own side carries the id of chr1 on the first contig and of chr2 on
    the second (the reference's chromID2ChrName of the tid): the split reads of the loci on those two contigs no longer pair up
    in the vote, the loci on chr3 / chr4 are called as before, and the tuple search must follow the own-side ids."""
    tum, nor = tumor_normal(extra_contigs=70_000 if header == "wide" else 0,
                            names4=("chr2", "chr1", "chr3", "chr4") if header == "swapped" else ("chr1", "chr2", "chr3", "chr4"))
    tcols, ncols = tum.to_soa(), nor.to_soa()
    t, n, w = run_pair(tum.contigs, tcols, ncols, fast)
    got = t.normal_support(n, w)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    scan, _ = n.fetch(abi.STAGE_SCAN)
    splits, _ = n.fetch(abi.STAGE_SPLITS)
    exp = expected_support(cl, scan, splits, ncols, w)
    assert got.dtype == abi.NORMAL_SUPPORT and len(got) == len(cl)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(cl[i], got[i], exp[i]) for i in bad[:5]]
    assert (cl["flags"] & 2).any()
    # the synthetic truth: every locus is called, germline calls have support in the normal, somatic calls have none
    seen = set()
    for c, s in zip(cl, got):
        L = locus_of(c, GERMLINE + [DENSE] + SOMATIC)
        if L is None:
            continue
        seen.add(L)
        if L in SOMATIC:
            assert s["n_drp"] == 0 and s["n_sr"] == 0, (c, s)
        else:
            assert s["n_drp"] > 0, (c, s)
            if c["flags"] & 2:
                assert s["n_sr"] > 0 and s["depth1"] > 0 and s["depth2"] > 0, (c, s)
        if L == DENSE:
            assert s["n_drp"] > 256, (c, s)
    assert seen == set(GERMLINE + [DENSE] + SOMATIC), seen
    if header != "swapped":
        assert sum(int(c["flags"]) >> 1 & 1 for c in cl) >= len(GERMLINE) + len(SOMATIC)
    t.close()
    n.close()


def test_normal_support_errors():
    tum, nor = tumor_normal()
    tcols, ncols = tum.to_soa(), nor.to_soa()
    t = capi.Context(tum.contigs)
    t.upload(tcols)
    n = capi.Context(nor.contigs)
    n.upload(ncols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.normal_support(n, 1000.0)
    w, _ = t.run(qual=QUAL, fast=True)
    with pytest.raises(capi.BreakIDError, match="normal context first"):
        t.normal_support(n, w)
    n.isize_stats()
    n.discordant_pairs(QUAL, w)
    n.split_evidence()
    with pytest.raises(capi.BreakIDError, match="tumour's distance"):
        t.normal_support(n, w + 1.0)
    n2 = capi.Context(nor.contigs)
    n2.upload(ncols)
    n2.isize_stats()
    n2.discordant_pairs(QUAL, w + 1.0)
    n2.split_evidence()
    with pytest.raises(capi.BreakIDError, match="mapq_min and w"):
        t.normal_support(n2, w)
    n2.close()
    other = [(name, ln + 1) for name, ln in tum.contigs]
    o = capi.Context(other)
    o.upload(ncols)
    o.isize_stats()
    o.discordant_pairs(QUAL, w)
    o.split_evidence()
    with pytest.raises(capi.BreakIDError, match="reference lists differ"):
        t.normal_support(o, w)
    # a normal without pairs or tuples: zeros
    e = synth.Dataset(list(tum.contigs))
    for i in range(2000):
        e.recs += synth._proper_pair(np.random.default_rng(i), i, i % 4, 1000, 1_999_000, 100, 350, 40)
    e.sort()
    z = capi.Context(e.contigs)
    z.upload(e.to_soa())
    z.isize_stats()
    assert z.discordant_pairs(QUAL, w)[0] == 0 and z.split_evidence() == 0
    got = t.normal_support(z, w)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    assert len(got) == len(cl) > 0 and not got["n_drp"].any() and not got["n_sr"].any()
    for c in (t, n, o, z):
        c.close()


# ---- 2. normal = tumour -----------------------------------------------------------------------------------------------------
def _self_case(name):
    if name == "cfg1M":
        contigs = [("chr%d" % i, 8_000_000) for i in range(1, 13)]
        return synth.make_cfg(11, contigs, 1_000_000, 1600, 16, 400, split_every=1, splits_per_locus=6, jitter=250, read_len=100)
    return next(ds for n, ds, _ in make_golden.datasets() if n == name)


def distinct_members(clustered):
    """(group, cluster id) -> number of distinct pairs (by record index) among the cluster's members"""
    trip = np.unique(np.stack([clustered["group"].astype(np.int64), clustered["cluster"].astype(np.int64), clustered["rec"].astype(np.int64)], 1), axis=0)
    gc, cnt = np.unique(trip[:, :2], axis=0, return_counts=True)
    return {(int(g), int(c)): int(k) for (g, c), k in zip(gc, cnt)}


@pytest.mark.parametrize("case", ["g1", "edge", "cfg1M"])
def test_normal_equal_to_tumor(case):
    """With the tumour as its own normal every cluster's pairs lie in its window, the tuple that produced the voted pair is
    in the normal, and the depths are the tumour's own.

    n_drp is compared with the cluster's DISTINCT pairs: the reference's clustering can list one pair twice in a cluster
    (cfg1M -fast has 13 such clusters, the oracle agrees), and the cluster's own n_drp counts it twice, while the normal's
    BK_STAGE_SCAN table holds it once."""
    ds = _self_case(case)
    cols = ds.to_soa()
    for fast in (True, False):
        t, n, w = run_pair(ds.contigs, cols, cols, fast)
        got = t.normal_support(n, w)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        voted = (cl["flags"] & 2) != 0
        assert len(got) == len(cl)
        clustered, _ = t.fetch(abi.STAGE_CLUSTERED)
        members = distinct_members(clustered)
        distinct = np.asarray([members[(int(c["group"]), int(c["id"]))] for c in cl], np.int64)
        assert (distinct <= cl["n_drp"]).all() and (got["n_drp"] >= distinct).all()
        assert (got["n_sr"][voted] >= 1).all()
        assert (got["n_sr"][~voted] == 0).all() and (got["depth1"][~voted] == 0).all()
        assert np.array_equal(got["depth1"][voted], cl["depth1"][voted]) and np.array_equal(got["depth2"][voted], cl["depth2"][voted])
        if case == "cfg1M":
            assert len(cols["tid"]) >= 1_000_000 and voted.sum() >= 1000, (len(cols["tid"]), voted.sum())
        t.close()
        n.close()


# ---- 3. command line --------------------------------------------------------------------------------------------------------
def _write(ds, path):
    ds.write_bam(path, aligned=True)
    bamio.write_bai(path)


@pytest.mark.parametrize("normal_aligned", [True, False])
@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_cli_normal_twin_files(mode, normal_aligned):
    """normal_aligned: the normal's records stay inside their BGZF blocks (the GPU feed's streaming decoder) or run across them"""
    tum, nor = tumor_normal()
    refgene = synth.random_refgene(tum.contigs, 60, 5)
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        _write(tum, tb)
        nor.write_bam(nb, aligned=normal_aligned)  # no index: the normal needs none
        side = synth.write_side_files(tum, tmp, refgene_lines=refgene)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        base = [BIN, "-i", tb, "-n", side["nib"], "-all"] + (["-fast"] if mode == "fast" else [])
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        r = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-o", b, "-normal", nb], env=dict(env, BK_DEBUG="feed"), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        feeds = [l for l in r.stderr.split("\n") if l.startswith("[feed/gpu]") and "file -> device table" in l]
        assert len(feeds) == 2 and ("records across blocks" in feeds[1]) == (not normal_aligned), feeds  # tumour, then the normal: GPU feed
        for suffix in ("_fusion.txt", "_fusion_all.txt"):
            assert open(a + suffix).read() == open(b + suffix).read(), suffix
        pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
        assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "normal_file\t" + nb + "\n", (pa, pb)
        fa, fb = open(a + "_performance.txt").read().split("\n"), open(b + "_performance.txt").read().split("\n")
        assert fa[0] == fb[0] and fa[1].split("\t")[:5] == fb[1].split("\t")[:5]
        assert not os.path.exists(a + "_fusion_normal.txt") and not os.path.exists(a + "_fusion_all_normal.txt")
        # the counts of the same calls through the C ABI (same records as the BAM files)
        t, n, w = run_pair(tum.contigs, tum.to_soa(), nor.to_soa(), mode == "fast")
        sup = t.normal_support(n, w)
        cl, _ = t.fetch(abi.STAGE_CLUSTERS)
        names = [nm for nm, _ in tum.contigs]
        by_call = {}
        for c, s in zip(cl, sup):
            if c["flags"] & 2:
                key = (names[c["p1_tid"]] + ":%d" % c["p1_exact"], names[c["p2_tid"]] + ":%d" % c["p2_exact"], str(c["n_drp"]), str(c["n_sr"]))
                by_call.setdefault(key, []).append([str(int(s[f])) for f in ("n_drp", "n_sr", "depth1", "depth2")])
        t.close()
        n.close()
        n_rows = 0
        for suffix in ("_fusion", "_fusion_all"):
            plain = open(b + suffix + ".txt").read().split("\n")
            twin = open(b + suffix + "_normal.txt").read().split("\n")
            assert len(plain) == len(twin)
            assert twin[0] == plain[0] + "\tNormal_DRP\tNormal_SR\tNormal_Depth1\tNormal_Depth2"
            for p, q in zip(plain[1:], twin[1:]):
                f = q.split("\t")
                assert "\t".join(f[:15]) == p
                if not p:
                    continue
                n_rows += 1
                cand = by_call[(f[1], f[2], f[7], f[8])]
                assert all(x == cand[0] for x in cand) and f[15:] == cand[0], (f, cand)
        assert n_rows >= len(GERMLINE) + len(SOMATIC)


def test_cli_normal_errors():
    tum, nor = tumor_normal()
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb, ob = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "o.bam")
        _write(tum, tb)
        _write(nor, nb)
        other = synth.Dataset([(name, ln + 10) for name, ln in nor.contigs], nor.recs)
        other.write_bam(ob, aligned=True)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "x")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-fast"]
        r = subprocess.run(base + ["-normal", ob], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: tumor and normal BAM headers differ" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(prefix + "_fusion_normal.txt")
        r = subprocess.run(base + ["-gpus", "2", "-normal", nb], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-normal cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
        r = subprocess.run(base + ["-normal", os.path.join(tmp, "missing.bam")], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: can not open normal bam-file" in r.stderr, r.stderr[-2000:]


def test_cli_normal_twins_of_a_tumour_without_calls():
    """no cluster in the tumour: the fusion files hold their header only, and so do their twins"""
    _, nor = tumor_normal()
    tum = synth.Dataset(list(nor.contigs))
    rng = np.random.default_rng(3)
    for i in range(4000):
        tum.recs += synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)
    tum.sort()
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        _write(tum, tb)
        nor.write_bam(nb, aligned=True)
        side = synth.write_side_files(tum, tmp)
        prefix = os.path.join(tmp, "z")
        r = subprocess.run([BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast", "-normal", nb], env=dict(os.environ, BREAKID_INSTALLDIR=side["install"]),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for suffix in ("_fusion", "_fusion_all"):
            plain = open(prefix + suffix + ".txt").read()
            assert plain.count("\n") == 1, plain
            assert open(prefix + suffix + "_normal.txt").read() == plain[:-1] + "\tNormal_DRP\tNormal_SR\tNormal_Depth1\tNormal_Depth2\n"

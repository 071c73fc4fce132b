"""VCF breakend output (`bk_junctions`, `bk_junction_sides`, `bk_vcf_breakend_alt`, `-vcf`): the junction evidence of every cluster
against a numpy evaluation of its definition (include/breakid_hip.h) over the fetched stage tables, exact and with no row left out;
the designed truth of loci whose retained sides are known; every table form a context can hold; and the command line's VCF read
back with a strict reader and compared, field by field, with what the C ABI gives for the same table."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests.callcases import (EXCLUDE, LOCI, MIX, NAMES, call_dataset, designed_normal, designed_refgene, designed_tumor, expected_junctions, fusion_rows,
                             quiet_tumor, rows_of, write_indexed)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")
QUAL = 20


def assert_rows_equal(got, exp, cl):
    assert got.dtype == abi.JUNCTION and len(got) == len(exp) == len(cl)
    bad = [i for i in range(len(cl)) if got[i].tobytes() != exp[i].tobytes()]
    assert not bad, [(cl[i], got[i], exp[i]) for i in bad[:5]]


def check_context(t, normal_sr=None):
    """bk_junctions of a context that has run, against the definition over its own fetched tables, and the invariants"""
    before = [t.fetch(st)[0] for st in (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)]
    got = t.junctions()
    clustered, splits, cl = [t.fetch(st)[0] for st in (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)]
    for a, b in zip(before, (clustered, splits, cl)):
        assert np.array_equal(a, b)  # the call changes nothing a fetch returns
    assert_rows_equal(got, expected_junctions(cl, clustered, splits), cl)
    assert np.array_equal(got["pairs"].astype(np.int64).sum(1), cl["n_drp"].astype(np.int64))
    unvoted = (cl["flags"] & 2) == 0
    assert not got["splits"][unvoted].any()
    if normal_sr is not None:
        assert np.array_equal(got["splits"].astype(np.int64).sum(1), normal_sr.astype(np.int64))
    assert_rows_equal(t.junctions(), got, cl)  # a second call returns the same rows
    return got, cl


def self_normal_sr(contigs, cols, t, w):
    """n_sr of bk_normal_support with a second context over the same table as the normal"""
    n = capi.Context(contigs)
    n.upload(cols)
    n.isize_stats()
    n.discordant_pairs(QUAL, w)
    n.split_evidence()
    sr = t.normal_support(n, w)["n_sr"]
    n.close()
    return sr


# ---- 1. the definition, every row ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["genotype", "edge", "cfg"])
@pytest.mark.parametrize("fast", [True, False])
def test_junctions_equal_their_definition(fast, name):
    ds, cols = call_dataset(name)
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    got, cl = check_context(t, self_normal_sr(ds.contigs, cols, t, w))
    if name != "edge":
        assert n_valid >= (5 if name == "genotype" else 100) and got["splits"].any()
    t.close()


@pytest.mark.parametrize("fast", [True, False])
def test_junctions_renamed_reference_list(fast):
    """a padded reference list that names chr2 before chr1: a tuple's own side carries the id of chr1 on the first contig and of
    chr2 on the second, and the tuple search must follow those ids"""
    tum, _ = cc.tumor_normal(extra_contigs=300, names4=("chr2", "chr1", "chr3", "chr4"))
    cols = tum.to_soa()
    t = capi.Context(tum.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    got, cl = check_context(t, self_normal_sr(tum.contigs, cols, t, w))
    assert n_valid >= 3 and got["splits"].any()
    t.close()


# ---- 2. designed truth --------------------------------------------------------------------------------------------------------
_DESIGNED = {}


def designed():
    if "t" not in _DESIGNED:
        ds = designed_tumor()
        _DESIGNED["t"] = (ds, ds.to_soa())
    return _DESIGNED["t"]


def zero_splits(row):
    r = np.zeros(1, abi.JUNCTION)
    r[0] = row
    r["splits"][0] = 0
    return r[0]


@pytest.mark.parametrize("fast", [True, False])
def test_designed_sides(fast):
    ds, cols = designed()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    got, cl = check_context(t, self_normal_sr(ds.contigs, cols, t, w))  # (every expected value comes from the fetched stage tables)
    for name, ta, bpa, da, tb, bpb, db in LOCI:
        rows = rows_of(cl, ta, bpa, tb, bpb)
        assert rows, "locus %s is not called" % name
        for i, a_first in rows:
            d1, d2 = (da, db) if a_first else (db, da)
            r1, r2 = int(d1 == "R"), int(d2 == "R")
            j = got[i]
            print(name, "fast" if fast else "default", "pairs", j["pairs"].tolist(), "splits", j["splits"].tolist())
            assert int(j["splits"][2 * r1 + r2]) == int(j["splits"].sum()) > 0, (name, j)
            assert int(j["pairs"][2 * r1 + r2]) == int(j["pairs"].sum()) > 0, (name, j)
            assert int(j["mapq_sum1"]) == int(j["mapq_sum2"]) == 60 * int(j["pairs"].sum())
            assert capi.junction_sides(j) == (r1, r2, 2), (name, j)
            assert capi.junction_sides(zero_splits(j)) == (r1, r2, 1), (name, j)
    _, ta, bpa, tb, bpb = MIX
    rows = rows_of(cl, ta, bpa, tb, bpb)
    assert rows, "the mixed locus is not called"
    for i, a_first in rows:
        j = got[i]
        strands = 1 if a_first else 2  # (forward, reverse) seen from side A
        assert int(j["pairs"][strands]) == int(j["pairs"].sum()) > 0, j
        assert int(j["splits"][0]) == int(j["splits"].sum()) > 0, j
        assert capi.junction_sides(j) == (0, 0, 2), j  # the split reads overrule the pairs
        assert capi.junction_sides(zero_splits(j)) == (strands >> 1, strands & 1, 1), j
    t.close()


# ---- 3. table forms, call order, errors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "device_side", "exclude_host", "exclude_device"])
def test_junctions_table_forms(form):
    import torch
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
    else:
        ds, cols = designed()
        t, hold = cc.make_ctx(ds.contigs, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            tid, beg, end = np.asarray([0, 3], np.int32), np.asarray([50_000, 100_000], np.int32), np.asarray([60_000, 120_000], np.int32)
            assert t.exclude_regions(tid, beg, end) > 0
    w, n_valid = t.run(qual=QUAL, fast=True)
    assert n_valid > 0
    got, cl = check_context(t)
    assert got["splits"].any()
    t.close()
    del hold


def test_junctions_call_order_and_errors():
    ds, cols = designed()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.junctions()
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    t.mask_and_cluster(w, True)
    t.split_evidence()
    t.cluster_summary(w)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints") as e:
        t.junctions()
    assert e.value.code == abi.BK_ERR_ARG
    t.split_breakpoints(w)
    got, cl = check_context(t)
    data, n = capi.C.c_void_p(), capi.C.c_uint64()
    assert t.L.bk_junctions(t.h, None, capi.C.byref(n)) == abi.BK_ERR_ARG and b"null output" in t.L.bk_last_error(t.h)
    assert t.L.bk_junctions(t.h, capi.C.byref(data), None) == abi.BK_ERR_ARG
    assert t.L.bk_junctions(None, capi.C.byref(data), capi.C.byref(n)) == abi.BK_ERR_ARG
    # the other mode on the same context: the rows follow the new clusters once the stages have run again
    t.mask_and_cluster(w, False)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.junctions()
    t.cluster_summary(w)
    t.split_breakpoints(w)
    check_context(t)
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts"):
        s.junctions()
    t.close()
    s.close()


def test_junctions_of_a_context_without_clusters():
    tum = quiet_tumor()
    t = capi.Context(tum.contigs)
    t.upload(tum.to_soa())
    t.run(qual=QUAL, fast=True)
    assert len(t.fetch(abi.STAGE_CLUSTERS)[0]) == 0
    got = t.junctions()
    assert got.dtype == abi.JUNCTION and len(got) == 0
    t.close()


# ---- 4. command line ----------------------------------------------------------------------------------------------------------
GT_TEXT = {0: "0/0", 1: "0/1", 2: "1/1", 255: "./."}
INFO_KEYS = ["SVTYPE", "MATEID", "EVENTTYPE", "PE", "SR", "MAPQ", "DP", "GENE", "SIDES"]
SOURCE_TEXT = {2: "SR", 1: "PE", 0: "NONE"}
ALT_RE = re.compile(r"^(?:([ACGTN])([\[\]])([^\[\]:]+):([0-9]+)([\[\]])|([\[\]])([^\[\]:]+):([0-9]+)([\[\]])([ACGTN]))$")


def fusion_type(mask):
    for bit, text in ((8, "Deletion"), (4, "Duplication"), (2, "Inversion"), (1, "Translocation")):
        if mask & bit:
            return text
    return "Unknown"


def nib_base(nib_dir, chrom, pos1):
    with open(os.path.join(nib_dir, "hg19_%s.nib" % chrom), "rb") as f:
        f.seek(8 + (pos1 - 1) // 2)
        b = f.read(1)[0]
    return "TCAG"[((b >> 4) if (pos1 - 1) % 2 == 0 else b) & 3]


def read_vcf(path, contigs):
    """a strict reader: (sample names, records); a record is a dict of its columns with INFO and the samples taken apart"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0] == "##fileformat=VCFv4.2" and lines[1] == "##source=BreakID", lines[:2]
    lines = lines[:-1]
    n_meta = next(i for i, l in enumerate(lines) if not l.startswith("##"))
    meta = lines[:n_meta]
    assert [l for l in meta if l.startswith("##contig=")] == ["##contig=<ID=%s,length=%d>" % c for c in contigs]
    declared = {"INFO": {}, "FORMAT": {}, "FILTER": {}}
    for l in meta[2:]:
        if l.startswith("##contig="):
            continue
        m = re.match(r'^##(INFO|FORMAT)=<ID=([A-Za-z0-9_]+),Number=(1|\.),Type=(Integer|String),Description="[^"]+">$', l) or \
            re.match(r'^##(FILTER)=<ID=([A-Za-z0-9_]+),Description="[^"]+">$', l)
        assert m, l
        assert m.group(2) not in declared[m.group(1)], l
        declared[m.group(1)][m.group(2)] = m.group(4) if m.group(1) != "FILTER" else None
    assert not any("date" in l.lower() or "command" in l.lower() for l in meta)
    cols = lines[n_meta].split("\t")
    assert cols[:9] == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] and cols[9] == "TUMOR" and cols[10:] in ([], ["NORMAL"]), cols
    index = {n: i for i, (n, _) in enumerate(contigs)}
    recs = []
    for l in lines[n_meta + 1:]:
        f = l.split("\t")
        assert len(f) == len(cols), l
        r = dict(zip(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"], f[:9]))
        assert r["CHROM"] in index and re.match(r"^[1-9][0-9]*$", r["POS"]) and r["QUAL"] == "." and r["REF"] in "ACGTN" and len(r["REF"]) == 1, l
        r["POS"] = int(r["POS"])
        assert 1 <= r["POS"] <= contigs[index[r["CHROM"]]][1]
        r["filters"] = r["FILTER"].split(";")
        assert all(x in declared["FILTER"] for x in r["filters"]) and (r["filters"] == ["PASS"] or "PASS" not in r["filters"]), l
        info = [kv.split("=") for kv in r["INFO"].split(";")]
        assert all(len(kv) == 2 and kv[1] != "" for kv in info) and [kv[0] for kv in info] == INFO_KEYS, l
        r["info"] = dict(info)
        for k, v in r["info"].items():
            assert k in declared["INFO"] and (declared["INFO"][k] != "Integer" or re.match(r"^[0-9]+$", v)), (k, v)
        keys = r["FORMAT"].split(":")
        assert all(k in declared["FORMAT"] for k in keys) and sorted(keys) == sorted(declared["FORMAT"]), l
        r["samples"] = []
        for s in f[9:]:
            v = s.split(":")
            assert len(v) == len(keys), l
            for k, x in zip(keys, v):
                assert re.match(r"^[0-9]+$", x) if declared["FORMAT"][k] == "Integer" else x in GT_TEXT.values(), (k, x)
            r["samples"].append(dict(zip(keys, v)))
        m = ALT_RE.match(r["ALT"])
        assert m, l
        g = m.groups()
        if g[0] is not None:
            r["alt"] = dict(base=g[0], own_right=0, mate_chr=g[2], mate_pos=int(g[3]), mate_right=int(g[1] == "["))
            assert g[1] == g[4]
        else:
            r["alt"] = dict(base=g[9], own_right=1, mate_chr=g[6], mate_pos=int(g[7]), mate_right=int(g[5] == "["))
            assert g[5] == g[8]
        assert r["alt"]["base"] == r["REF"] and r["info"]["SVTYPE"] == "BND"
        recs.append(r)
    order = [(index[r["CHROM"]], r["POS"], r["ID"]) for r in recs]
    assert order == sorted(order)
    by_id = {r["ID"]: r for r in recs}
    assert len(by_id) == len(recs)
    for r in recs:
        m = re.match(r"^bk([0-9]+)_([12])$", r["ID"])
        assert m and r["info"]["MATEID"] == "bk%s_%d" % (m.group(1), 3 - int(m.group(2))), r
        r["row"], r["side"] = int(m.group(1)), int(m.group(2))
        mate = by_id[r["info"]["MATEID"]]  # every MATEID resolves
        assert (mate["alt"]["mate_chr"], mate["alt"]["mate_pos"]) == (r["CHROM"], r["POS"]), (r, mate)
        assert mate["alt"]["mate_right"] == r["alt"]["own_right"], (r, mate)  # the mate's bracket agrees with where this record's base stands
        assert mate["FILTER"] == r["FILTER"] and mate["FORMAT"] == r["FORMAT"]
    return cols[9:], recs


def assert_other_files_identical(a, b, tmp):
    """every file of run `a` is in run `b`, byte-identical but for the prefix in _params.txt, its new last line and the timings of
    _performance.txt; run `b` has one more file, the VCF"""
    fa = sorted(f[len("a"):] for f in os.listdir(tmp) if f.startswith("a_"))
    fb = sorted(f[len("b"):] for f in os.listdir(tmp) if f.startswith("b_"))
    assert fb == sorted(fa + ["_fusion.vcf"]) and "_fusion.txt" in fa and "_params.txt" in fa, (fa, fb)
    for suffix in fa:
        if suffix == "_params.txt":
            pa, pb = open(a + suffix).read(), open(b + suffix).read()
            assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "vcf\t1\n", (pa, pb)
        elif suffix == "_performance.txt":
            xa, xb = open(a + suffix).read().split("\n"), open(b + suffix).read().split("\n")
            assert xa[0] == xb[0] and xa[1].split("\t")[:5] == xb[1].split("\t")[:5]
        else:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix


def check_vcf_against_abi(path, side, ds, cols, fast, variant, all_rows, fusion_path):
    """every field of every record against bk_fetch, bk_junctions, bk_ref_support, bk_normal_support and bk_genotype_call on the
    same table; returns the records"""
    with_normal, with_gt, with_x = variant.startswith("normal"), variant.endswith("genotype"), variant == "exclude"
    samples, recs = read_vcf(path, ds.contigs)
    assert samples == (["TUMOR", "NORMAL"] if with_normal else ["TUMOR"])
    t = capi.Context(ds.contigs)
    t.upload(cols)
    if with_x:
        t.exclude_regions(*EXCLUDE)
    w, _ = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    junc = t.junctions()
    rsup = t.ref_support(t, QUAL, 10, w) if with_gt else None
    nsup = rsup_n = None
    if with_normal:
        n = capi.Context(ds.contigs)
        n.upload(designed_normal().to_soa())
        n.isize_stats()
        n.discordant_pairs(QUAL, w)
        n.split_evidence()
        nsup = t.normal_support(n, w)
        rsup_n = t.ref_support(n, QUAL, 10, w) if with_gt else None
        n.close()
    t.close()
    # the calls of the fusion table of this run: (BreakPoint1, BreakPoint2) -> (Gene1, Gene2)
    table = {}
    for f in fusion_rows(fusion_path):
        table.setdefault((f[1], f[2], f[7], f[8]), []).append((f[3], f[5]))
    called = set()
    for r in recs:
        c, j = cl[r["row"]], junc[r["row"]]
        s = r["side"]
        assert c["flags"] & 2 and int(c["n_sr"]) > 0
        key = (NAMES[c["p1_tid"]] + ":%d" % c["p1_exact"], NAMES[c["p2_tid"]] + ":%d" % c["p2_exact"], str(c["n_drp"]), str(c["n_sr"]))
        assert key in table, (key, r)
        called.add(key)
        genes = table[key]
        assert all(g == genes[0] for g in genes)
        own = (NAMES[c["p%d_tid" % s]], int(c["p%d_exact" % s]))
        mate = (NAMES[c["p%d_tid" % (3 - s)]], int(c["p%d_exact" % (3 - s)]))
        assert (r["CHROM"], r["POS"]) == own
        assert r["REF"] == nib_base(side["nib"], own[0], own[1])
        right = capi.junction_sides(j)
        assert r["ALT"] == capi.vcf_breakend_alt(r["REF"], right[s - 1], mate[0], mate[1], right[2 - s]), (r, j)
        members = int(j["pairs"].sum())
        exp = dict(SVTYPE="BND", MATEID="bk%d_%d" % (r["row"], 3 - s), EVENTTYPE=fusion_type(int(c["type_mask"])), PE=str(c["n_drp"]), SR=str(c["n_sr"]),
                   MAPQ=str(int(j["mapq_sum%d" % s]) // members if members else 0), DP=str(c["depth%d" % s]), GENE=genes[0][s - 1], SIDES=SOURCE_TEXT[right[2]])
        assert r["info"] == exp, (r["info"], exp)
        no_pair = (genes[0][0] == "intergenic" and genes[0][1] == "intergenic") or genes[0][0] == genes[0][1]
        if not all_rows:
            assert r["FILTER"] == "PASS" and not no_pair
        elif r["FILTER"] != "PASS":
            assert ("NoGenePair" in r["filters"]) == no_pair
        else:
            assert not no_pair

        def sample(n_drp, n_sr, rs):
            if rs is None:
                return dict(DV=str(n_drp), RV=str(n_sr))
            g, gq, _ = capi.genotype_call(n_sr, (int(rs["ref_reads1"]) + int(rs["ref_reads2"]) + 1) // 2)
            return dict(GT=GT_TEXT[g], GQ=str(gq), DR=str(rs["ref_pairs%d" % s]), DV=str(n_drp), RR=str(rs["ref_reads%d" % s]), RV=str(n_sr))
        assert r["FORMAT"] == ("GT:GQ:DR:DV:RR:RV" if with_gt else "DV:RV")
        assert r["samples"][0] == sample(int(c["n_drp"]), int(c["n_sr"]), rsup[r["row"]] if with_gt else None), r
        if with_normal:
            ns = nsup[r["row"]]
            assert r["samples"][1] == sample(int(ns["n_drp"]), int(ns["n_sr"]), rsup_n[r["row"]] if with_gt else None), r
    assert called == set(table), (called, set(table))  # exactly the calls of the fusion table
    assert len(recs) == 2 * sum(len(v) for v in table.values())
    return recs


def designed_alts(recs, nib_dir):
    """the two ALT texts of every designed locus"""
    by_pos = {}
    for r in recs:
        by_pos.setdefault((r["CHROM"], r["POS"]), []).append(r)
    for name, ta, bpa, da, tb, bpb, db in LOCI:
        for (t, bp, d), (mt, mbp, md) in (((ta, bpa, da), (tb, bpb, db)), ((tb, bpb, db), (ta, bpa, da))):
            hits = by_pos.get((NAMES[t], bp))
            assert hits, "locus %s has no record at %s:%d" % (name, NAMES[t], bp)
            base = nib_base(nib_dir, NAMES[t], bp)
            br = "[" if md == "R" else "]"
            mate = "%s%s:%d%s" % (br, NAMES[mt], mbp, br)
            exp = mate + base if d == "R" else base + mate
            assert all(r["ALT"] == exp and r["info"]["SIDES"] == "SR" for r in hits), (name, exp, hits)


@pytest.mark.parametrize("variant", ["gpu_feed", "across_blocks", "host_decode", "exclude", "normal", "normal_genotype"])
@pytest.mark.parametrize("mode", ["fast", "default"])
def test_cli_vcf(mode, variant):
    ds = designed_tumor(mix=False)  # the eight-locus tumour
    cols = ds.to_soa()
    with_normal, with_gt, with_x = variant.startswith("normal"), variant.endswith("genotype"), variant == "exclude"
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb, bed = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "x.bed")
        write_indexed(ds, tb, aligned=variant != "across_blocks")
        side = synth.write_side_files(ds, tmp, refgene_lines=designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        if variant == "host_decode":
            env["BREAKID_HOST_DECODE"] = "1"
        extra = ["-fast"] if mode == "fast" else []
        if with_normal:
            designed_normal().write_bam(nb, aligned=True)
            extra += ["-normal", nb]
        if with_gt:
            extra += ["-genotype"]
        if with_x:
            with open(bed, "w") as f:
                for t, s, e in zip(*EXCLUDE):
                    f.write("%s\t%d\t%d\n" % (NAMES[t], s, e))
            extra += ["-x", bed]
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        r = subprocess.run(base + ["-all", "-o", a], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-all", "-o", b, "-vcf"], env=dict(env, BK_DEBUG="feed"), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        feeds = [l for l in r.stderr.split("\n") if l.startswith("[feed/gpu]") and "file -> device table" in l]
        if variant == "host_decode":
            assert not feeds, feeds
        elif not with_x:
            assert len(feeds) == 1 + with_normal and ("records across blocks" in feeds[0]) == (variant == "across_blocks"), feeds
        assert_other_files_identical(a, b, tmp)
        recs = check_vcf_against_abi(b + "_fusion.vcf", side, ds, cols, mode == "fast", variant, True, b + "_fusion_all.txt")
        designed_alts(recs, side["nib"])
        assert sum(r["FILTER"] == "PASS" for r in recs) >= 8 and any(r["FILTER"] == "NoGenePair" for r in recs)
        if shutil.which("bcftools"):
            assert subprocess.run(["bcftools", "view", b + "_fusion.vcf"], capture_output=True).returncode == 0
        if variant in ("gpu_feed", "normal_genotype"):
            # two runs give the same bytes; without -all only PASS rows and exactly the calls of _fusion.txt
            c, d = os.path.join(tmp, "c"), os.path.join(tmp, "d")
            r = subprocess.run(base + ["-all", "-o", c, "-vcf"], env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            assert open(c + "_fusion.vcf", "rb").read() == open(b + "_fusion.vcf", "rb").read()
            r = subprocess.run(base + ["-o", d, "-vcf"], env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            assert not os.path.exists(d + "_fusion_all.txt")
            kept = check_vcf_against_abi(d + "_fusion.vcf", side, ds, cols, mode == "fast", variant, False, d + "_fusion.txt")
            assert len(kept) >= 8 and all(r["FILTER"] == "PASS" for r in kept)
            assert "NoGenePair" not in open(d + "_fusion.vcf").read()
            assert [r for r in recs if r["FILTER"] == "PASS"] == kept


def test_cli_vcf_of_a_sample_without_calls_and_errors():
    tum = quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        r = subprocess.run(base + ["-vcf", "-gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-vcf cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        samples, recs = read_vcf(prefix + "_fusion.vcf", tum.contigs)
        assert samples == ["TUMOR"] and recs == []
        assert open(prefix + "_fusion.vcf").read().endswith("\tFORMAT\tTUMOR\n")
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\n")
        nb = os.path.join(tmp, "n.bam")
        designed_normal().write_bam(nb, aligned=True)
        r = subprocess.run(base + ["-vcf", "-normal", nb, "-genotype"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        samples, recs = read_vcf(prefix + "_fusion.vcf", tum.contigs)
        assert samples == ["TUMOR", "NORMAL"] and recs == []

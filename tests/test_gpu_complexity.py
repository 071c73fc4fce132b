"""Site complexity (`bk_site_complexity`, `-complexity`): the kernel against the Python definition (tests/complexitycases.py) byte for
byte on either side of every word boundary of the bit planes and at both ends of the ranges of flank and period; designed edges; two
runs and a permuted site list; errors, limits and empty inputs; timing; and the command line's files against the definition."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc
from tests import complexitycases as xc
from tests import homologycases as hc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL


@pytest.fixture(scope="module")
def ctx():
    t = capi.Context(cc.CONTIGS)  # any live context: no table, no stage
    yield t
    t.close()


def assert_rows(got, exp):
    assert got.dtype == abi.SITE_CPLX and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def tract(row, name):
    return tuple(int(row[name + f]) for f in ("_len", "_period", "_start"))


# ---- 1. the kernel against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flank", [1, 2, 31, 32, 33, 63, 64, 95, 96, 127, 128, 255])
def test_complexity_equals_its_definition(ctx, flank):
    ref, sites, plan = xc.random_case(flank, 200 if flank <= 64 else 48)
    L = 2 * flank + 1
    xc.assert_plan(plan, L)
    for max_period in (6, 1, 63, 64):
        got = ctx.site_complexity(ref, sites, flank, max_period)
        assert_rows(got, xc.expected_cplx(ref, sites, flank, max_period))
        found = plan["clean"] & (plan["period"] <= max_period)
        assert found.any() and (got["max_len"][found] >= plan["length"][found]).all()  # every planted tract is seen
        at = found & plan["covers"]
        assert at.any() and (got["bp_len"][at] >= plan["length"][at]).all()  # ... and at the breakpoint where it covers column R
        assert not got["reserved"].any()
    got = ctx.site_complexity(ref, sites, flank)  # the defaults' max_period
    assert_rows(got, xc.expected_cplx(ref, sites, flank, 6))
    if L >= 24:
        assert (got["max_len"][plan["clean"]] >= 24).all() and (got["mask_run"] > 0).sum() * 4 >= len(sites)


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    # a period at or above L: no tract of it and no error
    ref = xc.text_ref(["AAA", "ACGTACGTACGT"])
    sites = xc.as_sites([(0, 2), (1, 2)])
    got = ctx.site_complexity(ref, sites, 1, 64)
    assert_rows(got, xc.expected_cplx(ref, sites, 1, 64))
    assert tract(got[0], "max") == (3, 1, 0) and tract(got[1], "max") == (0, 0, 0)
    for R in (1, 2, 32, 100, 255):
        L = 2 * R + 1
        # a tract that is the whole window; mask_run that reaches both ends of it
        ref = xc.text_ref(["A" * 600, ("ca" * 300), ("CAG" * 200)])
        sites = xc.as_sites([(0, 300), (1, 300), (2, 300)])
        got = ctx.site_complexity(ref, sites, R, 6)
        assert_rows(got, xc.expected_cplx(ref, sites, R, 6))
        assert tract(got[0], "max") == tract(got[0], "bp") == (L, 1, 0) and int(got[0]["tri_pairs"]) == (L - 2) * (L - 3) // 2 and int(got[0]["tri_distinct"]) == 1
        assert int(got[1]["mask_run"]) == int(got[1]["masked"]) == L and int(got[0]["mask_run"]) == 0
        if L >= 4:
            assert tract(got[1], "max") == tract(got[1], "bp") == (L, 2, 0)
        if L >= 6:
            assert tract(got[2], "max") == (L, 3, 0)
        # a tract that ends in the window's last column, and one in its first; neither touches the breakpoint when R >= 32
        if R >= 2:
            n = min(R - 1, 30)
            text = ("CGT" * 200)[:300 + R - n] + "A" * n + ("CGT" * 100)
            ref = xc.text_ref([text])
            sites = xc.as_sites([(0, 300), (0, 300 + 2 * R - n + 1)])  # the run: the last n columns of the first window, the first n of the second
            got = ctx.site_complexity(ref, sites, R, 1)
            assert_rows(got, xc.expected_cplx(ref, sites, R, 1))
            assert tract(got[0], "max") == (n, 1, L - n) if n >= 2 else tract(got[0], "max") == (0, 0, 0)
            if n >= 2:
                assert tract(got[1], "max") == (n, 1, 0)
            if R >= 32:
                assert tract(got[0], "bp") == tract(got[1], "bp") == (0, 0, 0)
        # N in all four codes and masked N, segments that abut, a gap, odd lengths, soft-masked bases (homologycases.edge_table); a site
        # at position 1, at the contig's last base and beyond it; position 0; tid -1; a contig without a segment
        eref, _, _ = hc.edge_table()
        rows = [(0, 1), (0, hc.LENGTHS[0]), (0, hc.LENGTHS[0] + R), (1, 1), (1, hc.LENGTHS[1]), (0, 0), (-1, 300), (2, 300), (3, 11), (3, 12), (0, 301), (0, 400), (0, 470), (0, 520)]
        rows += [(0, int(p)) for p in np.random.default_rng(R).integers(1, 760, 40)] + [(1, int(p)) for p in np.random.default_rng(R + 1).integers(1, 800, 20)]
        sites = xc.as_sites(rows)
        got = ctx.site_complexity(eref, sites, R, 6)
        exp = xc.expected_cplx(eref, sites, R, 6)
        assert_rows(got, exp)
        assert int(got[0]["covered"]) == R + 1 and int(got[1]["covered"]) == R + 1 and int(got[2]["covered"]) == 1
        assert not got[6:8].tobytes().strip(b"\0")
        assert (got["covered"] > got["valid"]).any() and (got["masked"] > 0).any()
        # an empty table: every row zero
        none = ctx.site_complexity(hc.make_refseq([]), sites, R, 6)
        assert len(none) == len(sites) and not none.tobytes().strip(b"\0")
    # the N codes 4 .. 7 and their masked forms 12 .. 15, by hand
    ref = hc.make_refseq([(0, 0, np.asarray([2, 4, 5, 6, 7, 12, 13, 14, 15, 2, 9], np.uint8))])
    r = ctx.site_complexity(ref, xc.as_sites([(0, 6)]), 5, 6)[0]
    assert (int(r["covered"]), int(r["valid"]), int(r["masked"]), int(r["mask_run"]), int(r["tri_total"]), int(r["max_len"])) == (11, 3, 5, 4, 0, 0)


# ---- 3. same bytes -------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_permuted_site_list_give_the_same_bytes(ctx):
    ref, sites, _ = xc.random_case(64, 200)
    first = ctx.site_complexity(ref, sites, 64, 6)
    again = ctx.site_complexity(ref, sites, 64, 6)
    perm = np.random.default_rng(9).permutation(len(sites))
    moved = ctx.site_complexity(ref, sites[perm], 64, 6)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()


# ---- 4. errors, limits, empty inputs -------------------------------------------------------------------------------------------------
def raw_call(t, ref, sites, flank, max_period=6, n=None, n_segs=None, null=()):
    C = capi.C
    s, keep = capi.refseq_struct(ref)
    if n_segs is not None:
        s.n_segs = n_segs
    sites = np.ascontiguousarray(sites, abi.REF_SITE)
    out = C.c_void_p()
    rc = t.L.bk_site_complexity(None if "ctx" in null else t.h, None if "ref" in null else C.byref(s), None if "sites" in null else sites.ctypes.data,
                                len(sites) if n is None else n, flank, max_period, None if "out" in null else C.byref(out))
    del keep
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_and_limit_errors(ctx):
    ref, _, _ = hc.edge_table()
    sites = xc.as_sites([(0, 100), (1, 100), (0, 450), (3, 100), (1, 5), (0, 390)])
    assert raw_call(ctx, ref, sites, 32)[0] == abi.BK_OK
    for null in ("ctx", "ref", "sites", "out"):
        assert raw_call(ctx, ref, sites, 32, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(ctx, ref, sites, 32, n=0, null=("sites",))[0] == abi.BK_OK
    for flank in (0, 256):
        rc, msg = raw_call(ctx, ref, sites, flank)
        assert rc == abi.BK_ERR_ARG and "flank" in msg, msg
    for period in (0, 65):
        rc, msg = raw_call(ctx, ref, sites, 32, period)
        assert rc == abi.BK_ERR_ARG and "max_period" in msg, msg
    for flank, period in ((1, 1), (255, 64), (1, 64)):
        assert raw_call(ctx, ref, sites, flank, period)[0] == abi.BK_OK

    def with_col(name, index, value):
        r = dict(ref)
        r[name] = ref[name].copy()
        r[name][index] = value
        return r
    for bad, word in ((with_col("start", 1, 300), "overlaps"), (with_col("start", 2, 0), "out of order"), (with_col("tid", 0, 2), "out of order"),
                      (with_col("off", 3, int(ref["off"][2]) - 1), "off does not ascend"), (with_col("len", 3, 2 * int(ref["off"][4] - ref["off"][3]) + 1), "fewer bytes")):
        rc, msg = raw_call(ctx, bad, sites, 32)
        assert rc == abi.BK_ERR_ARG and word in msg and "bk_site_complexity" in msg, msg
    # the limits are looked at before any array: the small ones are never read beyond their end
    rc, msg = raw_call(ctx, ref, sites, 32, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg, msg
    rc, msg = raw_call(ctx, ref, sites, 32, n_segs=(1 << 20) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^20 segments" in msg, msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.site_complexity(ref, sites)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.site_complexity(ref, sites, 32, 6), xc.expected_cplx(ref, sites, 32, 6))  # the context still works, on the edge table too
    none = ctx.site_complexity(ref, np.zeros(0, abi.REF_SITE))
    assert len(none) == 0 and none.dtype == abi.SITE_CPLX


# ---- 5. timing -----------------------------------------------------------------------------------------------------------------------
def test_complexity_is_timed():
    ref, sites, _ = xc.random_case(96, 48)
    t = capi.Context(cc.CONTIGS)
    t.timing_enable(True)
    t.site_complexity(ref, sites, 96, 6)
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "site_complexity" in tm and tm["site_complexity"][0] > 0 and tm["site_complexity"][1] > 0
    assert touched["site_complexity"] == len(sites) * (72 + 2 * 96 + 1)  # the site row, the result row, L nibbles
    t.close()


# ---- 6. command line -----------------------------------------------------------------------------------------------------------------
INFO_LINES = ("##INFO=<ID=LCDUST,Number=1,Type=Float,", "##INFO=<ID=LCGC,Number=1,Type=Float,", "##INFO=<ID=LCMASK,Number=1,Type=Float,", "##INFO=<ID=LCSTR,Number=1,Type=String,")
CA_SITE, CA_FIRST = (0, 300_000), 299_985      # (CA)20 over chr1 299 985 .. 300 024, around the first designed locus
MASK_SITE, MASK_FIRST = (0, 600_000), 599_900  # chr1 599 900 .. 600 099 soft-masked, around the second
POLY_SITE, POLY_FIRST, POLY_N = (2, 900_000), 899_990, 25  # 25 A from chr3 899 990 on, around the fourth


class MaskedGenome(hc.Genome):
    """homologycases.Genome with soft-masked intervals [(tid, first, last)], 1-based and inclusive"""

    def __init__(self, lengths, patches=None, masked=()):
        super().__init__(lengths, patches)
        self.masked = list(masked)

    def nibbles(self, tid, start0, n):
        nib = super().nibbles(tid, start0, n).copy()
        for t, a, b in self.masked:
            lo, hi = max(a - 1 - start0, 0), min(b - start0, n)
            if t == tid and lo < hi:
                nib[lo:hi] |= 8
        return nib


def planted_genome():
    """homologycases.genome() with the dinucleotide tract, the homopolymer and the soft-masked interval; the base on either side of a
    tract is one that does not extend it"""
    patches = dict(hc.genome().patches)
    for j in range(40):
        patches[(CA_SITE[0], CA_FIRST + j)] = "CA"[j % 2]
    patches[(CA_SITE[0], CA_FIRST - 1)] = patches[(CA_SITE[0], CA_FIRST + 40)] = "G"
    for j in range(POLY_N):
        patches[(POLY_SITE[0], POLY_FIRST + j)] = "A"
    patches[(POLY_SITE[0], POLY_FIRST - 1)] = patches[(POLY_SITE[0], POLY_FIRST + POLY_N)] = "C"
    return MaskedGenome(hc.LENGTHS, patches, [(MASK_SITE[0], MASK_FIRST, MASK_FIRST + 199)])


@pytest.fixture(scope="module")
def cx_run():
    """the designed BAM with its side files and nib files written from the planted genome: one directory with every contig, one
    without chr2"""
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "t.bam")
        hc.write_plus_bam(bam)
        bamio.write_bai(bam)
        ds = hc.designed_plus()["ds"]
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        g = planted_genome()
        hc.write_nib_dir(side["nib"], g)
        less = os.path.join(tmp, "nib_less")
        os.makedirs(less)
        shutil.copy(os.path.join(side["nib"], "ref_names.txt"), less)
        for tid, (name, _) in enumerate(cc.CONTIGS):
            if tid != 1:
                shutil.copy(os.path.join(side["nib"], "hg19_%s.nib" % name), less)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        t = capi.Context(ds.contigs)
        t.upload(ds.to_soa())
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        t.close()
        yield {"tmp": tmp, "bam": bam, "nib": side["nib"], "nib_less": less, "env": env, "cl": cl, "genome": g}


def expected_fields(run, calls, flank, max_period, no_nib=()):
    """{call: [the twelve fields of side 1, those of side 2]} for the calls (rows of BK_STAGE_CLUSTERS), from the definition on the
    genome itself"""
    cl, g = run["cl"], run["genome"]
    rows = [(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"])) for i in calls]
    probes = hc.as_probes([(r[0], r[1], 0, r[2], r[3], 0, 0) for r in rows])
    ref = g.refseq(hc.merged_windows(probes, flank + 2, hc.LENGTHS))
    sites = xc.as_sites([(r[2 * s], r[2 * s + 1]) for r in rows for s in (0, 1)])
    cx = xc.expected_cplx(ref, sites, flank, max_period)
    out = {}
    for k, i in enumerate(calls):
        out[i] = [xc.twin_fields(ref, sites[2 * k + s], flank, None if rows[k][2 * s] in no_nib else cx[2 * k + s]) for s in (0, 1)]
    return out


def by_position(cl, calls):
    return {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}


def side_at(cl, seen, site):
    """the fields of the one side of a call that lies at `site`"""
    hit = [seen[i][s] for i in seen for s in (0, 1) if (int(cl[i]["p%d_tid" % (s + 1)]), int(cl[i]["p%d_exact" % (s + 1)])) == site]
    assert len(hit) == 1, site
    return hit[0]


@pytest.mark.parametrize("variant", ["plain", "everything"])
def test_cli_complexity(cx_run, variant):
    run = cx_run
    tmp, cl = run["tmp"], run["cl"]
    flank, period = (32, 6) if variant == "plain" else (100, 4)
    extra = [] if variant == "plain" else ["-vcf", "-consensus", "-homology", "-similar", "-clip", "-dedup", "-genotype", "-evidence"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-all", "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-complexity"] + ([] if variant == "plain" else ["-cplxflank", "100", "-cplxperiod", "4"]), env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_complexity.txt", "_fusion_complexity.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt", "_fusion.vcf"}
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    if variant == "everything":
        assert {"_fusion_consensus.txt", "_fusion_homology.txt", "_fusion_similar.txt", "_fusion_rescued.vcf", "_evidence.txt", "_fusion.vcf"} <= set(fa)
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "complexity_flank\t%d\ncomplexity_max_period\t%d\n" % (flank, period), (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's twelve fields of either side
    seen = {}
    for twin in twins:
        plain = twin.replace("_complexity", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(xc.COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) >= (3 if plain == "_fusion.txt" else 11)
        by_key = by_position(cl, calls)
        exp = expected_fields(run, calls, flank, period)
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            assert line == s + "\t" + "\t".join(exp[i][0] + exp[i][1]), (line, exp[i])
        seen.update(exp)
    # the three designed sites by their designed values
    L = 2 * flank + 1
    f = side_at(cl, seen, CA_SITE)
    assert f[6:9] == ["CA", "40", str(CA_FIRST)] and f[9:] == f[6:9] and f[0] == str(L) and f[4:6] == ["0.000", "0"] and float(f[2]) > (3.0 if flank == 32 else 1.0), f
    f = side_at(cl, seen, POLY_SITE)
    assert f[6:9] == ["A", str(POLY_N), str(POLY_FIRST)] and f[9:] == f[6:9] and f[4:6] == ["0.000", "0"], f
    f = side_at(cl, seen, MASK_SITE)
    run_len = min(MASK_SITE[1] + flank, MASK_FIRST + 199) - max(MASK_SITE[1] - flank, MASK_FIRST) + 1
    assert f[4:6] == ["%.3f" % (run_len / L), str(run_len)] and run_len == (65 if flank == 32 else 200) and int(f[7]) < 12, f
    others = [x for i in seen for s, x in enumerate(seen[i]) if (int(cl[i]["p%d_tid" % (s + 1)]), int(cl[i]["p%d_exact" % (s + 1)])) not in (CA_SITE, POLY_SITE, MASK_SITE)]
    assert len(others) >= 19 and all(x[4:6] == ["0.000", "0"] and int(x[10]) < 20 and x[0] == str(L) for x in others)  # what random windows hold
    # the log line counts the sites, the tracts of 12 columns or more at a breakpoint and the soft-masked breakpoint bases
    n_sites = 2 * len(written_calls(cl, b + "_fusion_all.txt"))
    assert r.stdout.count("complexity: ") == 1 and "complexity: " not in out_a
    assert "complexity: %d sites, 2 with a tract of 12 or more columns at the breakpoint, 1 with the breakpoint base soft-masked\n" % n_sites in r.stdout, r.stdout[-1500:]
    # 3. the VCF: the keys last in INFO on each breakend, for its own side; their four header lines; nothing else touched
    if variant == "plain":
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 4 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == n_sites
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        tail = xc.info_tail(seen[i][s])
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail and tail.startswith(";LCDUST=") and ";LCGC=" in tail and ";LCMASK=" in tail, lb
    assert sum(l.split("\t")[7].endswith(";LCSTR=CAx40") for l in body_b) == 1 and sum(l.split("\t")[7].endswith(";LCSTR=Ax%d" % POLY_N) for l in body_b) == 1
    assert sum(";LCMASK=0.995" in l for l in body_b) == 1
    assert open(a + "_fusion_rescued.vcf", "rb").read() == open(b + "_fusion_rescued.vcf", "rb").read()


def test_cli_complexity_without_calls_without_a_nib_file_and_errors(cx_run):
    run = cx_run
    tmp, cl = run["tmp"], run["cl"]
    # a contig without a nib file: the sides on it print "." and lose their keys, the other side of the call keeps its values
    c = os.path.join(tmp, "c")
    r = subprocess.run([BIN, "-i", run["bam"], "-n", run["nib_less"], "-o", c, "-all", "-fast", "-complexity", "-vcf"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = written_calls(cl, c + "_fusion_all.txt")
    exp = expected_fields(run, calls, 32, 6, no_nib=(1,))
    lines, src = open(c + "_fusion_all_complexity.txt").read().split("\n"), open(c + "_fusion_all.txt").read().split("\n")
    by_key = by_position(cl, calls)
    dotted = half = 0
    for line, s in zip(lines[1:-1], src[1:-1]):
        f = line.split("\t")
        i = by_key[(f[1], f[2])]
        assert line == s + "\t" + "\t".join(exp[i][0] + exp[i][1]), line
        on_one = [int(cl[i]["p1_tid"]) == 1, int(cl[i]["p2_tid"]) == 1]
        assert [f[-24:-12] == ["."] * 12, f[-12:] == ["."] * 12] == on_one
        dotted += sum(on_one)
        half += sum(on_one) == 1
    assert 3 <= dotted < 2 * len(calls) and half >= 2
    assert "complexity: %d sites," % (2 * len(calls) - dotted) in r.stdout
    body = [l.split("\t") for l in open(c + "_fusion.vcf").read().split("\n") if l and not l.startswith("#")]
    assert len(body) == 2 * len(calls)
    for y in body:
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        submitted = int(cl[i]["p%d_tid" % (s + 1)]) != 1
        assert all((k in y[7]) == submitted for k in (";LCDUST=", ";LCGC=", ";LCMASK=")) and (submitted or ";LCSTR=" not in y[7]), y
        assert y[7].endswith(xc.info_tail(exp[i][s]))
    # a sample without calls, and the option rules
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp2:
        tb = os.path.join(tmp2, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp2)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp2, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-cplxflank", "100"], "-cplxflank needs -complexity."), (["-cplxperiod", "4"], "-cplxperiod needs -complexity."),
                           (["-complexity", "-gpus", "2"], "-complexity cannot be combined with -gpus."),
                           (["-complexity", "-cplxflank", "0"], "-cplxflank must be a number from 1 to 255."),
                           (["-complexity", "-cplxflank", "256"], "-cplxflank must be a number from 1 to 255."),
                           (["-complexity", "-cplxperiod", "0"], "-cplxperiod must be a number from 1 to 64."),
                           (["-complexity", "-cplxperiod", "65"], "-cplxperiod must be a number from 1 to 64.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp2))
        r = subprocess.run(base + ["-complexity", "-vcf", "-cplxflank", "255", "-cplxperiod", "64"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_complexity.txt", "_fusion_all_complexity.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(xc.COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\ncomplexity_flank\t255\ncomplexity_max_period\t64\n")
        assert "complexity: 0 sites, 0 with a tract of 12 or more columns at the breakpoint, 0 with the breakpoint base soft-masked\n" in r.stdout

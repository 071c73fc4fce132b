"""Locus similarity (`bk_locus_similarity`, `-similar`): the kernel against the Python definition (tests/similarcases.py) byte for byte
at every word boundary of the bit planes and both ends of the flank's range; the excluded diagonal; the tie rules on repeats; pairs
with nothing to find; two runs and a permuted pair list; errors, limits and empty inputs; timing; and the command line's files
against the definition."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc
from tests import homologycases as hc
from tests import similarcases as sc
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
    assert got.dtype == abi.LOCUS_SIM and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


# ---- 1. the kernel against the definition ------------------------------------------------------------------------------------------
SEEN = set()  # (orient, diag >= 0) of the planted pairs that were found, over all flanks


@pytest.mark.parametrize("flank", [1, 2, 31, 32, 33, 63, 64, 95, 96, 127, 128, 255])
def test_similarity_equals_its_definition(ctx, flank):
    ref, pairs, planted = sc.random_case(flank, 200 if flank <= 64 else 48)
    got = ctx.locus_similarity(ref, pairs, flank)
    exp = sc.expected_sim(ref, pairs, flank)
    assert_rows(got, exp)
    assert planted.sum() >= 2 * len(pairs) // 5 and (got["found"][planted] == 1).all()  # every planted pair is found
    combos = {(int(r["orient"]), int(r["diag"]) >= 0) for r in got[planted]}
    SEEN.update(combos)
    if flank >= 31:
        assert len(combos) == 4, combos  # both orientations, diagonals of either sign
        assert (got["score"][planted] > 12).sum() > planted.sum() // 2  # ... and not as background
    if flank == 255:
        assert len(SEEN) == 4


# ---- 2. the excluded diagonal ------------------------------------------------------------------------------------------------------
def test_excluded_diagonal(ctx):
    rng = np.random.default_rng(31)
    codes = rng.integers(0, 4, 3000)
    rnd = sc.codes_to_ref([codes, codes])  # contig 1 holds the same bases as contig 0
    di, _ = hc.repeat_ref("AC", 3000)
    for R in (1, 31, 32, 100, 255):
        L = 2 * R + 1
        apart = [0, 1, -1, R, -R, 2 * R, -2 * R, 2 * R + 1, -(2 * R + 1)]
        same = sc.as_pairs([(0, 1500, 0, 1500 - a) for a in apart])
        other = sc.as_pairs([(0, 1500, 1, 1500 - a) for a in apart])
        for ref in (rnd, di):
            got = ctx.locus_similarity(ref, same, R)
            assert_rows(got, sc.expected_sim(ref, same, R))
        got = ctx.locus_similarity(rnd, same, R)
        if R >= 31:
            # the base-against-itself diagonal is never reported, and with pos_a == pos_b the result is background, not L
            assert not any(int(r["orient"]) == 0 and int(r["found"]) and int(r["diag"]) == a for r, a in zip(got, apart))
            assert 0 < int(got[0]["score"]) < 30
        # the same positions on two different tids score the whole overlap of the windows
        two = ctx.locus_similarity(rnd, other, R)
        assert_rows(two, sc.expected_sim(rnd, other, R))
        for r, a in zip(two, apart):
            n = L - abs(a)
            if n >= 30:
                assert (int(r["score"]), int(r["len"]), int(r["run"]), int(r["diag"]), int(r["orient"]), int(r["start"])) == (n, n, n, a, 0, max(0, -a)), (R, a, r)
        assert (int(two[0]["score"]), int(two[0]["len"])) == (L, L)
        # the dinucleotide: with pos_a == pos_b the neighbouring diagonal |d| = 2 wins, the non-negative one first
        r = ctx.locus_similarity(di, same[:1], R)[0]
        if R >= 2:
            assert (int(r["diag"]), int(r["orient"]), int(r["score"]), int(r["len"]), int(r["start"]), int(r["run"])) == (2, 0, L - 2, L - 2, 0, L - 2)


# ---- 3. tie rules ----------------------------------------------------------------------------------------------------------------------
def repeat_contigs(unit, n=1200):
    """three contigs: the unit repeated, the same again, and its complement base by base"""
    c = np.asarray(["ACGT".index(x) for x in (unit * n)[:n]], np.int64)
    return hc.make_refseq([(0, 0, hc.NIB_OF[c]), (1, 0, hc.NIB_OF[c]), (2, 0, hc.NIB_OF[sc.COMP[c]])])


def fields(r):
    return tuple(int(r[f]) for f in ("score", "len", "diag", "orient", "start"))


def test_tie_rules_on_repeats(ctx):
    poly, di, pal = repeat_contigs("A"), repeat_contigs("AC"), repeat_contigs("AT")
    for R in (1, 32, 100):
        L = 2 * R + 1
        pairs = sc.as_pairs([(0, 600, 1, 600), (0, 600, 1, 601), (0, 600, 0, 600), (0, 600, 0, 700), (0, 600, 2, 600), (0, 600, 2, 601), (0, 3, 1, 600), (0, 600, 1, 1199)])
        rows = {}
        for name, ref in (("poly", poly), ("di", di), ("pal", pal)):
            rows[name] = ctx.locus_similarity(ref, pairs, R)
            assert_rows(rows[name], sc.expected_sim(ref, pairs, R))
        got = rows["poly"]
        assert fields(got[0]) == (L, L, 0, 0, 0)  # poly-A on two contigs: every diagonal is clean, the longest one scores highest
        # the same contig: the main diagonal is excluded; d = 1 and d = -1 tie at L - 1 with |d| equal, and d >= 0 decides
        assert fields(got[2]) == (L - 1, L - 1, 1, 0, 0)
        assert fields(got[4]) == (L, L, 0, 1, 0)  # poly-A against poly-T: only the reverse complement matches
        if R >= 32:
            # window A runs over the contig's start and has R + 3 bases: the diagonals -(R - 2) .. 0 hold them all; |d| smallest decides
            assert fields(got[6]) == (R + 3, R + 3, 0, 0, R - 2)
        got = rows["di"]
        assert fields(got[0]) == (L, L, 0, 0, 0)
        assert fields(got[1]) == (L - 1, L - 1, 1, 0, 0)  # one base apart: the odd diagonals are clean, 1 and -1 tie, d >= 0 decides
        assert fields(got[4]) == (L, L, 0, 1, 0)           # AC against TG: the reverse complement of TG.. reads AC.. again
        # AT repeats are their own reverse complement: both orientations have a clean diagonal of L columns, and + stands first
        assert fields(rows["pal"][0]) == (L, L, 0, 0, 0)
    # the shortest segment and the smallest start: AA C AA against AA G AA: on d = 0 the whole scores 4 - 2 = 2 as each AA does
    ref = sc.codes_to_ref([np.asarray([0, 0, 1, 0, 0], np.int64), np.asarray([0, 0, 2, 0, 0], np.int64)])
    pairs = sc.as_pairs([(0, 3, 1, 3)])
    got = ctx.locus_similarity(ref, pairs, 2)
    assert_rows(got, sc.expected_sim(ref, pairs, 2))
    assert fields(got[0]) == (2, 2, 0, 0, 0) and int(got[0]["mism"]) == 0 and int(got[0]["run"]) == 2
    # + before -, then d >= 0: AAA C GGG C AAA against TTTT AAA TTTT, whose reverse complement AAAA TTT AAAA holds AAA as well
    ref = sc.codes_to_ref([np.asarray([0, 0, 0, 1, 2, 2, 2, 1, 0, 0, 0], np.int64), np.asarray([3, 3, 3, 3, 0, 0, 0, 3, 3, 3, 3], np.int64)])
    pairs = sc.as_pairs([(0, 6, 1, 6)])
    got = ctx.locus_similarity(ref, pairs, 5)
    assert_rows(got, sc.expected_sim(ref, pairs, 5))
    assert fields(got[0]) == (3, 3, 4, 0, 0)


# ---- 4. nothing to find --------------------------------------------------------------------------------------------------------------
def test_nothing_to_find(ctx):
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 4, 900)
    ref = hc.make_refseq([(0, 0, hc.NIB_OF[codes]), (1, 0, hc.NIB_OF[np.full(900, 4, np.int64)]), (3, 0, hc.NIB_OF[codes])])  # contig 1: N; contig 2: no segment
    pairs = sc.as_pairs([(-1, 400, 0, 400), (0, 400, -1, 400), (0, 400, 1, 400), (1, 400, 0, 400), (0, 400, 2, 400), (2, 400, 2, 400), (0, 5000, 3, 400), (0, 400, 3, 400)])
    for R in (1, 150, 255):
        got = ctx.locus_similarity(ref, pairs, R)
        assert_rows(got, sc.expected_sim(ref, pairs, R))
        assert not got[:7].tobytes().strip(b"\0") and int(got[7]["score"]) == 2 * R + 1
        none = ctx.locus_similarity(hc.make_refseq([]), pairs, R)
        assert len(none) == len(pairs) and not none.tobytes().strip(b"\0")
    ref2, pairs2, _ = sc.random_case(33, 200)
    assert_rows(ctx.locus_similarity(ref2, pairs2, 33), sc.expected_sim(ref2, pairs2, 33))  # the context still works


# ---- 5. same bytes -------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_permuted_pair_list_give_the_same_bytes(ctx):
    ref, pairs, _ = sc.random_case(64, 200)
    first = ctx.locus_similarity(ref, pairs, 64)
    again = ctx.locus_similarity(ref, pairs, 64)
    perm = np.random.default_rng(9).permutation(len(pairs))
    moved = ctx.locus_similarity(ref, pairs[perm], 64)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()


# ---- 6. errors, limits, empty inputs -------------------------------------------------------------------------------------------------
def raw_call(t, ref, pairs, flank, n=None, n_segs=None, null=()):
    C = capi.C
    s, keep = capi.refseq_struct(ref)
    if n_segs is not None:
        s.n_segs = n_segs
    pairs = np.ascontiguousarray(pairs, abi.LOCUS_PAIR)
    out = C.c_void_p()
    rc = t.L.bk_locus_similarity(None if "ctx" in null else t.h, None if "ref" in null else C.byref(s), None if "pairs" in null else pairs.ctypes.data,
                                 len(pairs) if n is None else n, flank, None if "out" in null else C.byref(out))
    del keep
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_and_limit_errors(ctx):
    ref, _, _ = hc.edge_table()
    pairs = sc.as_pairs([(0, 100, 1, 100), (0, 450, 3, 100), (1, 5, 0, 390)])
    assert raw_call(ctx, ref, pairs, 150)[0] == abi.BK_OK
    for null in ("ctx", "ref", "pairs", "out"):
        assert raw_call(ctx, ref, pairs, 150, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(ctx, ref, pairs, 150, n=0, null=("pairs",))[0] == abi.BK_OK
    for flank in (0, 256):
        rc, msg = raw_call(ctx, ref, pairs, flank)
        assert rc == abi.BK_ERR_ARG and "flank" in msg, msg

    def with_col(name, index, value):
        r = dict(ref)
        r[name] = ref[name].copy()
        r[name][index] = value
        return r
    for bad, word in ((with_col("start", 1, 300), "overlaps"), (with_col("start", 2, 0), "out of order"), (with_col("tid", 0, 2), "out of order"),
                      (with_col("off", 3, int(ref["off"][2]) - 1), "off does not ascend"), (with_col("len", 3, 2 * int(ref["off"][4] - ref["off"][3]) + 1), "fewer bytes")):
        rc, msg = raw_call(ctx, bad, pairs, 150)
        assert rc == abi.BK_ERR_ARG and word in msg and "bk_locus_similarity" in msg, msg
    # the limits are looked at before any array: the small ones are never read beyond their end
    rc, msg = raw_call(ctx, ref, pairs, 150, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 pairs" in msg, msg
    rc, msg = raw_call(ctx, ref, pairs, 150, n_segs=(1 << 20) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^20 segments" in msg, msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.locus_similarity(ref, pairs)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.locus_similarity(ref, pairs, 150), sc.expected_sim(ref, pairs, 150))  # the context still works, on the edge table too
    none = ctx.locus_similarity(ref, np.zeros(0, abi.LOCUS_PAIR))
    assert len(none) == 0 and none.dtype == abi.LOCUS_SIM


# ---- 7. timing -----------------------------------------------------------------------------------------------------------------------
def test_similarity_is_timed():
    ref, pairs, _ = sc.random_case(96, 48)
    t = capi.Context(cc.CONTIGS)
    t.timing_enable(True)
    t.locus_similarity(ref, pairs, 96)
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "locus_similarity" in tm and tm["locus_similarity"][0] > 0 and tm["locus_similarity"][1] > 0
    assert touched["locus_similarity"] == len(pairs) * (48 + 2 * 96 + 1)  # the pair row, the result row, L nibbles of each window
    t.close()


# ---- 8. command line -----------------------------------------------------------------------------------------------------------------
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=Integer," % k for k in ("SIMSCORE", "SIMLEN", "SIMRUN"))
FWD = (0, 300_000, 1, 700_000)  # the first designed locus: 80 bases of chr1 from 299 950 on lie at chr2 699 970, three of them substituted
REV = (2, 900_000, 3, 400_000)  # the fourth: 80 bases of chr3 from 899 980 on lie reverse-complemented at chr4 399 960


def planted_genome():
    """homologycases.genome() with the two copies; the bases around a copy are made unlike what would extend it"""
    g = hc.genome()
    plain = hc.Genome(hc.LENGTHS, g.patches)
    patches = dict(g.patches)
    src = plain.codes(0, 299_950 + np.arange(-1, 81))  # one base more on either side
    for j in range(80):
        c = int(src[1 + j])
        patches[(1, 699_970 + j)] = "ACGT"[(c + 1) % 4 if j in (20, 40, 60) else c]
    patches[(1, 699_969)], patches[(1, 700_050)] = "ACGT"[(int(src[0]) + 2) % 4], "ACGT"[(int(src[81]) + 2) % 4]
    src = plain.codes(2, 899_980 + np.arange(-1, 81))
    for j in range(80):
        patches[(3, 399_960 + j)] = "ACGT"[3 - int(src[80 - j])]
    patches[(3, 399_959)], patches[(3, 400_040)] = "ACGT"[(3 - int(src[81]) + 2) % 4], "ACGT"[(3 - int(src[0]) + 2) % 4]
    return hc.Genome(hc.LENGTHS, patches)


@pytest.fixture(scope="module")
def sim_run():
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


def expected_fields(run, calls, flank, no_nib=()):
    """{call: (the seven fields, the row or None)} for the calls (rows of BK_STAGE_CLUSTERS), from the definition on the genome itself"""
    cl, g = run["cl"], run["genome"]
    rows = [(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"])) for i in calls]
    pairs = sc.as_pairs(rows)
    probes = hc.as_probes([(r[0], r[1], 0, r[2], r[3], 0, 0) for r in rows])
    ref = g.refseq(hc.merged_windows(probes, flank + 2, hc.LENGTHS))
    sim = sc.expected_sim(ref, pairs, flank)
    out = {}
    for k, i in enumerate(calls):
        if rows[k][0] in no_nib or rows[k][2] in no_nib:
            out[i] = (["."] * 7, None)
        else:
            out[i] = (sc.twin_fields(pairs[k], flank, sim[k]), sim[k])
    return out


@pytest.mark.parametrize("variant", ["plain", "everything"])
def test_cli_similar(sim_run, variant):
    run = sim_run
    tmp, cl = run["tmp"], run["cl"]
    flank = 150 if variant == "plain" else 100
    extra = [] if variant == "plain" else ["-vcf", "-consensus", "-homology", "-clip", "-dedup", "-genotype", "-evidence"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-all", "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-o", b, "-similar"] + ([] if variant == "plain" else ["-simflank", "100"]), env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_similar.txt", "_fusion_similar.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt", "_fusion.vcf"}
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    if variant == "everything":
        assert {"_fusion_consensus.txt", "_fusion_homology.txt", "_fusion_rescued.vcf", "_evidence.txt", "_fusion.vcf"} <= set(fa)
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "similar_flank\t%d\n" % flank, (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's seven fields
    seen = {}
    for twin in twins:
        plain = twin.replace("_similar", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(sc.COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) >= (4 if plain == "_fusion.txt" else 11)
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        exp = expected_fields(run, calls, flank)
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            assert line == s + "\t" + "\t".join(exp[i][0]), (line, exp[i][0])
        seen.update(exp)
    # the two planted calls by their designed values, whichever side of the call is its first
    def call_at(locus):
        hit = [(i, v) for i, v in seen.items() if {(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"])), (int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"]))} == {locus[:2], locus[2:]}]
        assert len(hit) == 1, locus
        return hit[0][0], hit[0][1][0]
    i, f = call_at(FWD)
    assert f[:3] == ["71", "80", "3"] and int(f[3]) >= 20 and f[4] == "+" and f[5:] == (["299950", "699970"] if int(cl[i]["p1_tid"]) == 0 else ["699970", "299950"]), f
    i, f = call_at(REV)
    assert f[:5] == ["80", "80", "0", "80", "-"] and f[5:] == (["899980", "399960"] if int(cl[i]["p1_tid"]) == 2 else ["399960", "899980"]), f
    others = [v[0] for j, v in seen.items() if j not in (call_at(FWD)[0], call_at(REV)[0])]
    assert others and all(0 < int(v[0]) < 25 for v in others)  # every other call: what random windows share
    # 3. the VCF: the three keys last in INFO on both breakends of a call, their header lines, nothing else touched
    if variant == "plain":
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 2 * len(written_calls(cl, b + "_fusion_all.txt"))
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i = int(y[2][2:].split("_")[0])
        fields = seen[i][0]
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + ";SIMSCORE=%s;SIMLEN=%s;SIMRUN=%s" % (fields[0], fields[1], fields[3]), lb
    assert sum(";SIMSCORE=80;SIMLEN=80;SIMRUN=80" in l for l in body_b) == 2 and sum(";SIMSCORE=71;SIMLEN=80;" in l for l in body_b) == 2


def test_cli_similar_without_calls_without_a_nib_file_and_errors(sim_run):
    run = sim_run
    tmp, cl = run["tmp"], run["cl"]
    # a contig without a nib file: a call that touches it is not submitted
    c = os.path.join(tmp, "c")
    r = subprocess.run([BIN, "-i", run["bam"], "-n", run["nib_less"], "-o", c, "-all", "-fast", "-similar", "-vcf"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = written_calls(cl, c + "_fusion_all.txt")
    exp = expected_fields(run, calls, 150, no_nib=(1,))
    lines, src = open(c + "_fusion_all_similar.txt").read().split("\n"), open(c + "_fusion_all.txt").read().split("\n")
    by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
    dotted = 0
    for line, s in zip(lines[1:-1], src[1:-1]):
        f = line.split("\t")
        i = by_key[(f[1], f[2])]
        assert line == s + "\t" + "\t".join(exp[i][0]), line
        on_one = 1 in (int(cl[i]["p1_tid"]), int(cl[i]["p2_tid"]))
        assert (f[-7:] == ["."] * 7) == on_one
        dotted += on_one
    assert 3 <= dotted < len(calls)
    body = [l.split("\t") for l in open(c + "_fusion.vcf").read().split("\n") if l and not l.startswith("#")]
    assert len(body) == 2 * len(calls)
    for y in body:
        i = int(y[2][2:].split("_")[0])
        assert (";SIMSCORE=" in y[7]) == (exp[i][1] is not None) and (";SIMLEN=" in y[7]) == (";SIMRUN=" in y[7]) == (exp[i][1] is not None), y
    # a sample without calls, and the option rules
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp2:
        tb = os.path.join(tmp2, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp2)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp2, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-simflank", "100"], "-simflank needs -similar."), (["-similar", "-gpus", "2"], "-similar cannot be combined with -gpus."),
                           (["-similar", "-simflank", "0"], "-simflank must be a number from 1 to 255."),
                           (["-similar", "-simflank", "256"], "-simflank must be a number from 1 to 255.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp2))
        r = subprocess.run(base + ["-similar", "-vcf", "-simflank", "255"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_similar.txt", "_fusion_all_similar.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(sc.COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\nsimilar_flank\t255\n")

"""Fusion frame (`bk_fusion_frame`, `-frame`): the kernel against the definition in tests/framecases.py byte for byte.  Overlap counts
around the 64 candidates of a step and beyond the staging chunk, on a nested locus whose walk passes transcripts that do not overlap;
breakpoints on and beside every edge of transcripts, CDS and coding parts for both strands and directions on both sides; single-part,
non-coding and 363-part transcripts; sides that overlap nothing, an empty model, no sites; a permuted list and a second run; every
refusal; timing; and the command line's files against the definition."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import framecases as fc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
FRAME_CHUNK = abi.FRAME_CHUNK
CONTIGS = [("c0", 5_000_000), ("c1", 5_000_000), ("c2", 1_000_000)]


@pytest.fixture(scope="module")
def ctx():
    """a context that holds no records: bk_fusion_frame needs none"""
    t = capi.Context(CONTIGS)
    yield t
    t.close()


def assert_rows(got, exp):
    assert got.dtype == abi.FRAME_CALL and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def all_directions(t1, P1, t2, P2):
    return [(t1, P1, r1, t2, P2, r2) for r1 in (0, 1) for r2 in (0, 1)]


# ---- 1. overlap counts -----------------------------------------------------------------------------------------------------------------
COUNTS = [(a, b) for a in (0, 1, 63, 64, 65) for b in (0, 1, 63, 64, 65)] + [(FRAME_CHUNK + 72, 65), (1, 2 * FRAME_CHUNK + 1), (FRAME_CHUNK + 1, FRAME_CHUNK + 1)]


@pytest.mark.parametrize("n1,n2", COUNTS)
def test_overlap_counts_on_a_nested_locus(ctx, n1, n2):
    r1, P1 = fc.nested_locus(n1, tid=0, base=1_000_000, seed=1)
    r2, P2 = fc.nested_locus(n2, tid=1, base=2_000_000, seed=2)
    rows = sorted(r1 + r2, key=lambda r: (r[0], r[1]))
    cols = fc.make_cols(rows)
    sites = fc.as_sites(all_directions(0, P1, 1, P2) + all_directions(1, P2, 0, P1) + all_directions(0, P1 + 1, 1, P2 - 1) + all_directions(0, P1, 0, P1)
                        + all_directions(1, P2, 1, P2 + 3))
    exp = fc.expected(cols, sites)
    assert list(exp[0]["n_tx"]) == [n1, n2] and list(exp[4]["n_tx"]) == [n2, n1]
    # the walk backwards from the site passes the 300 short transcripts that end in front of it whenever the long one is there
    assert sum(1 for r in r1 if r[2] < P1) == 300 and (n1 == 0) == (not any(r[1] < P1 <= r[2] for r in r1))
    assert_rows(ctx.fusion_frame(cols, sites), exp)


# ---- 2. positions and transcript shapes ----------------------------------------------------------------------------------------------------
def shapes_model():
    """per contig and strand a three-part transcript with both UTRs, one without UTRs, a single-part one, a non-coding one, all
    overlapping each other; on c1 also a 363-part transcript"""
    rows = []
    for tid in (0, 1):
        for strand in (0, 1):
            o = 10_000 + 37 * strand
            rows += [(tid, o, o + 900, strand, [(o + 100, o + 200), (o + 300, o + 301), (o + 500, o + 777)]), (tid, o + 50, o + 700, strand, [(o + 50, o + 120), (o + 650, o + 700)]),
                     (tid, o + 150, o + 800, strand, [(o + 290, o + 620)]), (tid, o + 10, o + 910, strand, [])]
    many = [(20_000 + 10 * g, 20_000 + 10 * g + 1 + g % 9) for g in range(363)]
    rows.append((1, 19_990, 23_700, 1, many))
    rows.append((1, 19_000, 30_000, 0, [(19_500, 19_600), (29_000, 29_100)]))
    return sorted(rows, key=lambda r: (r[0], r[1]))


def edge_positions(rows, tid):
    pos = set()
    for r in rows:
        if r[0] != tid:
            continue
        for v in [r[1], r[2]] + [x for p in r[4] for x in p]:
            pos.update(P for P in (v, v + 1) if P >= 1)  # b = v - 1 and b = v: either side of the edge
    return sorted(pos)


def test_every_edge_of_transcripts_cds_and_parts(ctx):
    rows = shapes_model()
    cols = fc.make_cols(rows)
    assert max(len(r[4]) for r in rows) == 363 and any(len(r[4]) == 1 for r in rows) and any(not r[4] for r in rows)
    e0, e1 = edge_positions(rows, 0), edge_positions(rows, 1)
    site_rows = []
    for P in e0:  # every edge on side 1, then on side 2, against a fixed partner inside the 363-part transcript and its neighbour
        site_rows += all_directions(0, P, 1, 21_003) + all_directions(1, 21_003, 0, P)
    for P in e1:
        site_rows += [(1, P, r, 0, 10_350, 1 - r) for r in (0, 1)] + [(0, 10_350, r, 1, P, r) for r in (0, 1)]
    for P, Q in zip(e0[::2], e0[1::3]):  # both sides on edges of one locus: pairs of a transcript with itself among them
        site_rows += all_directions(0, P, 0, Q)
    sites = fc.as_sites(site_rows)
    exp = fc.expected(cols, sites)
    assert set(int(c) for c in exp["cls"]) == {0, 1, 2, 3, 4, 5} and set(int(v) for v in exp["loc"].ravel()) == {0, 1, 2, 3, 4, 5}
    assert int(exp["exon"].max()) == 363 and int((exp["tx"][:, 0] == exp["tx"][:, 1]).sum()) > 20
    assert_rows(ctx.fusion_frame(cols, sites), exp)


# ---- 3. degenerate inputs, stability -------------------------------------------------------------------------------------------------------
def test_sides_that_overlap_nothing_an_empty_model_and_no_sites(ctx):
    rows = shapes_model()
    cols = fc.make_cols(rows)
    sites = fc.as_sites([(-1, 10_350, 0, 1, 21_003, 1), (0, 10_350, 0, -1, 21_003, 1), (-1, 5, 1, -1, 5, 0), (2, 10_350, 0, 1, 21_003, 1), (0, 10_350, 1, 2, 500, 0),
                         (7, 10_350, 0, 0, 10_350, 0), (0, 0, 0, 0, 1, 1), (0, 4_999_999, 0, 1, 0xFFFFFFFF, 1), (0, 10_000, 0, 0, 10_001, 1), (0x7FFFFFFF, 10_350, 0, 0, 10_350, 1)])
    exp = fc.expected(cols, sites)
    assert [int(c) for c in exp["cls"]] == [0] * 8 + [0, 0] and list(exp[8]["n_tx"]) == [0, 1]
    assert list(exp[0]["tx"]) == [-1, int(exp[0]["tx"][1])] and int(exp[0]["tx"][1]) >= 0 and int(exp[0]["role"][1]) > 0
    assert_rows(ctx.fusion_frame(cols, sites), exp)
    empty = fc.make_cols([])
    got = ctx.fusion_frame(empty, sites)
    assert_rows(got, fc.expected(empty, sites))
    assert all(list(g["tx"]) == [-1, -1] and not g.tobytes().replace(b"\xff", b"").strip(b"\0") for g in got)
    none = ctx.fusion_frame(cols, np.zeros(0, abi.FRAME_SITE))
    assert len(none) == 0 and none.dtype == abi.FRAME_CALL
    assert len(ctx.fusion_frame(empty, np.zeros(0, abi.FRAME_SITE))) == 0


def test_a_permuted_list_and_a_second_run(ctx):
    r1, P1 = fc.nested_locus(70, tid=0, base=1_000_000, seed=5)
    rows = sorted(r1 + shapes_model(), key=lambda r: (r[0], r[1]))
    cols = fc.make_cols(rows)
    rng = np.random.default_rng(11)
    site_rows = []
    for _ in range(300):
        site_rows.append((int(rng.integers(-1, 3)), int(rng.choice([P1, P1 - 7, 10_000 + int(rng.integers(0, 1000)), 20_000 + int(rng.integers(0, 3700))])), int(rng.integers(0, 2)),
                          int(rng.integers(0, 2)), int(rng.choice([P1, 10_000 + int(rng.integers(0, 1000)), 20_000 + int(rng.integers(0, 3700))])), int(rng.integers(0, 2))))
    sites = fc.as_sites(site_rows)
    first = ctx.fusion_frame(cols, sites)
    assert_rows(first, fc.expected(cols, sites))
    assert ctx.fusion_frame(cols, sites).tobytes() == first.tobytes()
    perm = rng.permutation(len(sites))
    assert ctx.fusion_frame(cols, sites[perm]).tobytes() == first[perm].tobytes()
    model = capi.TxModel([(r[0], r[1], r[2], "+-"[r[3]], r[4], "T%d" % k, "G%d" % k) for k, r in enumerate(rows)])  # the helper gives the same columns
    assert all(np.array_equal(model.cols[k], cols[k]) for k, _ in abi.TXMODEL_COLS)
    assert ctx.fusion_frame(model, sites).tobytes() == first.tobytes()


# ---- 4. refusals, timing ---------------------------------------------------------------------------------------------------------------------
def raw_call(t, cols, sites, n=None, null=(), n_tx=None, n_parts=None):
    C = capi.C
    sites = np.ascontiguousarray(sites, abi.FRAME_SITE)
    m, keep = capi.txmodel_struct(cols)
    if n_tx is not None:
        m.n_tx = n_tx
    if n_parts is not None:
        m.n_parts = n_parts
    out = C.c_void_p()
    rc = t.L.bk_fusion_frame(None if "ctx" in null else t.h, None if "model" in null else C.byref(m), None if "sites" in null else sites.ctypes.data,
                             len(sites) if n is None else n, None if "out" in null else C.byref(out))
    del keep
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


GOOD = [(0, 100, 900, 0, [(150, 200), (300, 400)]), (0, 100, 500, 1, []), (1, 50, 800, 1, [(50, 60), (60, 800)])]


def test_argument_refusals(ctx):
    sites = fc.as_sites([(0, 350, 0, 1, 60, 1), (1, 700, 1, 0, 101, 0)])
    good = fc.make_cols(GOOD)
    assert raw_call(ctx, good, sites)[0] == abi.BK_OK
    for null in ("ctx", "model", "sites", "out"):
        assert raw_call(ctx, good, sites, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(ctx, good, sites, n=0, null=("sites",))[0] == abi.BK_OK
    for field in ("right1", "right2"):
        bad = sites.copy()
        bad[1][field] = 2
        rc, msg = raw_call(ctx, good, bad)
        assert rc == abi.BK_ERR_ARG and "site 1" in msg and "right" in msg, msg
    rc, msg = raw_call(ctx, good, sites, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg, msg
    # the model's limits are looked at before any array: the columns here are three rows long
    rc, msg = raw_call(ctx, good, sites, n_tx=(1 << 24) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^24 transcripts" in msg, msg
    rc, msg = raw_call(ctx, good, sites, n_parts=(1 << 28) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^28" in msg, msg

    def broken(change, word):
        rows = [list(r[:4]) + [list(r[4])] for r in GOOD]
        cols = fc.make_cols(change(rows) or rows)
        rc, msg = raw_call(ctx, cols, sites)
        assert rc == abi.BK_ERR_ARG and word in msg, (word, msg)

    broken(lambda r: r.reverse(), "out of order")                                    # tid descends
    broken(lambda r: r[1].__setitem__(1, 99), "out of order")                        # tx_start descends on one tid
    broken(lambda r: r[0].__setitem__(3, 2), "strand above 1")
    broken(lambda r: r[0].__setitem__(0, -1), "negative tid")
    broken(lambda r: r[1].__setitem__(2, 99), "ends in front of its start")
    broken(lambda r: r[0].__setitem__(4, [(300, 400), (150, 200)]), "descend or overlap")
    broken(lambda r: r[0].__setitem__(4, [(150, 301), (300, 400)]), "descend or overlap")
    broken(lambda r: r[0].__setitem__(4, [(150, 150)]), "empty or descending")
    broken(lambda r: r[0].__setitem__(4, [(200, 150)]), "empty or descending")
    broken(lambda r: r[0].__setitem__(4, [(99, 200)]), "outside [tx_start, tx_end)")
    broken(lambda r: r[2].__setitem__(4, [(50, 60), (60, 801)]), "outside [tx_start, tx_end)")
    for off, word in (([0, 2, 1, 4], "ex_off does not ascend"), ([1, 2, 2, 4], "ex_off does not run"), ([0, 2, 2, 3], "ex_off does not run"), ([0, 2, 5, 4], "ex_off does not ascend")):
        cols = dict(good, ex_off=np.asarray(off, np.uint32))
        rc, msg = raw_call(ctx, cols, sites)
        assert rc == abi.BK_ERR_ARG and word in msg, (off, msg)
    for name, _ in abi.TXMODEL_COLS:
        cols = dict(good)
        cols[name] = np.zeros(0, cols[name].dtype)
        m, keep = capi.txmodel_struct(cols)
        m.n_tx, m.n_parts = 3, 4
        out = capi.C.c_void_p()
        rc = ctx.L.bk_fusion_frame(ctx.h, capi.C.byref(m), sites.ctypes.data, len(sites), capi.C.byref(out))
        assert rc == abi.BK_ERR_ARG and "lacks a column" in (ctx.L.bk_last_error(ctx.h) or b"").decode(), name
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.fusion_frame(good, sites)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.fusion_frame(good, sites), fc.expected(good, sites))  # the context still works


def test_frame_is_timed_and_changes_no_stage():
    ds = synth.make_g1()
    cols = ds.to_soa()
    model, _ = capi.TxModel.from_refgene(synth.G1_REFGENE, [n for n, _ in ds.contigs])
    sites = fc.as_sites([(0, 50099, 0, 1, 80200, 1)])
    t = capi.Context(ds.contigs)
    t.timing_enable(True)
    got = t.fusion_frame(model, sites)  # before any record is there
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    bytes_model = 21 * 2 + 16 * 5 + 72 * 1
    assert names[-1] == "fusion_frame" and tm["fusion_frame"][0] > 0 and tm["fusion_frame"][1] == bytes_model == touched["fusion_frame"]
    t.timing_enable(False)
    assert int(got[0]["cls"]) == fc.ANTISENSE and list(got[0]["cod"]) == [599, 9301]
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=True)  # the stages behind it give the G1 call, as on a context that never made the call
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    assert n_valid == 1 and (int(cl[0]["p1_exact"]), int(cl[0]["p2_exact"])) == (50099, 80200)
    assert t.fusion_frame(model, sites).tobytes() == got.tobytes()
    t.close()


# ---- 5. command line -------------------------------------------------------------------------------------------------------------------------
# three calls: a '+' head on chr1 joined to a '+' tail on chr2 (in frame with one isoform of the tail, out of frame with the other), a
# '+' head on chr1 joined to a '-' tail on chr3 (out of frame with both isoforms), and two '+' tails (antisense)
FRAME_LOCI = [("IN", 0, 300_000, "L", 1, 700_000, "R"), ("OUT", 0, 600_000, "L", 2, 500_000, "L"), ("ANTI", 1, 300_000, "R", 3, 900_000, "R")]
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=String," % k for k in ("FRCLASS", "FR5P", "FR3P"))


def gene_line(acc, chrom, strand, tx, cds, exons, gene):
    return "0\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t0\t%s\tcmpl\tcmpl\t%s" % (acc, chrom, strand, tx[0], tx[1], cds[0], cds[1], len(exons), "".join("%d," % s for s, _ in exons),
                                                                              "".join("%d," % e for _, e in exons), gene, "0," * len(exons))


def frame_refgene():
    head = lambda bp: [(bp - 10_000, bp - 9_000), (bp - 1_000, bp), (bp + 5_000, bp + 10_000)]                 # the second exon ends at the breakpoint
    tail = lambda bp: [(bp - 10_000, bp - 9_000), (bp - 1, bp + 1_000), (bp + 5_000, bp + 10_000)]             # the second exon starts at the breakpoint base
    rows = []
    for bp, gene in ((300_000, "HEADA"), (600_000, "HEADC")):                                                  # h = 900 + 1000 = 1900, remainder 1
        rows.append(gene_line("NM_%s1" % gene, "chr1", "+", (bp - 10_000, bp + 10_000), (bp - 9_900, bp + 9_900), head(bp), gene))
        rows.append(gene_line("NM_%s2" % gene, "chr1", "+", (bp - 10_000, bp + 10_000), (bp + 6_000, bp + 9_900), head(bp), gene))  # its CDS lies behind the breakpoint: h = 0
    rows.append(gene_line("NR_HEADA3", "chr1", "+", (290_000, 310_000), (310_000, 310_000), head(300_000), "HEADA"))
    rows.append(gene_line("NM_TAILB1", "chr2", "+", (690_000, 710_000), (690_099, 709_900), tail(700_000), "TAILB"))    # t = 901, remainder 1: in frame
    rows.append(gene_line("NM_TAILB2", "chr2", "+", (690_000, 710_000), (690_100, 709_900), tail(700_000), "TAILB"))    # t = 900: out of frame
    rows.append(gene_line("NM_TAILB3", "chr2", "+", (695_000, 699_999), (695_100, 699_900), [(695_000, 699_999)], "TAILB"))  # ends one base in front of the breakpoint base
    dm = [(490_000, 491_000), (499_000, 500_001), (505_000, 510_000)]                                          # '-': what lies right of the breakpoint is lost
    rows.append(gene_line("NM_TAILD1", "chr3", "-", (490_000, 510_000), (490_100, 509_900), dm, "TAILD"))              # t = 4900 + 1 = 4901, remainder 2
    rows.append(gene_line("NM_TAILD2", "chr3", "-", (490_000, 510_000), (490_100, 509_898), dm, "TAILD"))              # t = 4899, remainder 0
    rows.append(gene_line("NM_TAILE1", "chr2", "+", (290_000, 310_000), (290_100, 309_900), tail(300_000), "TAILE"))
    rows.append(gene_line("NM_TAILF1", "chr4", "+", (890_000, 910_000), (890_100, 909_900), tail(900_000), "TAILF"))
    rows.append(gene_line("NM_TAILF2", "chr4", "+", (899_000, 901_000), (899_000, 899_000), [(899_000, 901_000)], "TAILF"))  # cdsStart == cdsEnd: non-coding
    rows.append(gene_line("NM_ELSE1", "chrUn_gl000220", "+", (100, 5_000), (200, 4_000), [(100, 5_000)], "ELSE"))      # a contig the input lacks
    return rows


@pytest.fixture(scope="module")
def frame_run():
    with tempfile.TemporaryDirectory() as tmp:
        ds = cc.designed_tumor(mix=False, loci=FRAME_LOCI, n_proper=3000)
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        lines = frame_refgene()
        side = synth.write_side_files(ds, tmp, refgene_lines=lines)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        t = capi.Context(ds.contigs)
        t.upload(ds.to_soa())
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        sides = [capi.junction_sides(j)[:2] for j in t.junctions()]
        model, dropped = capi.TxModel.from_refgene(lines, cc.NAMES)
        assert dropped == 1 and len(model) == len(lines) - 2
        sites = fc.as_sites([(int(c["p1_tid"]), int(c["p1_exact"]), sides[i][0], int(c["p2_tid"]), int(c["p2_exact"]), sides[i][1]) for i, c in enumerate(cl)])
        exp = fc.expected(model.cols, sites)
        assert_rows(t.fusion_frame(model, sites), exp)
        t.close()
        yield {"tmp": tmp, "bam": bam, "nib": side["nib"], "env": env, "cl": cl, "exp": exp, "model": model}


@pytest.mark.parametrize("variant", ["plain", "all_vcf"])
def test_cli_frame(frame_run, variant):
    run = frame_run
    tmp, cl, exp, model = run["tmp"], run["cl"], run["exp"], run["model"]
    extra = ["-all", "-vcf"] if variant == "all_vcf" else []
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-frame"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    keep = lambda text: [l for l in text.split("\n") if "costs time" not in l]
    said = "frame model: %d transcripts, 1 on contigs the input lacks" % len(model)
    assert [l for l in keep(r.stdout) if l != said] == keep(out_a.replace(a, b)) and r.stdout.count(said + "\n") == 1
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_frame.txt", "_fusion_frame.txt"] if variant == "all_vcf" else ["_fusion_frame.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    for suffix in fa:
        if suffix not in {"_params.txt", "_performance.txt", "_fusion.vcf"}:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "frame\n", (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's columns
    classes = {}
    for twin in twins:
        plain = twin.replace("_frame", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(fc.FRAME_COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            assert line == s + "\t" + "\t".join(fc.call_fields(exp[i], model.names, model.genes)), line
            classes[i] = f[len(s.split("\t"))]
        if plain == "_fusion_all.txt" or variant == "plain":
            assert sorted(classes.values()) == ["antisense", "inframe", "outframe"], classes
    by_class = {v: exp[i] for i, v in classes.items()}
    def pair(c):  # (transcripts, cod) of the reported pair, the 5' partner first
        x = [(model.names[c["tx"][k]], int(c["cod"][k])) for k in range(2)]
        return x if int(c["order"]) == 1 else x[::-1]

    c = by_class["inframe"]
    assert pair(c) == [("NM_HEADA1", 1900), ("NM_TAILB1", 901)] and list(c["n_tx"]) == [2, 2] and (int(c["n_inframe"]), int(c["n_compatible"])) == (1, 4)
    c = by_class["outframe"]
    assert pair(c) == [("NM_HEADC1", 1900), ("NM_TAILD1", 4901)] and int(c["n_inframe"]) == 0 and int(c["n_compatible"]) == 4
    c = by_class["antisense"]
    assert list(c["role"]) == [fc.TAIL, fc.TAIL] and int(c["n_compatible"]) == 0 and int(c["n_tx"][0]) * int(c["n_tx"][1]) == 2
    # 3. the VCF: FRCLASS / FR5P / FR3P last in INFO of both breakends, their header lines, nothing else touched
    if variant == "plain":
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 6
    tails = set()
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i = int(y[2][2:].split("_")[0])
        tail = fc.info_fields(exp[i], model.genes)
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail, lb
        tails.add(tail)
    assert tails == {";FRCLASS=inframe;FR5P=HEADA;FR3P=TAILB", ";FRCLASS=outframe;FR5P=HEADC;FR3P=TAILD", ";FRCLASS=antisense"}


def test_cli_frame_refusals_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp, refgene_lines=frame_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-frame", "-gpus", "2"], "-frame cannot be combined with -gpus."), (["-frame", "-covflank", "5"], "-covflank needs -coverage."),
                           (["-frame", "-gpus", "2", "-simflank", "3"], "-simflank needs -similar.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-frame", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_frame.txt", "_fusion_all_frame.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(fc.FRAME_COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\nframe\n")
        assert "frame model: " in r.stdout

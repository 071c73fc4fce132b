"""Junction fit (`bk_junction_fit`, `-homology`): the kernel against the Python definition (tests/homologycases.py) bit for bit at
every word boundary of the query and every corner of the three maxima; reference edges; the tie rules on repeats; homology running
into its caps; two runs and a permuted probe list; the bases of bk_clip_consensus fed straight in; errors, limits and empty inputs;
timing; and the command line's files against the definition."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc
from tests import clipcases
from tests import consensuscases as kc
from tests import homologycases as hc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    t = capi.Context(cc.CONTIGS)  # any live context: no table, no stage
    yield t
    t.close()


def random_case(qlen):
    """(ref, probes, query) at max_len = qlen: 260 seeded probes inside the contigs and 40 within 70 bases of their ends, computed once"""
    if qlen not in _CACHE:
        g = hc.genome()
        rng = np.random.default_rng(1000 + qlen)
        p1, q1 = hc.random_table(g, rng, 260, qlen, qlen)
        p2, q2 = hc.random_table(g, rng, 40, qlen, qlen, near_edges=True)
        probes, query = np.concatenate([p1, p2]), np.concatenate([q1, q2])
        _CACHE[qlen] = (g.refseq(hc.merged_windows(probes, qlen + 64 + 64 + 1, hc.LENGTHS)), probes, query)
    return _CACHE[qlen]


def assert_rows(got, exp):
    assert got.dtype == abi.JUNCTION_FIT and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


# ---- 1. the kernel against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_hom", [0, 3, 64])
@pytest.mark.parametrize("max_shift,max_ins", [(0, 0), (1, 1), (32, 32), (64, 64), (64, 0), (0, 64)])
@pytest.mark.parametrize("qlen", [1, 31, 32, 33, 63, 64, 65, 255, 256])
def test_fit_equals_its_definition(ctx, qlen, max_shift, max_ins, max_hom):
    ref, probes, query = random_case(qlen)
    got = ctx.junction_fit(ref, probes, query, max_shift, max_ins, max_hom)
    exp = hc.expected_fit(ref, probes, query, qlen, max_shift, max_ins, max_hom)
    assert_rows(got, exp)
    assert (got["placed"] == 1).all() and len({(int(p["dir_own"]), int(p["dir_mate"])) for p in probes}) == 4
    if qlen >= 31 and max_shift == 64 and max_ins == 64:  # the search finds what the queries were cut with
        assert (got["ins"] > 0).sum() > 20 and (got["shift"] != 0).sum() > 100 and (got["mism"] * 4 < got["aligned"]).sum() > 200


def test_reference_edges(ctx):
    ref, probes, query = hc.edge_table()
    got = ctx.junction_fit(ref, probes, query)
    assert_rows(got, hc.expected_fit(ref, probes, query, 100))
    assert list(got["placed"][-5:]) == [0, 0, 0, 1, 1] and not got[-5:-2].tobytes().strip(b"\0")
    assert (got["mism"] > 0).sum() > 10 and (got["mism"] == 0).sum() > 10
    on_two = probes["tid_own"] == 2  # a contig without a segment: the own walk is N, so no homology
    assert on_two.sum() > 10 and not got["hom_fwd"][on_two].any() and not got["hom_back"][on_two].any()
    # no segment at all: every walk is N, every column a mismatch, and the first placement of the tie order is chosen
    none = hc.make_refseq([])
    got = ctx.junction_fit(none, probes, query)
    assert_rows(got, hc.expected_fit(none, probes, query, 100))
    live = got["placed"] == 1
    assert (got["shift"][live] == 0).all() and (got["ins"][live] == np.minimum(32, probes["qlen"][live] - 1)).all()
    assert_rows(ctx.junction_fit(ref, probes, query, 64, 64, 64), hc.expected_fit(ref, probes, query, 100, 64, 64, 64))


# ---- 2. tie rules, caps, same bytes --------------------------------------------------------------------------------------------------
def test_tie_rules_on_repeats(ctx):
    rows, texts = [], []
    poly, _ = hc.repeat_ref("A")
    di, text = hc.repeat_ref("AC")
    for d_own in (0, 1):
        for d_mate in (0, 1):
            for qlen in (1, 30, 64, 65, 130):
                rows.append((0, 300, d_own, 0, 330, d_mate, qlen))
    probes = hc.as_probes(rows)
    for ref, units in ((poly, ("A", "T")), (di, ("AC", "CA", "GT", "TG", "AG"))):
        for unit in units:
            query = hc.as_query([(unit * 130)[:r[6]] for r in rows], 130)
            for maxima in ((32, 32, 32), (64, 64, 64), (5, 0, 64), (0, 7, 1)):
                got = ctx.junction_fit(ref, probes, query, *maxima)
                assert_rows(got, hc.expected_fit(ref, probes, query, 130, *maxima))
    # poly-A against poly-A: every placement without mismatch ties: the smallest ins, the smallest |shift|
    q = hc.as_query(["A" * r[6] for r in rows], 130)
    got = ctx.junction_fit(poly, probes, q)
    same = probes["dir_own"] != probes["dir_mate"]  # (equal directions read the complement: poly-T)
    assert (got["ins"][same] == 0).all() and (got["shift"][same] == 0).all() and (got["mism"][same] == 0).all()
    # the dinucleotide: the query starts on M[3]; shifts 3, 1, -1, -3, .. fit alike, |1| ties and the non-negative one wins
    r = ctx.junction_fit(di, hc.as_probes([(0, 300, 0, 0, 400, 1, 30)]), hc.as_query([text[402:432]], 64))[0]
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"])) == (0, 1, 0)


def test_homology_runs_into_its_caps(ctx):
    poly, _ = hc.repeat_ref("A")
    for qlen in (1, 63, 64, 65, 128, 200, 256):
        for max_hom in (0, 1, 31, 63, 64):
            p = hc.as_probes([(0, 300, 0, 0, 100, 1, qlen), (0, 300, 1, 0, 400, 0, qlen), (0, 10, 0, 0, 100, 1, qlen), (0, 500, 0, 0, 100, 1, qlen)])
            q = hc.as_query(["A" * qlen] * 4, 256)
            got = ctx.junction_fit(poly, p, q, 32, 32, max_hom)
            assert_rows(got, hc.expected_fit(poly, p, q, 256, 32, 32, max_hom))
            assert not got["shift"].any() and not got["ins"].any()
            for k in (0, 1):  # both caps, on either pair of directions
                assert int(got[k]["hom_fwd"]) == qlen and int(got[k]["hom_back"]) == max_hom
            # ... and the segment's ends: ten retained bases at 1 .. 10, a hundred bases behind 500
            assert int(got[2]["hom_back"]) == min(max_hom, 10) and int(got[3]["hom_fwd"]) == min(qlen, 100)


def test_two_runs_and_a_permuted_probe_list_give_the_same_bytes(ctx):
    ref, probes, query = random_case(65)
    first = ctx.junction_fit(ref, probes, query, 64, 64, 64)
    again = ctx.junction_fit(ref, probes, query, 64, 64, 64)
    perm = np.random.default_rng(9).permutation(len(probes))
    moved = ctx.junction_fit(ref, probes[perm], query[perm], 64, 64, 64)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()


def test_consensus_bases_feed_the_fit(ctx):
    """bases of clip_consensus on the designed table, as they lie, reproduce the designed truth"""
    d = kc.designed()
    sites = d["sites"]
    rows, bases, _ = ctx.clip_consensus(kc.designed_reads(), sites, QUAL, kc.MIN_CLIP, kc.MAX_LEN, kc.MIN_DEPTH)
    probes, texts = hc.designed_table()
    by = {(int(s["tid"]), int(s["pos"]), int(s["dir"])): k for k, s in enumerate(sites)}
    at = [by[(int(p["tid_own"]), int(p["pos_own"]), int(p["dir_own"]))] for p in probes]
    probes["qlen"] = rows["len"][at]
    g = hc.genome()
    ref = g.refseq(hc.merged_windows(probes, 64 + 32 + 33, hc.LENGTHS))
    got = ctx.junction_fit(ref, probes, bases[at])
    assert_rows(got, hc.expected_fit(ref, probes, hc.as_query(texts, 64), 64))
    assert (got["shift"] == 0).all() and (got["ins"] == 0).all() and int(got["mism"].sum()) == 1 and list(got["aligned"]) == [40, 60] * 9


# ---- 3. errors, limits, empty inputs, timing ------------------------------------------------------------------------------------------
def raw_call(t, ref, probes, query, max_len, n=None, n_segs=None, maxima=(32, 32, 32), null=()):
    C = capi.C
    s, keep = capi.refseq_struct(ref)
    if n_segs is not None:
        s.n_segs = n_segs
    probes = np.ascontiguousarray(probes, abi.JUNCTION_PROBE)
    query = np.ascontiguousarray(query, np.uint8)
    out = C.c_void_p()
    rc = t.L.bk_junction_fit(None if "ctx" in null else t.h, None if "ref" in null else C.byref(s), None if "probes" in null else probes.ctypes.data,
                             len(probes) if n is None else n, None if "query" in null else query.ctypes.data, max_len, *maxima, None if "out" in null else C.byref(out))
    del keep
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_and_limit_errors(ctx):
    ref, probes, query = hc.edge_table()
    assert raw_call(ctx, ref, probes, query, 100)[0] == abi.BK_OK
    for null in ("ctx", "ref", "probes", "query", "out"):
        assert raw_call(ctx, ref, probes, query, 100, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(ctx, ref, probes, query, 100, n=0, null=("probes", "query"))[0] == abi.BK_OK
    for max_len in (0, 257):
        rc, msg = raw_call(ctx, ref, probes, query, max_len)
        assert rc == abi.BK_ERR_ARG and "max_len" in msg, msg
    for i, word in enumerate(("max_shift", "max_ins", "max_hom")):
        m = [32, 32, 32]
        m[i] = 65
        rc, msg = raw_call(ctx, ref, probes, query, 100, maxima=tuple(m))
        assert rc == abi.BK_ERR_ARG and word in msg, msg
    for field, value, word in (("dir_own", 2, "dir above 1"), ("dir_mate", 2, "dir above 1"), ("qlen", 101, "qlen above max_len")):
        bad = probes.copy()
        bad[1][field] = value
        rc, msg = raw_call(ctx, ref, bad, query, 100)
        assert rc == abi.BK_ERR_ARG and word in msg and "probe 1" in msg, msg
    for byte in (0, ord("a"), ord("R")):
        bad = query.copy()
        bad[2, int(probes[2]["qlen"]) - 1] = byte
        rc, msg = raw_call(ctx, ref, probes, bad, 100)
        assert rc == abi.BK_ERR_ARG and "probe 2" in msg and "outside ACGTN" in msg, msg
    ok = query.copy()
    ok[2, int(probes[2]["qlen"]):] = 0  # behind qlen anything goes: that is how bk_clip_consensus leaves its rows
    assert raw_call(ctx, ref, probes, ok, 100)[0] == abi.BK_OK

    def with_col(name, index, value):
        r = dict(ref)
        r[name] = ref[name].copy()
        r[name][index] = value
        return r
    for bad, word in ((with_col("start", 1, 300), "overlaps"), (with_col("start", 2, 0), "out of order"), (with_col("tid", 0, 2), "out of order"),
                      (with_col("off", 3, int(ref["off"][2]) - 1), "off does not ascend"), (with_col("len", 3, 2 * int(ref["off"][4] - ref["off"][3]) + 1), "fewer bytes")):
        rc, msg = raw_call(ctx, bad, probes, query, 100)
        assert rc == abi.BK_ERR_ARG and word in msg, msg
    # the limits are looked at before any array: the small ones are never read beyond their end
    rc, msg = raw_call(ctx, ref, probes, query, 100, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 probes" in msg, msg
    rc, msg = raw_call(ctx, ref, probes, query, 100, n_segs=(1 << 20) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^20 segments" in msg, msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.junction_fit(ref, probes, query)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.junction_fit(ref, probes, query), hc.expected_fit(ref, probes, query, 100))  # the context still works
    none = ctx.junction_fit(ref, np.zeros(0, abi.JUNCTION_PROBE), np.zeros((0, 64), np.uint8))
    assert len(none) == 0 and none.dtype == abi.JUNCTION_FIT


def test_fit_is_timed():
    ref, probes, query = random_case(64)
    t = capi.Context(cc.CONTIGS)
    t.timing_enable(True)
    rows = t.junction_fit(ref, probes, query)
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "junction_fit" in tm and tm["junction_fit"][0] > 0 and tm["junction_fit"][1] > 0
    # the byte model: the probe row, qlen query bytes, the nibbles of both walks, the result row
    n, qsum = len(probes), int(probes["qlen"].sum())
    assert touched["junction_fit"] == n * 64 + qsum + (2 * qsum + n * 4 * 32 + 1) // 2
    t.close()


# ---- 4. command line ----------------------------------------------------------------------------------------------------------------
HOM_COLUMNS = [c + s for s in "12" for c in ("J_Shift", "J_Ins", "J_Aligned", "J_Mism", "J_HomLen", "J_HomSeq", "J_InsSeq")]
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=%s," % kv for kv in (("HOMLEN", "Integer"), ("HOMSEQ", "String"), ("JINS", "String"), ("JAL", "Integer"), ("JMM", "Integer"),
                                                                     ("JSH", "Integer")))


@pytest.fixture(scope="module")
def plus_run():
    """the designed BAM with the insertion and the microhomology locus, its side files, and nib files written from the same genome:
    one directory with every contig, one without chr2"""
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "t.bam")
        hc.write_plus_bam(bam)
        bamio.write_bai(bam)
        ds = hc.designed_plus()["ds"]
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        g = hc.genome()
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
        js = t.junctions()
        t.close()
        whole = g.refseq([(tid, 0, n) for tid, n in enumerate(hc.LENGTHS)])
        yield {"tmp": tmp, "bam": bam, "nib": side["nib"], "nib_less": less, "env": env, "cl": cl, "js": js, "genome": g, "ref": whole, "reads": hc.plus_reads()}


def expected_sides(run, calls, conslen, max_shift, max_ins, no_nib=()):
    """{(call, side): (the seven fields, the fit row or None, the consensus text)} for the calls (rows of BK_STAGE_CLUSTERS)"""
    cl, js, g = run["cl"], run["js"], run["genome"]
    sites = []
    for i in calls:
        d1, d2 = clipcases.junction_sides(js[i])
        sites += [(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), 0, d1), (int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"]), 0, d2)]
    rows, bases, _ = kc.expected_consensus(run["reads"], kc.as_sites(sites), QUAL, kc.MIN_CLIP, conslen, kc.MIN_DEPTH)
    probes, texts, where = [], [], []
    for x, s in enumerate(sites):
        m = sites[x ^ 1]
        if int(rows[x]["len"]) > 0 and s[0] not in no_nib and m[0] not in no_nib:
            probes.append((s[0], s[1], s[3], m[0], m[1], m[3], int(rows[x]["len"])))
            texts.append(bytes(bases[x, :int(rows[x]["len"])]).decode())
            where.append(x)
    probes = hc.as_probes(probes)
    fit = hc.expected_fit(run["ref"], probes, hc.as_query(texts, conslen), conslen, max_shift, max_ins, 32)
    out = {(i, s): (["."] * 7, None, "") for i in calls for s in (0, 1)}
    for k, x in enumerate(where):
        out[(calls[x // 2], x & 1)] = (hc.side_fields(g, probes[k], texts[k], fit[k]), fit[k], texts[k])
    return out


@pytest.mark.parametrize("variant", ["plain", "everything"])
def test_cli_homology(plus_run, variant):
    run = plus_run
    tmp, cl = run["tmp"], run["cl"]
    conslen, max_shift, max_ins = (64, 32, 32) if variant == "plain" else (50, 40, 10)
    extra = [] if variant == "plain" else ["-evidence", "-dedup", "-clip", "-genotype", "-conslen", "50"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-all", "-fast", "-consensus", "-vcf"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-o", b, "-homology"] + ([] if variant == "plain" else ["-homshift", "40", "-homins", "10"]), env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical (the _consensus twins too)
    twins = ["_fusion_all_homology.txt", "_fusion_homology.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt", "_fusion.vcf"}
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    assert {"_fusion_consensus.txt", "_fusion_all_consensus.txt"} <= set(fa) - changed
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "homology_max_shift\t%d\nhomology_max_ins\t%d\n" % (max_shift, max_ins), (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's seven fields per side
    seen = {}
    for twin in twins:
        plain = twin.replace("_homology", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(HOM_COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) >= (4 if plain == "_fusion.txt" else 11)
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        exp = expected_sides(run, calls, conslen, max_shift, max_ins)
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            assert line == s + "\t" + "\t".join(exp[(i, 0)][0] + exp[(i, 1)][0]), (line, exp[(i, 0)][0], exp[(i, 1)][0])
        seen.update(exp)
    # the designed loci by their texts: the insertion as the BAM reads it, the homology on either contig
    def side_at(t, bp):
        hit = [v for (i, s), v in seen.items() if (int(cl[i]["p%d_tid" % (s + 1)]), int(cl[i]["p%d_exact" % (s + 1)])) == (t, bp)]
        assert len(hit) == 1, (t, bp)
        return hit[0][0]
    f = side_at(*hc.INS_LOCUS[1:3])
    assert f[:4] == [str(hc.INS_SHIFT), "7", "33", "0"] and f[6] == hc.ins_locus_inserted()
    fa_, fb_ = side_at(*hc.HOM_LOCUS[1:3]), side_at(*hc.HOM_LOCUS[4:6])
    assert fa_[:5] == ["0", "0", "40", "0", "6"] and fb_[4] == "6" and fa_[5] == fb_[5] and len(fa_[5]) == 6 and fa_[6] == "."
    assert fa_[5][-hc.HOM_PATCHED:] == run["genome"].text(hc.HOM_LOCUS[1], hc.HOM_LOCUS[2] + 1, hc.HOM_LOCUS[2] + hc.HOM_PATCHED)
    assert sum(v[1] is not None for v in seen.values()) >= 22
    # 3. the VCF: the six keys last in INFO on each breakend for its own side, their header lines, nothing else touched
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 6 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 2 * len(written_calls(cl, b + "_fusion_all.txt"))
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        fields, fit, _ = seen[(i, s)]
        tail = ""
        if fit is not None:
            if fields[4] != "0":
                tail += ";HOMLEN=%s;HOMSEQ=%s" % (fields[4], fields[5])
            if fields[6] != ".":
                tail += ";JINS=" + fields[6]
            tail += ";JAL=%s;JMM=%s;JSH=%s" % (fields[2], fields[3], fields[0])
        assert ";CSN=" in x[7] and y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail, lb
    assert any(";HOMLEN=6;" in l for l in body_b) and any(";JINS=" in l for l in body_b)


def test_cli_homology_without_calls_without_a_nib_file_and_errors(plus_run):
    run = plus_run
    tmp, cl = run["tmp"], run["cl"]
    # a contig without a nib file: a side on it, or whose mate is on it, is not submitted
    c = os.path.join(tmp, "c")
    r = subprocess.run([BIN, "-i", run["bam"], "-n", run["nib_less"], "-o", c, "-all", "-fast", "-consensus", "-homology"], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = written_calls(cl, c + "_fusion_all.txt")
    exp = expected_sides(run, calls, 64, 32, 32, no_nib=(1,))
    lines, src = open(c + "_fusion_all_homology.txt").read().split("\n"), open(c + "_fusion_all.txt").read().split("\n")
    by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
    dotted = 0
    for line, s in zip(lines[1:-1], src[1:-1]):
        f = line.split("\t")
        i = by_key[(f[1], f[2])]
        assert line == s + "\t" + "\t".join(exp[(i, 0)][0] + exp[(i, 1)][0]), line
        on_one = 1 in (int(cl[i]["p1_tid"]), int(cl[i]["p2_tid"]))
        assert (f[-14:] == ["."] * 14) == on_one
        dotted += on_one
    assert 3 <= dotted < len(calls)
    # a sample without calls, and the option rules
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp2:
        tb = os.path.join(tmp2, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp2)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp2, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-homology"], "-homology needs -consensus"), (["-consensus", "-homshift", "3"], "-homshift and -homins need -homology"),
                           (["-consensus", "-homology", "-gpus", "2"], "-homology cannot be combined with -gpus"),
                           (["-consensus", "-homology", "-homshift", "65"], "-homshift and -homins must be numbers from 0 to 64"),
                           (["-consensus", "-homology", "-homins", "-1"], "-homshift and -homins must be numbers from 0 to 64")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and word in r.stderr, (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp2))
        r = subprocess.run(base + ["-consensus", "-homology", "-vcf", "-homshift", "0", "-homins", "64"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_homology.txt", "_fusion_all_homology.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(HOM_COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("consensus_max_len\t64\nhomology_max_shift\t0\nhomology_max_ins\t64\n")

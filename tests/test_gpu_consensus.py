"""Junction consensus (`bk_clip_consensus`, `-consensus`): the kernels against the Python definition (tests/consensuscases.py) byte for
byte on the designed table and on the numpy-only ones, at every column-round boundary; two runs and a permuted table; the identity
with bk_clip_reads; errors, limits and empty inputs; and the command line's files against the definition and the designed truth."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import clipcases
from tests import consensuscases as kc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
_CACHE = {}


def tables():
    """(reads, sites) of the designed table and of the crowd table, and the definition's results, computed once"""
    if not _CACHE:
        _CACHE["designed"] = (kc.designed_reads(), kc.designed()["sites"])
        _CACHE["crowd"] = kc.crowd_table()
        _CACHE["expected"] = {}
    return _CACHE


def expected(name, max_len, min_depth):
    t = tables()
    key = (name, max_len, min_depth)
    if key not in t["expected"]:
        t["expected"][key] = kc.expected_consensus(*t[name], QUAL, kc.MIN_CLIP, max_len, min_depth)
    return t["expected"][key]


@pytest.fixture(scope="module")
def ctx():
    t = capi.Context(cc.CONTIGS)  # any live context: no table, no stage
    yield t
    t.close()


def assert_equal(got, exp):
    (gr, gb, gd), (er, eb, ed) = got, exp
    assert gr.dtype == abi.CONSENSUS and gb.dtype == np.uint8 and gd.dtype == np.uint32
    bad = [k for k in range(len(er)) if gr[k].tobytes() != er[k].tobytes()]
    assert len(gr) == len(er) and not bad, [(k, gr[k], er[k]) for k in bad[:5]]
    assert gd.tobytes() == ed.tobytes(), np.argwhere(gd != ed)[:5]
    assert gb.tobytes() == eb.tobytes(), np.argwhere(gb != eb)[:5]


# ---- 1. the kernels against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_len,min_depth", [(1, 2), (63, 2), (64, 2), (65, 2), (256, 2), (64, 1), (64, 3), (100, 2)])
@pytest.mark.parametrize("name", ["designed", "crowd"])
def test_consensus_equals_its_definition(ctx, name, max_len, min_depth):
    reads, sites = tables()[name]
    got = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, max_len, min_depth)
    exp = expected(name, max_len, min_depth)
    assert_equal(got, exp)
    kc.check_invariants(*got, max_len)
    assert got[0]["n_reads"].sum() > 300 if name == "crowd" else got[0]["n_reads"].sum() >= 18 * 8
    rows_only = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, max_len, min_depth, col_depth=False)
    assert rows_only[2] is None and rows_only[0].tobytes() == got[0].tobytes() and rows_only[1].tobytes() == got[1].tobytes()


def test_designed_truth_from_the_device(ctx):
    d = kc.designed()
    reads, sites = tables()["designed"]
    rows, bases, depth = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, kc.MAX_LEN, kc.MIN_DEPTH)
    by = {(int(s["tid"]), int(s["pos"]), int(s["dir"])): k for k, s in enumerate(sites)}
    for key, text in d["truth"].items():
        assert bytes(bases[by[key], :int(rows[by[key]]["len"])]).decode() == text, key


@pytest.mark.parametrize("name", ["designed", "crowd"])
def test_two_runs_and_a_permuted_table_give_the_same_bytes(ctx, name):
    reads, sites = tables()[name]
    max_len = 100 if name == "crowd" else 64
    first = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, max_len, 2)
    again = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, max_len, 2)
    perm = np.random.default_rng(9).permutation(len(reads["tid"]))
    moved = ctx.clip_consensus(kc.permuted(reads, perm), sites, QUAL, kc.MIN_CLIP, max_len, 2)
    for other in (again, moved):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, other))
    # other thresholds move the events as the definition says
    got = ctx.clip_consensus(reads, sites, 0, 9, max_len, 2)
    assert_equal(got, kc.expected_consensus(reads, sites, 0, 9, max_len, 2))
    if name == "designed":  # (its reads below -q and its clip of 9; the crowd table has neither)
        assert got[0]["n_reads"].sum() == first[0]["n_reads"].sum() + 2


def test_n_reads_is_the_count_of_clip_reads():
    """on a table without SA tags, 0x100 or 0x800 records the events are those of bk_clip_reads (a record table has no l_seq: the two
    reads whose l_seq is designed to be wrong are left out)"""
    d = kc.designed()
    recs = [r for r in d["ds"].recs if not r.sa and not r.flag & 0x900 and r.qname not in ("xShort", "xNoseq")]
    ds = synth.Dataset(list(cc.CONTIGS), recs)
    cols = ds.to_soa()
    assert (np.diff(cols["aux_off"].astype(np.int64)) == 0).all()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.isize_stats()
    sites = d["sites"]
    counts = t.clip_reads(sites, QUAL, kc.MIN_CLIP, listing=False)
    rows, _, _ = t.clip_consensus(kc.designed_reads(recs), sites, QUAL, kc.MIN_CLIP)  # (on the context that holds the records: nothing of it changes)
    assert counts.sum() == 9 and np.array_equal(counts, rows["n_reads"]), (counts, rows["n_reads"])
    assert np.array_equal(t.clip_reads(sites, QUAL, kc.MIN_CLIP, listing=False), counts)
    t.close()


# ---- 2. errors, limits, empty inputs, timing ------------------------------------------------------------------------------------------
def raw_call(t, reads, sites, n_sites=None, mapq_min=20, min_clip=10, max_len=64, min_depth=2, n=None, null=()):
    C = capi.C
    s, keep = capi.reads_struct(reads)
    if n is not None:
        s.n = n
    sites = np.ascontiguousarray(sites, abi.CLIP_SITE)
    out, bases, depth = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = t.L.bk_clip_consensus(None if "ctx" in null else t.h, None if "reads" in null else C.byref(s), None if "sites" in null else sites.ctypes.data,
                               len(sites) if n_sites is None else n_sites, mapq_min, min_clip, max_len, min_depth, None if "out" in null else C.byref(out),
                               None if "bases" in null else C.byref(bases), C.byref(depth))
    del keep
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_and_limit_errors(ctx):
    reads, sites = kc.crowd_table()
    assert raw_call(ctx, reads, sites)[0] == abi.BK_OK
    for null in ("ctx", "reads", "sites", "out", "bases"):
        assert raw_call(ctx, reads, sites, null=(null,))[0] == abi.BK_ERR_ARG, null
    for kw, word in (({"max_len": 0}, "max_len"), ({"max_len": 257}, "max_len"), ({"min_depth": 0}, "min_depth"), ({"min_clip": 0}, "min_clip"), ({"mapq_min": -1}, "mapq_min")):
        rc, msg = raw_call(ctx, reads, sites, **kw)
        assert rc == abi.BK_ERR_ARG and word in msg, (kw, msg)
    for field, value, word in (("dir", 2, "dir above 1"), ("tol", 1, "tol")):
        bad = sites.copy()
        bad[1][field] = value
        rc, msg = raw_call(ctx, reads, bad)
        assert rc == abi.BK_ERR_ARG and word in msg and "site 1" in msg, msg
    for col, word in (("cigar_off", "cigar_off does not ascend"), ("seq_off", "seq_off does not ascend")):
        bad = dict(reads)
        bad[col] = reads[col].copy()
        bad[col][5] = bad[col][7] + 1
        rc, msg = raw_call(ctx, bad, sites)
        assert rc == abi.BK_ERR_ARG and word in msg, msg
    bad = dict(reads)
    bad["l_seq"] = reads["l_seq"].copy()
    bad["l_seq"][3] += 2  # one byte more than its span holds
    rc, msg = raw_call(ctx, bad, sites)
    assert rc == abi.BK_ERR_ARG and "read 3" in msg and "seq bytes" in msg, msg
    # the limits are looked at before any column: the small arrays are never read beyond their end
    rc, msg = raw_call(ctx, reads, sites, n=(1 << 32) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^32 reads" in msg, msg
    rc, msg = raw_call(ctx, reads, sites, n_sites=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 sites" in msg, msg
    s = capi.Context(cc.CONTIGS)
    ds = cc.quiet_tumor()
    s.upload(ds.to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.clip_consensus(reads, sites, QUAL, 10)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_equal(ctx.clip_consensus(reads, sites, QUAL, 10, 100, 2), expected("crowd", 100, 2))  # the context still works


def test_empty_table_and_empty_site_list(ctx):
    reads, sites = tables()["crowd"]
    rows, bases, depth = ctx.clip_consensus(reads, np.zeros(0, abi.CLIP_SITE), QUAL, 10)
    assert len(rows) == 0 and bases.shape == (0, 64) and depth.shape == (0, 64)
    none = kc.make_reads([])
    rows, bases, depth = ctx.clip_consensus(none, sites, QUAL, 10, 100, 2)
    assert len(rows) == len(sites) and not rows.tobytes().strip(b"\0") and not bases.any() and not depth.any()
    only_gone = sites[[1, 2]]  # an empty site and one with tid = -1
    rows, bases, depth = ctx.clip_consensus(reads, only_gone, QUAL, 10)
    assert not rows.tobytes().strip(b"\0") and not bases.any() and not depth.any()


def test_consensus_is_timed():
    reads, sites = tables()["crowd"]
    t = capi.Context(cc.CONTIGS)
    t.timing_enable(True)
    rows, bases, depth = t.clip_consensus(reads, sites, QUAL, 10, 100, 2)
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "consensus" in tm and tm["consensus"][0] > 0 and tm["consensus"][1] > 0
    # the byte model: the CIGAR words of both walks and ceil(min(c, max_len) / 2) bytes of SEQ per contribution
    seq_bytes = 2 * 300 * 45 + sum((int(c) + 1) // 2 for c in (reads["cigar"][reads["cigar_off"][:-1]] >> 4)[reads["pos"] == 6999])
    assert touched["consensus"] >= seq_bytes + 2 * 4 * len(reads["cigar"]) + rows.nbytes + bases.nbytes + depth.nbytes
    t.close()


# ---- 3. command line --------------------------------------------------------------------------------------------------------------
CONS_COLUMNS = ["Cons_N1", "Cons_Len1", "Cons_Agree1", "Cons_Seq1", "Cons_N2", "Cons_Len2", "Cons_Agree2", "Cons_Seq2"]
INFO_LINES = ("##INFO=<ID=CSEQ,Number=1,Type=String,", "##INFO=<ID=CSN,Number=1,Type=Integer,")


@pytest.fixture(scope="module")
def designed_run():
    """the designed BAM with its side files, and its records as a table"""
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "t.bam")
        kc.write_designed_bam(bam)
        from breakid_amd import bamio
        bamio.write_bai(bam)
        ds = kc.designed()["ds"]
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        yield tmp, bam, side, env


def outputs(tmp, prefix):
    return sorted(f[len(prefix):] for f in os.listdir(tmp) if f.startswith(prefix + "_"))


@pytest.mark.parametrize("variant", ["plain", "everything"])
@pytest.mark.parametrize("mode", ["fast", "default"])
def test_cli_consensus(designed_run, mode, variant):
    tmp, bam, side, env = designed_run
    d = kc.designed()
    ds = d["ds"]
    reads, _ = tables()["designed"]
    conslen = 64 if variant == "plain" else 50
    extra = (["-fast"] if mode == "fast" else []) + (["-all", "-vcf", "-evidence", "-dedup", "-clip"] if variant != "plain" else [])
    base = [BIN, "-i", bam, "-n", side["nib"]] + extra
    a, b = os.path.join(tmp, "a_%s_%s" % (mode, variant)), os.path.join(tmp, "b_%s_%s" % (mode, variant))
    r = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-o", b, "-consensus"] + (["-conslen", "50"] if conslen != 64 else []), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # the API on the same records: the calls and their sides
    t = capi.Context(ds.contigs)
    t.upload(ds.to_soa())
    t.run(qual=QUAL, fast=mode == "fast")
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    js = t.junctions()
    t.close()
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_consensus.txt"] + (["_fusion_all_consensus.txt"] if variant != "plain" else [])
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa, fb = outputs(tmp, pa), outputs(tmp, pb)
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt"} | ({"_fusion.vcf"} if variant != "plain" else set())
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    if variant != "plain":
        assert {"_fusion_rescued.txt", "_fusion_rescued.vcf", "_evidence.txt", "_evidence.bam", "_fusion_all_dedup.txt", "_fusion_all_clip.txt"} <= set(fa) - changed
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "consensus_max_len\t%d\n" % conslen, (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then per side the definition's numbers at (ps_tid, ps_exact, 0, d_s)
    truth_seen = set()
    side_of = {}
    for twin in twins:
        plain = twin.replace("_consensus", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(CONS_COLUMNS)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) >= (4 if plain == "_fusion.txt" else 9)
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        sites = []
        for i in calls:
            d1, d2 = clipcases.junction_sides(js[i])
            sites += [(int(cl[i]["p1_tid"]), int(cl[i]["p1_exact"]), 0, d1), (int(cl[i]["p2_tid"]), int(cl[i]["p2_exact"]), 0, d2)]
        rows, bases, _ = kc.expected_consensus(reads, kc.as_sites(sites), QUAL, kc.MIN_CLIP, conslen, kc.MIN_DEPTH)
        where = {i: 2 * k for k, i in enumerate(calls)}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            k = where[i]
            fields = kc.side_text(rows[k], bases[k], sites[k][3]) + kc.side_text(rows[k + 1], bases[k + 1], sites[k + 1][3])
            assert line == s + "\t" + "\t".join(fields), (line, fields)
            for x in (k, k + 1):
                side_of[(i, x - k)] = (int(rows[x]["n_reads"]), fields[4 * (x - k) + 3])
                key = (sites[x][0], sites[x][1], sites[x][3])
                if key in d["truth"]:  # ... and the designed partner sequence, as the BAM reads it
                    text = d["truth"][key][:conslen]
                    assert fields[4 * (x - k) + 3] == (text[::-1] if sites[x][3] == kc.RIGHT else text), (key, fields)
                    truth_seen.add(key)
    want = {k for k in d["truth"] if variant != "plain" or any(k[:2] == (L[1], L[2]) or k[:2] == (L[4], L[5]) for L in cc.LOCI[:4])}
    assert truth_seen == want and len(want) == (8 if variant == "plain" else 18)
    if variant == "plain":
        return
    # 3. the VCF: CSEQ / CSN last in INFO on each breakend for its own side, their header lines, nothing else touched
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 2 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 2 * len(written_calls(cl, b + "_fusion_all.txt"))
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i, s = int(y[2][2:].split("_")[0]), int(y[2].split("_")[1]) - 1
        n, seq = side_of[(i, s)]
        assert "UPE=" in x[7] and y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + (";CSEQ=" + seq if seq != "." else "") + ";CSN=%d" % n, lb
    assert any(";CSEQ=" in l for l in body_b)


def test_cli_consensus_of_a_sample_without_calls_and_errors():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        r = subprocess.run(base + ["-consensus", "-gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-consensus cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
        for bad in (["-conslen", "0"], ["-conslen", "257"]):
            r = subprocess.run(base + ["-consensus"] + bad, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and "-conslen must be a number from 1 to 256" in r.stderr, r.stderr[-2000:]
        r = subprocess.run(base + ["-conslen", "10"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-conslen needs -consensus" in r.stderr, r.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-consensus", "-vcf", "-minclip", "12"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_consensus.txt", "_fusion_all_consensus.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(CONS_COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("consensus_max_len\t64\n")

"""Window coverage (`bk_window_coverage`, `-coverage`): the kernels against the numpy definition (tests/coveragecases.py) byte for byte
at every tile boundary and on a table large enough for the sampled search keys; window edges on and around record edges; records that
reach across an edge but do not count; a long record among short ones; a contig and sums beyond 32 bits; two runs, a permuted window
list and two thresholds on one context; every table form; errors; timing; and the command line's files against the definition."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import coveragecases as vc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = [("c0", 3_000_000), ("c1", 1_000_000), ("c2", 500_000), ("big", 2_000_000_000)]
NT = len(CONTIGS)


def context(cols, where="host", contigs=CONTIGS):
    t, keep = cc.make_ctx(contigs, cols, where)
    t.isize_stats()
    return t, keep


def assert_rows(got, exp):
    assert got.dtype == abi.WINDOW_COV and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def edge_windows(cols, rng, n_records=40, n_random=60, contigs=CONTIGS):
    """windows on a record's pos and endpos and one base either side of each (inside one record, exactly one record, one base more),
    single bases at both ends, random ones, whole contigs, in front of a contig's first record and behind its last"""
    rows = [(-1, 0, 100), (NT, 0, 100), (0, 50, 50), (0, 60, 50)]
    n = len(cols["tid"])
    ln = vc.eligible_len(cols, 0)
    mapped = np.flatnonzero(cols["tid"] >= 0)
    for i in (rng.choice(mapped, min(n_records, len(mapped)), replace=False) if len(mapped) else []):
        t, p = int(cols["tid"][i]), int(cols["pos"][i])
        e = p + max(1, int(ln[i]))
        rows += [(t, max(0, p + d), e + d2) for d in (-1, 0, 1) for d2 in (-1, 0, 1)]
        rows += [(t, p, p + 1), (t, max(0, p - 1), p), (t, e - 1, e), (t, e, e + 1)]
    for t, (_, length) in enumerate(contigs[:3]):
        m = cols["tid"] == t
        rows += [(t, 0, length), (t, 0, 1), (t, length - 1, length), (t, length, length + 1000)]
        if m.any():
            first, last = int(cols["pos"][m].min()), int((cols["pos"][m].astype(np.int64) + ln[m]).max())
            rows += [(t, 0, first), (t, 0, first + 1), (t, last, length), (t, max(0, last - 1), length)]
        for _ in range(n_random // 3):
            a = int(rng.integers(0, max(1, min(length, 30_000))))
            rows.append((t, a, a + int(rng.integers(1, 3000))))
    assert n >= 0
    return vc.as_windows(rows)


# ---- 1. tile boundaries and the partial tile -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513])
def test_record_counts_at_the_tile_boundaries(n):
    """n records in all; from two on the last one is unmapped (tid -1 behind the last contig's records); contig c1 has none"""
    rng = np.random.default_rng(100 + n)
    cols = vc.random_table(rng, n - (n >= 2), [(0, 20_000), (2, 8_000)], read_len=150, unmapped=int(n >= 2))
    assert len(cols["tid"]) == n
    windows = edge_windows(cols, rng)
    t, _ = context(cols)
    for q in (0, 20):
        exp = vc.expected_cov(cols, NT, windows, q)
        assert_rows(t.window_coverage(windows, q), exp)
        assert n < 255 or int(exp["bases"].max()) > 5_000
    assert not t.window_coverage(windows[:4], 0).tobytes().strip(b"\0")
    t.close()


# ---- 2. the sampled search keys; windows across tiles ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    """70 000 records (more than 64 strides of 1024: rec_lower searches its sampled keys first) on two contigs, 40 unmapped behind them"""
    rng = np.random.default_rng(7)
    cols = vc.random_table(rng, 70_000 - 40, [(0, 2_900_000), (2, 400_000)], read_len=150, unmapped=40)
    t, _ = context(cols)
    yield cols, t
    t.close()


def test_sampled_keys_and_windows_across_tiles(large):
    cols, t = large
    rng = np.random.default_rng(8)
    windows = edge_windows(cols, rng, n_records=60, n_random=90)
    rows = []
    pos, tid = cols["pos"], cols["tid"]
    for tile in (0, 1, 17, 60, 100, 125):
        for ahead in (1, 3):
            i, j = 256 * tile + 200, 256 * (tile + ahead) + 10
            assert tid[i] == tid[j] == 0
            rows += [(0, int(pos[i]), int(pos[j])), (0, int(pos[i]) + 1, int(pos[j]) + 149), (0, int(pos[256 * tile]), int(pos[256 * (tile + ahead)]))]
    last0 = int(np.flatnonzero(tid == 0)[-1])  # the last records of a contig, with those of the next one in the same tile
    rows += [(0, int(pos[last0 - 300]), 3_000_000), (2, 0, int(pos[last0 + 300])), (2, 0, 500_000), (2, 399_000, 500_000), (1, 0, 1_000_000)]
    windows = np.concatenate([windows, vc.as_windows(rows)])
    for q in (0, 30):
        assert_rows(t.window_coverage(windows, q), vc.expected_cov(cols, NT, windows, q))
    whole = t.window_coverage(vc.as_windows([(0, 0, 3_000_000), (2, 0, 500_000), (3, 0, 2_000_000_000)]), 0)
    ln = vc.eligible_len(cols, 0)
    assert int(whole["bases"].sum()) == int(ln.sum()) and int(whole["reads"].sum()) == int((ln > 0).sum()) and int(whole[2]["reads"]) == 0


# ---- 3. records that reach across an edge but do not count ----------------------------------------------------------------------------
def test_straddling_records_that_are_not_eligible_are_not_subtracted():
    q = 20
    plain = [(0, 1000 + 10 * k, 0x1, 60, "100M") for k in range(300)]
    edge = 2500
    barred = [(0, edge - 50, 0x1 | f, 60, "100M") for f in (0x4, 0x100, 0x200, 0x400, 0x800)]
    barred += [(0, edge - 50, 0x1, q - 1, "100M"), (0, edge - 50, 0x1, 60, "100S"), (0, edge - 50, 0x1, 60, "30S10I60S"), (0, edge - 50, 0x1, 60, "")]
    counted = [(0, edge - 50, 0x1, q, "100M"), (0, edge - 30, 0x1 | 0x10 | 0x2, 60, "10S50M7D40M")]
    windows = vc.as_windows([(0, edge, edge + 500), (0, edge - 500, edge), (0, edge - 50, edge + 50), (0, edge - 1, edge + 1), (0, 0, edge), (0, edge, 10_000), (0, edge - 49, edge + 49)])
    rows = {}
    for name, recs in (("plain", plain + counted), ("all", plain + counted + barred)):
        cols = vc.make_cols(recs)
        t, _ = context(cols)
        rows[name] = t.window_coverage(windows, q)
        assert_rows(rows[name], vc.expected_cov(cols, NT, windows, q))
        if name == "all":  # at threshold 0 the record one below the threshold counts
            low = t.window_coverage(windows, 0)
            assert_rows(low, vc.expected_cov(cols, NT, windows, 0))
            assert int(low[2]["bases"]) == int(rows[name][2]["bases"]) + 100 and int(low[2]["reads"]) == int(rows[name][2]["reads"]) + 1
        t.close()
    assert rows["plain"].tobytes() == rows["all"].tobytes()


# ---- 4. a long record among short ones ------------------------------------------------------------------------------------------------
def test_a_long_record_widens_the_walk():
    rng = np.random.default_rng(12)
    recs = [(0, int(p), 0x1, int(rng.integers(0, 61)), "150M") for p in rng.integers(0, 300_000, 6000)]
    recs += [(0, 50_000, 0x1, 60, "75M99850N75M"), (0, 120_000, 0x1, 60, "50M100000D50M"), (2, 10, 0x1, 60, "100M")]
    cols = vc.make_cols(recs)
    rows = [(0, 50_000, 150_000), (0, 50_075, 149_925), (0, 149_999, 150_001), (0, 150_000, 150_100), (0, 100_000, 100_001), (0, 220_099, 220_101), (0, 0, 3_000_000), (0, 149_000, 151_000)]
    windows = np.concatenate([edge_windows(cols, rng), vc.as_windows(rows)])
    t, _ = context(cols)
    for q in (0, 20):
        got = t.window_coverage(windows, q)
        assert_rows(got, vc.expected_cov(cols, NT, windows, q))
    one = t.window_coverage(vc.as_windows([(0, 100_000, 100_001)]), 61)[0]  # only the two long records reach mapq 60... none reaches 61
    assert (int(one["bases"]), int(one["reads"])) == (0, 0)
    t.close()


# ---- 5. beyond 32 bits ----------------------------------------------------------------------------------------------------------------
def test_a_contig_and_sums_beyond_32_bits():
    """eight records of 10^9 aligned bases (four CIGAR words of 250 000 000M: one word holds 28 bits) on a contig of 2 * 10^9"""
    long = "250000000M" * 4
    recs = [(3, 100_000_000 * k, 0x1, 60, long) for k in range(8)] + [(0, 5, 0x1, 60, "100M"), (-1, -1, 0x4, 0, "")]
    cols = vc.make_cols(recs)
    rows = [(3, 0, 2_000_000_000), (3, 0, 0xFFFFFFFF), (3, 1_500_000_000, 2_000_000_000), (3, 999_999_999, 1_000_000_001), (3, (1 << 31) - 5, (1 << 31) + 5),
            (3, 0xFFFFFFF0, 0xFFFFFFFF), (3, 700_000_000, 1_000_000_000), (3, 1_700_000_000, 1_700_000_001), (3, 1_699_999_999, 1_700_000_000), (0, 0, 3_000_000),
            (3, 99_999_999, 100_000_001), (2, 0, 0xFFFFFFFF)]
    windows = vc.as_windows(rows)
    t, _ = context(cols)
    got = t.window_coverage(windows, 0)
    assert_rows(got, vc.expected_cov(cols, NT, windows, 0))
    assert int(got[0]["bases"]) == 8 * 10**9 > 1 << 32 and int(got[0]["reads"]) == 8
    assert (int(got[6]["bases"]), int(got[6]["reads"])) == (300_000_000 * 8, 8) and (int(got[7]["bases"]), int(got[8]["bases"])) == (0, 1)
    assert not got[4:6].tobytes().strip(b"\0") and int(got[9]["bases"]) == 100
    t.close()


# ---- 6. same bytes --------------------------------------------------------------------------------------------------------------------
def test_two_runs_a_permuted_list_and_two_thresholds(large):
    cols, t = large
    rng = np.random.default_rng(9)
    windows = edge_windows(cols, rng, n_records=50)
    first = t.window_coverage(windows, 20)
    again = t.window_coverage(windows, 20)
    perm = rng.permutation(len(windows))
    moved = t.window_coverage(windows[perm], 20)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()
    # the tile sums belong to the threshold of the call: 50, then 5, then 50 again, each equal to its own definition
    hi, lo = vc.expected_cov(cols, NT, windows, 50), vc.expected_cov(cols, NT, windows, 5)
    assert int(lo["bases"].sum()) > int(hi["bases"].sum()) * 2
    assert_rows(t.window_coverage(windows, 50), hi)
    assert_rows(t.window_coverage(windows, 5), lo)
    assert_rows(t.window_coverage(windows, 50), hi)


# ---- 7. table forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_table_forms_and_the_excluded_table(where):
    rng = np.random.default_rng(15)
    cols = vc.random_table(rng, 3000, [(0, 60_000), (2, 30_000)], read_len=150, unmapped=5)
    windows = edge_windows(cols, rng)
    t, keep = context(cols, where)
    assert_rows(t.window_coverage(windows, 10), vc.expected_cov(cols, NT, windows, 10))
    t.close()
    # bk_exclude_regions: the records that overlap an interval count nowhere
    tid, beg, end = np.asarray([0, 2], np.int32), np.asarray([10_000, 0], np.int32), np.asarray([12_000, 5_000], np.int32)
    x, keep2 = cc.make_ctx(CONTIGS, cols, where)
    removed = x.exclude_regions(tid, beg, end)
    x.isize_stats()
    kept = cc.filtered(cols, ~cc.excluded_mask(cols, tid, beg, end))
    assert removed == len(cols["tid"]) - len(kept["tid"]) > 100
    more = np.concatenate([windows, vc.as_windows([(0, 9_000, 13_000), (0, 10_000, 12_000), (2, 0, 5_000), (2, 0, 6_000)])])
    got = x.window_coverage(more, 10)
    assert_rows(got, vc.expected_cov(kept, NT, more, 10))
    assert int(got[-3]["bases"]) == 0 and int(got[-2]["bases"]) == 0 and int(got[-1]["bases"]) > 0
    x.close()
    del keep, keep2


# ---- 8. errors, empty inputs ----------------------------------------------------------------------------------------------------------
def raw_call(t, windows, mapq_min=0, n=None, null=()):
    C = capi.C
    windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
    out = C.c_void_p()
    rc = t.L.bk_window_coverage(None if "ctx" in null else t.h, None if "windows" in null else windows.ctypes.data, len(windows) if n is None else n, mapq_min,
                                None if "out" in null else C.byref(out))
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_errors(large):
    cols, t = large
    windows = vc.as_windows([(0, 1000, 2000), (2, 0, 500)])
    assert raw_call(t, windows)[0] == abi.BK_OK
    for null in ("ctx", "windows", "out"):
        assert raw_call(t, windows, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(t, windows, n=0, null=("windows",))[0] == abi.BK_OK
    none = t.window_coverage(np.zeros(0, abi.COV_WINDOW), 0)
    assert len(none) == 0 and none.dtype == abi.WINDOW_COV
    rc, msg = raw_call(t, windows, mapq_min=-1)
    assert rc == abi.BK_ERR_ARG and "mapq_min" in msg, msg
    bad = windows.copy()
    bad[1]["reserved"] = 7
    rc, msg = raw_call(t, bad)
    assert rc == abi.BK_ERR_ARG and "reserved" in msg and "window 1" in msg, msg
    rc, msg = raw_call(t, windows, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 windows" in msg, msg
    small = vc.random_table(np.random.default_rng(1), 300, [(0, 20_000)], unmapped=0)
    early = capi.Context(CONTIGS)
    with pytest.raises(capi.BreakIDError, match="bk_isize_stats first") as e:
        early.window_coverage(windows)  # no table at all
    assert e.value.code == abi.BK_ERR_ARG
    early.upload(small)
    with pytest.raises(capi.BreakIDError, match="bk_isize_stats first") as e:
        early.window_coverage(windows)
    assert e.value.code == abi.BK_ERR_ARG
    early.isize_stats()
    assert_rows(early.window_coverage(windows, 0), vc.expected_cov(small, NT, windows, 0))
    early.close()
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.window_coverage(windows)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(t.window_coverage(windows, 0), vc.expected_cov(cols, NT, windows, 0))  # the context still works


# ---- 9. command line, timing -----------------------------------------------------------------------------------------------------------------
# one call across two contigs (the first designed locus of callcases, with its genes), a deletion whose span lies at half the depth of
# its flanks, a duplication at twice the depth, and a call 600 bases from a contig's start, where a flank of 1000 is clamped
COV_LOCI = [("X", 0, 300_000, "L", 1, 700_000, "R"), ("DEL", 0, 1_000_000, "L", 0, 1_010_000, "R"), ("DUP", 2, 1_200_000, "R", 2, 1_210_000, "L"),
            ("START", 3, 600, "R", 1, 1_500_000, "L")]
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=Float," % k for k in ("COVL", "COVR", "RDRATIO"))


def tile(ds, tag, tid, lo, hi, step):
    """proper pairs of two 100M reads 200 apart, one pair every `step` bases: a depth of 200 / step"""
    for k, s in enumerate(range(lo, hi, step)):
        q = "%s_%d" % (tag, k)
        ds.recs += [synth.Rec(q, 0x1 | 0x2 | 0x20 | 0x40, tid, s, 60, "100M", tid, s + 200, 300), synth.Rec(q, 0x1 | 0x2 | 0x10 | 0x80, tid, s + 200, 60, "100M", tid, s, -300)]


def coverage_tumor():
    ds = cc.designed_tumor(mix=False, loci=COV_LOCI, n_proper=3000)
    tile(ds, "delL", 0, 997_000, 1_000_000, 10)
    tile(ds, "delS", 0, 1_000_000, 1_010_000, 20)
    tile(ds, "delR", 0, 1_010_000, 1_013_000, 10)
    tile(ds, "dupL", 2, 1_197_000, 1_200_000, 10)
    tile(ds, "dupS", 2, 1_200_000, 1_210_000, 5)
    tile(ds, "dupR", 2, 1_210_000, 1_213_000, 10)
    ds.sort()
    return ds


def coverage_normal():
    ds = cc.quiet_tumor()
    tile(ds, "ndel", 0, 997_000, 1_013_000, 20)
    tile(ds, "ndup", 2, 1_197_000, 1_213_000, 25)
    tile(ds, "nstart", 3, 0, 3_000, 50)
    ds.sort()
    return ds


@pytest.fixture(scope="module")
def cov_run():
    with tempfile.TemporaryDirectory() as tmp:
        ds, nor = coverage_tumor(), coverage_normal()
        bam, nbam = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        cc.write_indexed(ds, bam)
        nor.write_bam(nbam, aligned=True)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        cols = ds.to_soa()
        t = capi.Context(ds.contigs)
        t.upload(cols)
        t.run(qual=QUAL, fast=True)
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        sides = [capi.junction_sides(j)[:2] for j in t.junctions()]
        t.close()
        yield {"tmp": tmp, "bam": bam, "nbam": nbam, "nib": side["nib"], "env": env, "cl": cl, "sides": sides, "cols": cols, "ncols": nor.to_soa()}


# (timing, and what a later stage returns)
def test_coverage_is_timed_and_changes_no_stage(cov_run):
    """on the designed tumour of the command-line tests: the call stands between bk_isize_stats and the stages, and the clusters
    that come out are those of a context that never made it"""
    cols, want = cov_run["cols"], cov_run["cl"]
    t = capi.Context(cc.CONTIGS)
    t.upload(cols)
    t.isize_stats()
    t.timing_enable(True)
    windows = vc.as_windows([(0, 299_000, 301_000), (1, 0, 2_000_000), (3, 5, 10)])
    got = t.window_coverage(windows, QUAL)
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    n, nw = len(cols["tid"]), int(cols["cigar_off"][-1])
    model = 11 * n + 4 * nw + 16 * ((n + 255) // 256) + 32 * len(windows)
    assert names[-3:] == ["window_coverage", "window_coverage_tiles", "window_coverage_windows"]
    assert tm["window_coverage"][0] > 0 and tm["window_coverage"][1] == model and touched["window_coverage"] == model > 0
    assert tm["window_coverage"][0] >= tm["window_coverage_tiles"][0] > 0 and tm["window_coverage"][0] >= tm["window_coverage_windows"][0] > 0
    assert touched["window_coverage_tiles"] + touched["window_coverage_windows"] == model
    t.timing_enable(False)
    assert_rows(got, vc.expected_cov(cols, len(cc.CONTIGS), windows, QUAL))
    t.run(qual=QUAL, fast=True)
    assert t.fetch(abi.STAGE_CLUSTERS)[0].tobytes() == want.tobytes()
    assert_rows(t.window_coverage(windows, QUAL), got)
    t.close()


def locus_of(c):
    for name, ta, pa, _, tb, pb, _ in COV_LOCI:
        if {(int(c["p1_tid"]), int(c["p1_exact"])), (int(c["p2_tid"]), int(c["p2_exact"]))} == {(ta, pa), (tb, pb)}:
            return name
    return None


@pytest.mark.parametrize("variant", ["plain", "everything"])
def test_cli_coverage(cov_run, variant):
    run = cov_run
    tmp, cl, sides = run["tmp"], run["cl"], run["sides"]
    lens = np.asarray([l for _, l in cc.CONTIGS], np.uint32)
    flank = 1000 if variant == "plain" else 700
    with_normal = variant == "everything"
    extra = [] if variant == "plain" else ["-vcf", "-normal", run["nbam"], "-genotype"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-all", "-fast"] + extra
    a, b = os.path.join(tmp, "a_" + variant), os.path.join(tmp, "b_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-coverage"] + ([] if variant == "plain" else ["-covflank", "700"]), env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [l for l in r.stdout.split("\n") if "costs time" not in l] == [l for l in out_a.replace(a, b).split("\n") if "costs time" not in l]  # stdout gains nothing
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_coverage.txt", "_fusion_coverage.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt", "_fusion.vcf"}
    for suffix in fa:
        if suffix not in changed:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
    if with_normal:
        assert {"_fusion_normal.txt", "_fusion_genotype.txt", "_fusion.vcf"} <= set(fa)
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "coverage_flank\t%d\n" % flank, (ta, tb)
    # 2. the twins: the rows of their fusion table in its order, then the definition's columns
    columns = vc.COLUMNS + (["Normal_" + c for c in vc.COLUMNS] if with_normal else [])
    seen = {}
    for twin in twins:
        plain = twin.replace("_coverage", "")
        lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(columns)
        calls = written_calls(cl, b + plain)
        assert len(calls) == len(lines) - 2 and len(calls) == (1 if plain == "_fusion.txt" else 4)
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            exp, w = vc.expected_call_fields(cl[i], sides[i][0], sides[i][1], flank, lens, run["cols"], QUAL)
            if with_normal:
                exp = exp + vc.expected_call_fields(cl[i], sides[i][0], sides[i][1], flank, lens, run["ncols"], QUAL)[0]
            assert line == s + "\t" + "\t".join(exp), (line, exp)
            seen[i] = (exp, w)
    # the designed calls by what they were designed for
    by_name = {locus_of(cl[i]): i for i in seen}
    assert set(by_name) == {"X", "DEL", "DUP", "START"}
    f = seen[by_name["X"]][0]
    assert f[4] == "." and f[5] == "." and "." not in f[:4] + f[6:8]
    f = seen[by_name["DEL"]][0]
    assert 0.35 < float(f[5]) < 0.6 and 9.0 < float(f[4]) < 12.0 and f[6] == f[7], f
    f = seen[by_name["DUP"]][0]
    assert 1.6 < float(f[5]) < 2.2 and 38.0 < float(f[4]) < 43.0, f
    if with_normal:
        assert 0.9 < float(seen[by_name["DEL"]][0][8 + 5]) < 1.1 and 0.9 < float(seen[by_name["DUP"]][0][8 + 5]) < 1.1
    f, w = seen[by_name["START"]]
    s = 0 if int(cl[by_name["START"]]["p1_tid"]) == 3 else 1
    assert (int(w[2 * s]["beg"]), int(w[2 * s]["end"])) == (0, 599) and int(w[2 * s + 1]["end"]) - int(w[2 * s + 1]["beg"]) == flank and f[2 * s] != "." and f[4] == "."
    # 3. the VCF: COVL / COVR of the breakend's own side and RDRATIO last in INFO, their header lines, nothing else touched
    if variant == "plain":
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 8
    with_ratio = 0
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i = int(y[2][2:].split("_")[0])
        side = int(y[2].split("_")[1]) - 1
        f = seen[i][0]
        tail = ";COVL=%s;COVR=%s" % (f[2 * side], f[2 * side + 1]) + (";RDRATIO=" + f[5] if f[5] != "." else "")
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail, lb
        with_ratio += f[5] != "."
    assert with_ratio == 4


def test_cli_coverage_limits_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-covflank", "100"], "-covflank needs -coverage."), (["-coverage", "-gpus", "2"], "-coverage cannot be combined with -gpus."),
                           (["-coverage", "-covflank", "0"], "-covflank must be a number from 1 to 1000000."),
                           (["-coverage", "-covflank", "1000001"], "-covflank must be a number from 1 to 1000000."),
                           (["-coverage", "-covflank", "5", "-simflank", "3"], "-simflank needs -similar.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        header = None
        for flank in ("1", "1000000"):
            r = subprocess.run(base + ["-coverage", "-vcf", "-covflank", flank], env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            header = open(prefix + "_fusion.txt").read()
            assert header.count("\n") == 1
            for twin in ("_fusion_coverage.txt", "_fusion_all_coverage.txt"):
                assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(vc.COLUMNS) + "\n"
            assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
            assert open(prefix + "_params.txt").read().endswith("vcf\t1\ncoverage_flank\t%s\n" % flank)

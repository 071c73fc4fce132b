"""Window context (`bk_window_context`, `-context`): the kernels against the numpy definition (tests/contextcases.py) byte for byte at
every tile boundary and on a table large enough for the sampled search keys; window edges on and around record starts; every class
one by one; pile-ups across tiles; two runs, a permuted window list and two thresholds on one context; every table form; errors;
timing and its byte model; and the command line's files against the definition."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import contextcases as xc
from tests import coveragecases as vc
from tests.test_cpu_context import DESIGNED, Q, designed_table
from tests.test_gpu_coverage import cov_run  # noqa: F401  (the designed inputs of the -coverage command-line test, as a fixture)
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = [("c0", 3_000_000), ("c1", 1_000_000), ("c2", 500_000), ("big", 2_000_000_000)]
NT = len(CONTIGS)
ZERO_ROWS = [(-1, 0, 100), (NT, 0, 100), (0, 50, 50), (0, 60, 50)]


def assert_rows(got, exp):
    assert got.dtype == abi.WINDOW_CTX and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def start_windows(cols, rng, n_records=40, n_random=45, contigs=CONTIGS):
    """windows with an edge on a record's pos and one base either side of it (pos == beg counts, pos == end does not), single bases,
    random ones, whole contigs, the stretch in front of a contig's first record and behind its last, and the four zero rows"""
    rows = list(ZERO_ROWS)
    mapped = np.flatnonzero(cols["tid"] >= 0)
    for i in (rng.choice(mapped, min(n_records, len(mapped)), replace=False) if len(mapped) else []):
        t, p = int(cols["tid"][i]), int(cols["pos"][i])
        rows += [(t, max(0, p + d), p + 300) for d in (-1, 0, 1)] + [(t, max(0, p - 300), max(0, p + d)) for d in (-1, 0, 1)]
        rows += [(t, p, p + 1), (t, max(0, p - 1), p), (t, p + 1, p + 2)]
    for t, (_, length) in enumerate(contigs[:3]):
        m = cols["tid"] == t
        rows += [(t, 0, length), (t, 0, 1), (t, length - 1, length), (t, length, length + 1000), (t, 0, 0xFFFFFFFF)]
        if m.any():
            first, last = int(cols["pos"][m].min()), int(cols["pos"][m].max())
            rows += [(t, 0, first), (t, 0, first + 1), (t, last + 1, length), (t, last, length)]
        for _ in range(n_random // 3):
            a = int(rng.integers(0, max(1, min(length, 30_000))))
            rows.append((t, a, a + int(rng.integers(1, 3000))))
    return xc.as_windows(rows)


# ---- 5b. independence: no other result changes ----------------------------------------------------------------------------------------
def test_the_call_changes_no_other_result(cov_run):  # noqa: F811
    """on the designed tumour of the command-line tests: before bk_isize_stats, between the stages and after them; window coverage and
    the fetched stages are those of a context that never made the call.  (Part of 5 below; it stands first because it runs the
    stages, which are at their best while no other context of the process is alive: the `large` table of the later tests is.)"""
    cols, want = cov_run["cols"], cov_run["cl"]
    nt = len(cc.CONTIGS)
    windows = vc.as_windows([(0, 299_000, 301_000), (1, 0, 2_000_000), (3, 5, 10), (2, 1_199_000, 1_201_000)])
    exp = xc.expected_ctx(cols, nt, windows, QUAL)
    t = capi.Context(cc.CONTIGS)
    t.upload(cols)
    assert_rows(t.window_context(windows, QUAL), exp)  # no bk_isize_stats yet
    t.isize_stats()
    cov = t.window_coverage(windows, QUAL)
    assert_rows(t.window_context(windows, QUAL), exp)
    assert t.window_coverage(windows, QUAL).tobytes() == cov.tobytes()
    t.run(qual=QUAL, fast=True)
    stages = (abi.STAGE_SCAN, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)
    before = [t.fetch(s)[0].tobytes() for s in stages]
    assert before[3] == want.tobytes()
    assert_rows(t.window_context(windows, 0), xc.expected_ctx(cols, nt, windows, 0))
    assert [t.fetch(s)[0].tobytes() for s in stages] == before
    assert t.window_coverage(windows, QUAL).tobytes() == cov.tobytes()
    t.close()


# ---- 1. tile boundaries and the partial tile -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513])
def test_record_counts_at_the_tile_boundaries(n):
    """n records in all; from two on the last one is unmapped (tid -1 behind the last contig's records); contig c1 has none"""
    rng = np.random.default_rng(200 + n)
    cols = xc.random_table(rng, n - (n >= 2), [(0, 20_000), (2, 8_000)], read_len=100, unmapped=int(n >= 2))
    assert len(cols["tid"]) == n
    windows = start_windows(cols, rng)
    t, _ = cc.make_ctx(CONTIGS, cols, "host")
    for q in (0, 20):
        exp = xc.expected_ctx(cols, NT, windows, q)
        assert_rows(t.window_context(windows, q), exp)
        assert n < 255 or min(int(exp[f].max()) for f in xc.FIELDS if f != "lowq" or q) > 0
    assert not t.window_context(windows[:4], 0).tobytes().strip(b"\0")
    t.close()


# ---- 2. the sampled search keys; windows across tiles ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    """70 000 records (more than 64 strides of 1024: rec_lower searches its sampled keys first) on two contigs, 40 unmapped behind them"""
    rng = np.random.default_rng(17)
    cols = xc.random_table(rng, 70_000 - 40, [(0, 2_900_000), (2, 400_000)], read_len=100, unmapped=40)
    t, _ = cc.make_ctx(CONTIGS, cols, "host")
    yield cols, t
    t.close()


def test_sampled_keys_and_windows_across_tiles(large):
    cols, t = large
    rng = np.random.default_rng(18)
    windows = start_windows(cols, rng, n_records=30, n_random=30)
    rows = []
    pos, tid = cols["pos"], cols["tid"]
    for tile in (0, 1, 17, 60, 100, 125):
        for ahead in (1, 3):
            i, j = 256 * tile + 200, 256 * (tile + ahead) + 10
            assert tid[i] == tid[j] == 0
            rows += [(0, int(pos[i]), int(pos[j])), (0, int(pos[i]) + 1, int(pos[j]) + 1), (0, int(pos[256 * tile]), int(pos[256 * (tile + ahead)]))]
    last0 = int(np.flatnonzero(tid == 0)[-1])  # the last records of a contig, with those of the next one in the same tile
    rows += [(0, int(pos[last0 - 300]), 3_000_000), (0, int(pos[last0]), int(pos[last0]) + 1), (2, 0, int(pos[last0 + 300])), (2, 0, int(pos[last0 + 1]) + 1), (2, 399_000, 500_000)]
    whole = [(0, 0, 3_000_000), (1, 0, 1_000_000), (2, 0, 500_000), (3, 0, 2_000_000_000)]
    windows = np.concatenate([windows, xc.as_windows(rows + whole)])
    for q in (0, 30):
        got = t.window_context(windows, q)
        assert_rows(got, xc.expected_ctx(cols, NT, windows, q))
        totals = xc.class_totals(cols, q)
        assert {f: int(got[-4:][f].sum()) for f in xc.FIELDS} == totals and totals["reads"] > 40_000 and min(totals[f] for f in xc.FIELDS if f != "lowq" or q) > 500
        assert not got[-3].tobytes().strip(b"\0") and not got[-1].tobytes().strip(b"\0")


# ---- 3. classes one by one ------------------------------------------------------------------------------------------------------------
def test_every_class_on_its_own_record():
    """the designed table of tests/test_cpu_context.py, whose rows are also written down by hand there: one single-base window per record"""
    cols, windows = designed_table()
    t, _ = cc.make_ctx(CONTIGS, cols, "host")
    for q in (Q, 0, Q + 1, 256):
        got = t.window_context(windows, q)
        assert_rows(got, xc.expected_ctx(cols, NT, windows, q))
        assert_rows(got, xc.expected_ctx_slow(cols, NT, windows, q))
    got = t.window_context(windows, Q)
    at = {r[1]: got[k] for k, r in enumerate(DESIGNED)}
    assert int(at[250]["secsup"]) == 1 and int(at[250]["dup"]) == 0 and int(at[200]["secsup"]) == 1 and not at[440].tobytes().strip(b"\0")
    assert int(at[520]["clipped"]) == int(at[530]["clipped"]) == int(at[590]["clipped"]) == 1 and int(at[580]["clipped"]) == int(at[540]["clipped"]) == int(at[570]["clipped"]) == 0
    assert (int(at[310]["lowq"]), int(at[320]["lowq"]), int(at[300]["mq0"]), int(at[330]["mapq_sum"])) == (1, 0, 1, 255)
    t.close()


# ---- 4. pile-ups ----------------------------------------------------------------------------------------------------------------------
def test_pile_ups_across_tile_boundaries():
    """100 records in front, 700 at one position (a run across two tile boundaries), 50 behind, and 300 more on the very last base of
    contig c2, unmapped records behind them"""
    rng = np.random.default_rng(41)
    draw = lambda: (xc.FLAGS[int(rng.integers(0, len(xc.FLAGS)))], (0, 5, 20, 60)[int(rng.integers(0, 4))], ("100M", "30S70M", "70M30S", "")[int(rng.integers(0, 4))])
    recs = [(0, 1000 + 7 * k) + draw() for k in range(100)] + [(0, 5000) + draw() for _ in range(700)] + [(0, 5001 + 9 * k) + draw() for k in range(50)]
    recs += [(2, 499_999) + draw() for _ in range(300)] + [(-1, -1, 0x4 | 0x1, 0, "")] * 3
    cols = xc.make_cols(recs)
    rows = [(0, a, b) for a in (0, 4999, 5000, 5001) for b in (4999, 5000, 5001, 5002, 10_000) if b > a]
    rows += [(2, 499_998, 499_999), (2, 499_999, 500_000), (2, 500_000, 500_001), (2, 0, 499_999), (2, 0, 500_000), (2, 499_999, 0xFFFFFFFF)]
    windows = xc.as_windows(rows)
    t, _ = cc.make_ctx(CONTIGS, cols, "host")
    for q in (0, 20):
        got = t.window_context(windows, q)
        exp = xc.expected_ctx(cols, NT, windows, q)
        assert_rows(got, exp)
    pile = exp[rows.index((0, 5000, 5001))]
    assert sum(int(pile[f]) for f in ("reads", "dup", "secsup")) > 500 and not exp[rows.index((0, 4999, 5000))].tobytes().strip(b"\0")
    t.close()


# ---- 5. determinism and independence -------------------------------------------------------------------------------------------------
def test_two_runs_a_permuted_list_and_two_thresholds(large):
    cols, t = large
    rng = np.random.default_rng(19)
    windows = start_windows(cols, rng, n_records=30, n_random=30)
    first = t.window_context(windows, 20)
    again = t.window_context(windows, 20)
    perm = rng.permutation(len(windows))
    moved = t.window_context(windows[perm], 20)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()
    # lowq belongs to the threshold of the call: 50, then 5, then 50 again, each equal to its own definition
    hi, lo = xc.expected_ctx(cols, NT, windows, 50), xc.expected_ctx(cols, NT, windows, 5)
    assert int(hi["lowq"].sum()) > int(lo["lowq"].sum()) * 2 > 0
    assert_rows(t.window_context(windows, 50), hi)
    assert_rows(t.window_context(windows, 5), lo)
    assert_rows(t.window_context(windows, 50), hi)


# ---- 6. table forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "device_side", "exclude_host", "exclude_device", "decode_ctx"])
def test_table_forms(form):
    import torch
    rng = np.random.default_rng(25)
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(300_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
        cols = {k: dcols[k].cpu().numpy().view(dt) for k, dt in (("tid", np.int32), ("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("cigar_off", np.uint32), ("cigar", np.uint32))}
        cols["cigar_off"], cols["cigar"] = cols["cigar_off"][:dcols["n"] + 1], cols["cigar"][:dcols["n_cigar_words"]]
        nt = len(contigs)
        picks = rng.choice(np.flatnonzero(cols["tid"] >= 0), 12, replace=False)
        rows = [(int(cols["tid"][i]), max(0, int(cols["pos"][i]) + d), int(cols["pos"][i]) + 5000) for i in picks for d in (0, 1)] + [(k, 0, int(contigs[k][1])) for k in range(0, nt, 5)]
        windows = xc.as_windows(rows)
    elif form == "decode_ctx":
        ds = cc.designed_tumor(mix=False, n_proper=3000)
        cols = ds.to_soa()
        nt = len(ds.contigs)
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
        windows = start_windows(cols, rng, contigs=cc.CONTIGS)
        windows = windows[windows["tid"] < nt]
    else:
        nt = NT
        cols = xc.random_table(rng, 3000, [(0, 60_000), (2, 30_000)], read_len=100, unmapped=5)
        windows = start_windows(cols, rng)
        t, hold = cc.make_ctx(CONTIGS, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            # bk_exclude_regions: the records that overlap an interval count nowhere; the expected rows come from the kept records
            tid, beg, end = np.asarray([0, 2], np.int32), np.asarray([10_000, 0], np.int32), np.asarray([12_000, 5_000], np.int32)
            removed = t.exclude_regions(tid, beg, end)
            kept = cc.filtered(cols, ~cc.excluded_mask(cols, tid, beg, end))
            assert removed == len(cols["tid"]) - len(kept["tid"]) > 100
            cols = kept
            windows = np.concatenate([windows, xc.as_windows([(0, 9_000, 13_000), (0, 10_000, 11_900), (2, 0, 4_900), (2, 0, 6_000)])])
    for q in (10, 0):
        got = t.window_context(windows, q)
        assert_rows(got, xc.expected_ctx(cols, nt, windows, q))
    assert int(got["reads"].sum()) > 100
    if form.startswith("exclude"):  # (a record that starts inside an interval overlaps it when it has a reference length)
        assert int(got[-3]["reads"]) + int(got[-2]["reads"]) < 10 and int(got[-1]["reads"]) > 0 and int(got[-4]["reads"]) > 0
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


# ---- 7. errors, empty inputs, timing --------------------------------------------------------------------------------------------------
def raw_call(t, windows, mapq_min=0, n=None, null=()):
    C = capi.C
    windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
    out = C.c_void_p()
    rc = t.L.bk_window_context(None if "ctx" in null else t.h, None if "windows" in null else windows.ctypes.data, len(windows) if n is None else n, mapq_min,
                               None if "out" in null else C.byref(out))
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_errors(large):
    cols, t = large
    windows = xc.as_windows([(0, 1000, 2000), (2, 0, 500)])
    assert raw_call(t, windows)[0] == abi.BK_OK
    assert raw_call(t, windows, null=("ctx",))[0] == abi.BK_ERR_ARG
    for null in ("windows", "out"):
        rc, msg = raw_call(t, windows, null=(null,))
        assert rc == abi.BK_ERR_ARG and "null" in msg, (null, msg)
    assert raw_call(t, windows, n=0, null=("windows",))[0] == abi.BK_OK
    none = t.window_context(np.zeros(0, abi.COV_WINDOW), 0)
    assert len(none) == 0 and none.dtype == abi.WINDOW_CTX
    rc, msg = raw_call(t, windows, mapq_min=-1)
    assert rc == abi.BK_ERR_ARG and "mapq_min" in msg, msg
    bad = windows.copy()
    bad[1]["reserved"] = 7
    rc, msg = raw_call(t, bad)
    assert rc == abi.BK_ERR_ARG and "reserved" in msg and "window 1" in msg, msg
    rc, msg = raw_call(t, windows, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 windows" in msg, msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.window_context(windows)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(t.window_context(windows, 0), xc.expected_ctx(cols, NT, windows, 0))  # the context still works
    bare = capi.Context(CONTIGS)
    with pytest.raises(capi.BreakIDError, match="holds no record table") as e:
        bare.window_context(windows)  # no table at all
    assert e.value.code == abi.BK_ERR_ARG
    bare.close()
    # an empty table is no error, and the call needs no bk_isize_stats
    e = capi.Context(CONTIGS)
    e.upload(xc.make_cols([]))
    assert not e.window_context(windows, 5).tobytes().strip(b"\0")
    e.close()
    small = xc.random_table(np.random.default_rng(1), 300, [(0, 20_000)], unmapped=0)
    early = capi.Context(CONTIGS)
    early.upload(small)
    assert_rows(early.window_context(windows, 20), xc.expected_ctx(small, NT, windows, 20))
    early.close()


def test_timing_scopes_and_the_byte_model(large):
    cols, t = large
    windows = xc.as_windows([(0, 299_000, 301_000), (1, 0, 2_000_000), (2, 5, 10)])
    t.timing_enable(True)
    got = t.window_context(windows, QUAL)
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    t.timing_enable(False)
    n = len(cols["tid"])
    tiles = (n + 255) // 256
    model_tiles, model_windows = (2 + 1 + 4 + 4 + 8) * n + 40 * tiles, (16 + 40) * len(windows)
    assert names[-3:] == ["window_context", "window_context_tiles", "window_context_windows"]
    assert tm["window_context"][0] > 0 and tm["window_context"][1] == model_tiles + model_windows == touched["window_context"]
    assert tm["window_context"][0] >= tm["window_context_tiles"][0] > 0 and tm["window_context"][0] >= tm["window_context_windows"][0] > 0
    assert touched["window_context_tiles"] == model_tiles and touched["window_context_windows"] == model_windows
    assert_rows(got, xc.expected_ctx(cols, NT, windows, QUAL))


# ---- 8. command line --------------------------------------------------------------------------------------------------------------------
INFO_LINES = tuple("##INFO=<ID=%s,Number=1,Type=%s," % k for k in (("CXN", "Integer"), ("MQ0F", "Float"), ("MEANMQ", "Float")))


def strip_keys(info):
    return ";".join(f for f in info.split(";") if f.split("=")[0] not in ("CXN", "MQ0F", "MEANMQ"))


def check_twins(prefix, twins, cl, sides, lens, flank, cols, ncols, n_calls):
    """the twins hold the rows of their fusion table in its order, then the definition's columns; returns {call: its columns}"""
    columns = xc.COLUMNS + (["Normal_" + c for c in xc.COLUMNS] if ncols is not None else [])
    seen = {}
    for twin in twins:
        plain = twin.replace("_context", "")
        lines, src = open(prefix + twin).read().split("\n"), open(prefix + plain).read().split("\n")
        assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(columns)
        calls = written_calls(cl, prefix + plain)
        assert len(calls) == len(lines) - 2 and len(calls) == n_calls[plain]
        by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
        for line, s in zip(lines[1:-1], src[1:-1]):
            f = line.split("\t")
            i = by_key[(f[1], f[2])]
            pair, w = xc.expected_call_rows(cl[i], sides[i][0], sides[i][1], flank, lens, cols, QUAL)
            exp = xc.expected_columns(pair)
            if ncols is not None:
                exp = exp + xc.expected_columns(xc.expected_call_rows(cl[i], sides[i][0], sides[i][1], flank, lens, ncols, QUAL)[0])
            assert line == s + "\t" + "\t".join(exp), (line, exp)
            seen[i] = (exp, pair, w)
    return seen


@pytest.mark.parametrize("variant", ["plain", "everything"])
def test_cli_context(cov_run, variant):  # noqa: F811
    run = cov_run
    tmp, cl, sides = run["tmp"], run["cl"], run["sides"]
    lens = np.asarray([l for _, l in cc.CONTIGS], np.uint32)
    flank = 500 if variant == "plain" else 700
    with_normal = variant == "everything"
    panel = os.path.join(tmp, "panel.bedpe")
    open(panel, "w").write("chr1\t299000\t301000\tchr2\t699000\t701000\tX\t5\t+\t-\n")
    extra = [] if variant == "plain" else ["-vcf", "-normal", run["nbam"], "-genotype", "-coverage", "-known", panel, "-bedpe"]
    base = [BIN, "-i", run["bam"], "-n", run["nib"], "-all", "-fast"] + extra
    a, b = os.path.join(tmp, "cxa_" + variant), os.path.join(tmp, "cxb_" + variant)
    r = subprocess.run(base + ["-o", a], env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out_a = r.stdout
    r = subprocess.run(base + ["-o", b, "-context"] + ([] if variant == "plain" else ["-ctxflank", "700"]), env=run["env"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # 1. the files: the twins are new, the VCF and the two logs change, every other file is byte-identical
    twins = ["_fusion_all_context.txt", "_fusion_context.txt"]
    pa, pb = os.path.basename(a), os.path.basename(b)
    fa = sorted(f[len(pa):] for f in os.listdir(tmp) if f.startswith(pa + "_"))
    fb = sorted(f[len(pb):] for f in os.listdir(tmp) if f.startswith(pb + "_"))
    assert fb == sorted(fa + twins), (fa, fb)
    changed = {"_params.txt", "_performance.txt", "_fusion.vcf"}
    for suffix in fa:
        if suffix not in changed:  # (the name column of a BEDPE line is the prefix's base name)
            assert open(a + suffix, "rb").read().replace(pa.encode(), pb.encode()) == open(b + suffix, "rb").read(), suffix
    if with_normal:
        assert {"_fusion_normal.txt", "_fusion_genotype.txt", "_fusion.vcf", "_fusion_coverage.txt", "_fusion_known.txt", "_fusion.bedpe"} <= set(fa)
    ta, tb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
    assert tb == ta.replace("out_file\t" + a, "out_file\t" + b) + "context_flank\t%d\n" % flank, (ta, tb)
    # 2. the twins, and the stdout line from their rows
    seen = check_twins(b, twins, cl, sides, lens, flank, run["cols"], run["ncols"] if with_normal else None, {"_fusion.txt": 1, "_fusion_all.txt": 4})
    reads = sum(int(p[s]["reads"]) for _, p, _ in seen.values() for s in (0, 1))
    mq0 = sum(int(p[s]["mq0"]) for _, p, _ in seen.values() for s in (0, 1))
    line = "context: 4 calls, %d reads in their windows, %d of them with mapping quality 0" % (reads, mq0)
    quiet = lambda text: [l for l in text.split("\n") if "costs time" not in l]
    assert reads > 500 and line in r.stdout.split("\n") and [l for l in quiet(r.stdout) if l != line] == quiet(out_a.replace(a, b))
    # the split reads at a breakpoint are clipped, and their partners are secondary alignments
    assert all(int(p[0]["clipped"]) + int(p[1]["clipped"]) > 0 and int(p[0]["secsup"]) + int(p[1]["secsup"]) > 0 for _, p, _ in seen.values())
    # 3. the VCF: CXN, MQ0F and MEANMQ of the breakend's own side last in INFO, their header lines last among the INFO lines
    if variant == "plain":
        return
    va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
    assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in INFO_LINES)
    assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
    info = [k for k, l in enumerate(vb) if l.startswith("##INFO")]
    assert [vb[k].startswith(i) for k, i in zip(info[-3:], INFO_LINES)] == [True] * 3
    body_a = [l for l in va if l and not l.startswith("#")]
    body_b = [l for l in vb if l and not l.startswith("#")]
    assert len(body_a) == len(body_b) == 8
    for la, lb in zip(body_a, body_b):
        x, y = la.split("\t"), lb.split("\t")
        i = int(y[2][2:].split("_")[0])
        side = int(y[2].split("_")[1]) - 1
        f = seen[i][0][9 * side:9 * side + 9]
        tail = ";CXN=" + f[0] + (";MQ0F=%s;MEANMQ=%s" % (f[2], f[1]) if f[0] != "0" else "")
        assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + tail and strip_keys(y[7]) == x[7], lb


SHORT = [("chr1", 2_000_000), ("chr2", 2_000_000), ("chr3", 2_000_000), ("chr4", 400_000)]
SHORT_LOCI = [("S", 0, 300_000, "L", 3, 200_000, "R"), ("E", 3, 399_500, "L", 1, 700, "R")]


def test_cli_flank_of_one_base_and_flanks_beyond_the_contig():
    """-ctxflank 1, and the largest flank (1 000 000) around calls on a contig of 400 000 bases, 500 bases from its end and 700 from
    another contig's start: every window is clamped, some to nothing"""
    rng = np.random.default_rng(6)
    ds = cc.designed_tumor(mix=False, contigs=SHORT, loci=SHORT_LOCI, n_proper=0)
    for i in range(3000):
        tid = int(rng.integers(0, 4))
        ds.recs += synth._proper_pair(rng, i, tid, 1000, SHORT[tid][1] - 1000, 100, 350, 40)
    ds.sort()
    cols = ds.to_soa()
    lens = np.asarray([l for _, l in SHORT], np.uint32)
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.run(qual=QUAL, fast=True)
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    sides = [capi.junction_sides(j)[:2] for j in t.junctions()]
    t.close()
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, bam)
        side = synth.write_side_files(ds, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        for flank in (1, 1_000_000):
            prefix = os.path.join(tmp, "f%d" % flank)
            r = subprocess.run([BIN, "-i", bam, "-n", side["nib"], "-all", "-fast", "-o", prefix, "-context", "-ctxflank", str(flank)], env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            seen = check_twins(prefix, ["_fusion_all_context.txt"], cl, sides, lens, flank, cols, None, {"_fusion_all.txt": 2})
            assert open(prefix + "_params.txt").read().endswith("context_flank\t%d\n" % flank)
            if flank == 1:
                assert all(int(w["end"]) - int(w["beg"]) == 1 for _, _, w4 in seen.values() for w in w4)
            else:
                spans = sorted((int(w["tid"]), int(w["beg"]), int(w["end"])) for _, _, w4 in seen.values() for w in w4 if int(w["tid"]) == 3)
                assert [s[1] for s in spans] == [0, 0, 199_999, 399_500] and [s[2] for s in spans] == [199_999, 399_500, 400_000, 400_000], spans
                assert sum(int(p[s]["reads"]) for _, p, _ in seen.values() for s in (0, 1)) > 1000


def test_cli_limits_and_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        for args, word in ((["-ctxflank", "100"], "-ctxflank needs -context."), (["-context", "-gpus", "2"], "-context cannot be combined with -gpus."),
                           (["-gpus", "2", "-context", "-ctxflank", "0"], "-context cannot be combined with -gpus."),
                           (["-context", "-ctxflank", "0"], "-ctxflank must be a number from 1 to 1000000."),
                           (["-context", "-ctxflank", "1000001"], "-ctxflank must be a number from 1 to 1000000."),
                           (["-context", "-ctxflank", "5", "-covflank", "3"], "-covflank needs -coverage.")):
            r = subprocess.run(base + args, env=env, capture_output=True, text=True)
            assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-2000:])
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-context", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1 and "context: 0 calls, 0 reads in their windows, 0 of them with mapping quality 0" in r.stdout.split("\n")
        for twin in ("_fusion_context.txt", "_fusion_all_context.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(xc.COLUMNS) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("vcf\t1\ncontext_flank\t500\n")

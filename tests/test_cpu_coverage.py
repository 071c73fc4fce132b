"""Window coverage without a GPU: the row layouts and the exports, the numpy definition (tests/coveragecases.py) against a plain double
loop, the window rule of `bk_call_windows` at its edges (the library's host function against its statement in Python), the formatting
of the twin columns, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import coveragecases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.COV_WINDOW.itemsize == 16 and abi.WINDOW_COV.itemsize == 16
    assert list(abi.COV_WINDOW.names) == ["tid", "beg", "end", "reserved"] and list(abi.WINDOW_COV.names) == ["bases", "reads", "reserved"]
    assert [abi.COV_WINDOW.fields[f][1] for f in abi.COV_WINDOW.names] == [0, 4, 8, 12]
    assert [abi.WINDOW_COV.fields[f][1] for f in abi.WINDOW_COV.names] == [0, 8, 12]
    assert abi.COV_WINDOW.fields["tid"][0] == np.dtype("<i4") and abi.WINDOW_COV.fields["bases"][0] == np.dtype("<u8")
    for name in ("bk_window_coverage", "bk_call_windows"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert hasattr(capi.Context, "window_coverage") and hasattr(capi, "call_windows")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_cov_window { int32_t tid; uint32_t beg, end; uint32_t reserved; };" in header
    assert "struct bk_window_cov { uint64_t bases; uint32_t reads; uint32_t reserved; };" in header
    assert "int bk_window_coverage(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_cov **out);" in header
    assert "int bk_call_windows(const bk_cluster *c, int right1, int right2, uint32_t flank, const uint32_t *target_len, struct bk_cov_window out[5]);" in header
    assert "cal_mean_depth" in header and "[a + 1, b]" in header


def test_definition_equals_a_double_loop(monkeypatch):
    """60 seeded small tables: three contigs (one without records), barred flags, clip-only CIGARs, deletions, unmapped records, windows
    on and around record edges, beyond the contig, empty, reversed and on contigs that do not exist; both forms of the difference array"""
    rng = np.random.default_rng(21)
    total = 0
    for case in range(60):
        n = int(rng.integers(0, 60))
        cols = vc.random_table(rng, n, [(0, 600), (2, 900)], read_len=int(rng.integers(5, 80)), unmapped=case % 3)
        rows = [(-1, 0, 100), (3, 0, 100), (1, 0, 900), (0, 50, 50), (0, 60, 50), (0, 0, 1 << 31), (2, 0, 0xFFFFFFFF)]
        for i in range(len(cols["tid"])):
            t, p = int(cols["tid"][i]), int(cols["pos"][i])
            if t >= 0 and rng.random() < 0.3:
                e = p + int(vc.eligible_len(cols, 0)[i])
                rows += [(t, max(0, p + d), max(0, e + d2)) for d in (-1, 0, 1) for d2 in (-1, 0, 1)]
        for _ in range(20):
            a = int(rng.integers(0, 1000))
            rows.append((int(rng.integers(0, 3)), a, a + int(rng.integers(0, 400))))
        windows = vc.as_windows(rows)
        for q in (0, 20, 61):
            slow = vc.brute_force(cols, 3, windows, q)
            fast = vc.expected_cov(cols, 3, windows, q)
            assert fast.tobytes() == slow.tobytes(), (case, q)
            monkeypatch.setattr(vc, "DENSE_MAX", 0)  # the form for contigs too long for one entry per base
            sparse = vc.expected_cov(cols, 3, windows, q)
            monkeypatch.undo()
            assert sparse.tobytes() == slow.tobytes(), (case, q)
            total += int(slow["bases"].sum())
        assert not fast[:5].tobytes().strip(b"\0")
    assert total > 100_000


def test_definition_on_designed_records():
    # one 100M read at 1000, one 50M1000N50M at 1100 (span 1100), a duplicate, a mapq-5 read and a clip-only read on top of the first
    cols = vc.make_cols([(0, 1000, 0, 60, "100M"), (0, 1100, 0, 60, "50M1000N50M"), (0, 1000, 0x400, 60, "100M"), (0, 1000, 0, 5, "100M"), (0, 1000, 0, 60, "100S"),
                         (1, 0, 0, 60, "30S70M")])
    w = vc.as_windows([(0, 1000, 1100), (0, 999, 1101), (0, 1050, 1060), (0, 1100, 2200), (0, 1150, 2150), (0, 0, 5000), (0, 1099, 1100), (0, 1100, 1101), (1, 0, 70), (1, 70, 80)])
    q20 = vc.expected_cov(cols, 2, w, 20)
    assert [(int(r["bases"]), int(r["reads"])) for r in q20] == [(100, 1), (101, 2), (10, 1), (1100, 1), (1000, 1), (1200, 2), (1, 1), (1, 1), (70, 1), (0, 0)]
    q0 = vc.expected_cov(cols, 2, w, 0)
    assert [(int(r["bases"]), int(r["reads"])) for r in q0[:3]] == [(200, 2), (201, 3), (20, 2)]


LENS = np.asarray([10_000, 500, 10_000], np.uint32)


def cluster(t1, e1, t2, e2):
    c = np.zeros(1, abi.CLUSTER)[0]
    c["p1_tid"], c["p1_exact"], c["p2_tid"], c["p2_exact"], c["flags"] = t1, e1, t2, e2, 3
    return c


def rows(w):
    return [(int(x["tid"]), int(x["beg"]), int(x["end"]), int(x["reserved"])) for x in w]


def test_window_rule_at_its_edges():
    cases = []
    for r1 in (0, 1):
        for r2 in (0, 1):
            for flank in (1, 100, 1000, 20_000):
                cases += [(cluster(0, 1, 0, 10_000), r1, r2, flank),      # position 1 and the contig's last base
                          (cluster(0, 10_000, 0, 1), r1, r2, flank),      # ... in the other order
                          (cluster(0, 5000, 0, 5000), r1, r2, flank),     # equal positions: equal cuts when the directions agree
                          (cluster(0, 5000, 0, 5001), r1, r2, flank),     # ... or one apart
                          (cluster(1, 250, 1, 300), r1, r2, flank),       # flank longer than the contig
                          (cluster(0, 700, 2, 9000), r1, r2, flank),      # different contigs
                          (cluster(-1, 700, 2, 9000), r1, r2, flank), (cluster(0, 700, -1, 9000), r1, r2, flank), (cluster(-1, 5, -1, 5), r1, r2, flank)]
    for c, r1, r2, flank in cases:
        got = capi.call_windows(c, r1, r2, flank, LENS)
        exp = vc.call_windows(c, r1, r2, flank, LENS)
        assert got.tobytes() == exp.tobytes(), (c, r1, r2, flank, rows(got), rows(exp))
    # by hand.  A LEFT side at position 1: its cut is 1, the breakpoint base (0-based 0) is the left window
    w = rows(vc.call_windows(cluster(0, 1, 0, 10_000), 0, 1, 100, LENS))
    assert w == [(0, 0, 1, 0), (0, 1, 101, 0), (0, 9899, 9999, 0), (0, 9999, 10_000, 0), (0, 1, 9999, 0)]
    # a RIGHT side at position 1: cut 0, nothing to its left; a LEFT side at the last base: cut = the length, nothing to its right
    w = rows(vc.call_windows(cluster(0, 1, 0, 10_000), 1, 0, 100, LENS))
    assert w == [(0, 0, 0, 0), (0, 0, 100, 0), (0, 9900, 10_000, 0), (0, 0, 0, 0), (0, 0, 10_000, 0)]
    # either order gives the same span; equal cuts give an empty one
    assert rows(vc.call_windows(cluster(0, 10_000, 0, 1), 0, 1, 100, LENS))[4] == (0, 0, 10_000, 0)
    assert rows(vc.call_windows(cluster(0, 5000, 0, 5000), 0, 0, 100, LENS))[4] == (0, 0, 0, 0)
    assert rows(vc.call_windows(cluster(0, 5000, 0, 5000), 0, 1, 100, LENS))[4] == (0, 4999, 5000, 0)
    # a flank longer than the contig is the contig's part on that side
    assert rows(vc.call_windows(cluster(1, 250, 1, 300), 0, 0, 1000, LENS)) == [(1, 0, 250, 0), (1, 250, 500, 0), (1, 0, 300, 0), (1, 300, 500, 0), (1, 250, 300, 0)]
    # different contigs and negative tids: no span; the side of a negative tid is empty
    assert rows(vc.call_windows(cluster(0, 700, 2, 9000), 0, 1, 100, LENS)) == [(0, 600, 700, 0), (0, 700, 800, 0), (2, 8899, 8999, 0), (2, 8999, 9099, 0), (-1, 0, 0, 0)]
    assert rows(vc.call_windows(cluster(-1, 700, 2, 9000), 0, 1, 100, LENS))[:2] == [(-1, 0, 0, 0), (-1, 0, 0, 0)]
    assert rows(vc.call_windows(cluster(-1, 5, -1, 5), 0, 1, 100, LENS))[4] == (-1, 0, 0, 0)
    # errors
    with pytest.raises(capi.BreakIDError) as e:
        capi.call_windows(cluster(0, 700, 2, 9000), 0, 1, 0, LENS)
    assert e.value.code == abi.BK_ERR_ARG
    C = capi.C
    c = np.zeros(1, abi.CLUSTER)
    out = np.zeros(5, abi.COV_WINDOW)
    L = capi.lib()
    assert L.bk_call_windows(None, 0, 1, 100, LENS.ctypes.data, out.ctypes.data) == abi.BK_ERR_ARG
    assert L.bk_call_windows(c.ctypes.data, 0, 1, 100, None, out.ctypes.data) == abi.BK_ERR_ARG
    assert L.bk_call_windows(c.ctypes.data, 0, 1, 100, LENS.ctypes.data, None) == abi.BK_ERR_ARG
    assert C.sizeof(C.c_void_p) == 8


def cov_rows(values):
    c = np.zeros(len(values), abi.WINDOW_COV)
    c["bases"] = values
    return c


def test_formatting_of_dots_and_of_the_ratio():
    c = cluster(0, 5000, 0, 7000)
    w = np.zeros(7, abi.COV_WINDOW)
    w[:5] = vc.call_windows(c, 0, 1, 1000, LENS)
    w[5]["end"] = w[6]["end"] = 10_000
    cuts = vc.call_cuts(c, 0, 1)
    assert cuts == (5000, 6999)
    # flanks at depth 30 and 10 (mean 20), the span at 10: 0.5
    f = vc.call_fields(w, cov_rows([30_000, 11_111, 9_999, 10_000, 19_990, 123_456, 123_456]), cuts)
    assert f == ["30.00", "11.11", "10.00", "10.00", "10.00", "0.500", "12.35", "12.35"]
    # the sides in the other order: the outer flanks are still the lowest left and the highest right window
    c2 = cluster(0, 7000, 0, 5000)
    w2 = np.zeros(7, abi.COV_WINDOW)
    w2[:5] = vc.call_windows(c2, 1, 0, 1000, LENS)
    f2 = vc.call_fields(w2, cov_rows([9_999, 10_000, 30_000, 11_111, 19_990, 0, 0]), vc.call_cuts(c2, 1, 0))
    assert f2[:6] == ["10.00", "10.00", "30.00", "11.11", "10.00", "0.500"] and f2[6:] == [".", "."]
    # flanks without a base: no ratio, but means of 0.00
    assert vc.call_fields(w, cov_rows([0, 5, 5, 0, 1999, 0, 0]), cuts)[:6] == ["0.00", "0.01", "0.01", "0.00", "1.00", "."]
    # an empty span, an empty flank, different contigs
    eq = cluster(0, 5000, 0, 5000)
    we = np.zeros(7, abi.COV_WINDOW)
    we[:5] = vc.call_windows(eq, 0, 0, 1000, LENS)
    assert vc.call_fields(we, cov_rows([1000] * 7), (5000, 5000))[4:6] == [".", "."]
    edge = cluster(0, 1, 0, 3000)
    wd = np.zeros(7, abi.COV_WINDOW)
    wd[:5] = vc.call_windows(edge, 1, 1, 1000, LENS)
    fd = vc.call_fields(wd, cov_rows([0, 2000, 1000, 1000, 2999, 0, 0]), vc.call_cuts(edge, 1, 1))
    assert fd[:6] == [".", "2.00", "1.00", "1.00", "1.00", "."]
    x = cluster(0, 700, 2, 9000)
    wx = np.zeros(7, abi.COV_WINDOW)
    wx[:5] = vc.call_windows(x, 0, 1, 100, LENS)
    assert vc.call_fields(wx, cov_rows([100] * 7), vc.call_cuts(x, 0, 1))[:6] == ["1.00", "1.00", "1.00", "1.00", ".", "."]
    # rounding is printf's, on the quotient of two doubles
    one = vc.as_windows([(0, 0, 3)])
    assert vc.mean_text(one[0], cov_rows([2])[0]) == "0.67" and vc.mean_text(one[0], cov_rows([1])[0]) == "0.33"


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_coverage(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-coverage"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -coverage needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-coverage", "-covflank", "500", "-all", "-fast", "-similar"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -similar needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    r = subprocess.run(base + ["-coverage", "-covflank", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -coverage needs the GPU library" in r.stderr, r.stderr[-2000:]  # (the library row stands before the range)
    # the usage refusals stand behind the help text, in the order of the table
    for args, word in ((["-covflank", "100"], "Error: -covflank needs -coverage."), (["-coverage", "-gpus", "2"], "Error: -coverage cannot be combined with -gpus."),
                       (["-covflank", "100", "-gpus", "2"], "Error: -covflank needs -coverage."), (["-coverage", "-covflank", "0", "-gpus", "2"], "Error: -coverage cannot be combined with -gpus."),
                       (["-covflank", "100", "-simflank", "9"], "Error: -simflank needs -similar.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-coverage" in r.stderr and "-covflank" in r.stderr and "Error" not in r.stderr

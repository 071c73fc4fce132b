"""CIGAR gaps without a GPU: the row layout, the exports and the header's text; the two statements of the definition in
tests/gapcases.py on designed inputs and on a few hundred seeded small tables that reach every operation, every kind of dropped record,
chains, ties and shared reads; the hand example of the header; how the command line prints a row; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import gapcases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
CONTIGS = [("chr1", 1_000_000), ("chr2", 5_000)]
TLEN = [l for _, l in CONTIGS]


def test_row_layout_and_exports():
    d = abi.CIGAR_GAP
    assert d.itemsize == 64 and list(d.names) == list(gc.FIELDS)
    assert [d.fields[f][1] for f in d.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56]
    assert d.fields["tid"][0] == np.dtype("<i4") and d.fields["start"][0] == np.dtype("<u4") and d.fields["mapq_sum"][0] == np.dtype("<u8")
    assert abi.GAP_MAX_TOL == gc.MAX_TOL == 100 and abi.GAP_MAX_LEN == gc.MAX_LEN == 1_000_000 and (abi.GAP_DEL, abi.GAP_INS) == (0, 1)
    for name in ("bk_cigar_gaps", "bk_cigar_gap_counts"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert hasattr(capi.Context, "cigar_gaps") and hasattr(capi.Context, "cigar_gap_counts")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert ("int bk_cigar_gaps(bk_ctx *records, int mapq_min, uint32_t min_len, uint32_t anchor, uint32_t tol, uint32_t min_reads, const struct bk_cigar_gap **out, "
            "uint64_t *count);") in header
    assert "int bk_cigar_gap_counts(bk_ctx *records, uint64_t out[8]);" in header and "#define BK_GAP_MAX_TOL 100u\n" in header
    for line in ("  int32_t tid; uint32_t start; uint32_t len; uint32_t kind;", "  uint32_t n_reads, n_rows, n_exact;", "  uint32_t top_reads;", "  uint32_t lo_start, hi_start, lo_len, hi_len;",
                 "  uint32_t n_fwd, n_rev;", "  uint64_t mapq_sum;"):
        assert line in header, line
    assert "scope `cigar_gaps`" in header and "Nothing is capped" in header and "bridges their starts" in header and "No atomic anywhere" in header
    assert "The host reads a count four times" in header
    # the shim of the CPU build does not have the call
    shim = open(os.path.join(ROOT, "oracle", "Makefile")).read() + "".join(open(os.path.join(ROOT, "oracle", f)).read() for f in os.listdir(os.path.join(ROOT, "oracle")) if f.endswith((".cc", ".h")))
    assert "bk_cigar_gaps" not in shim


def hand_example():
    recs = [gc.read(q, 0, 999, "70M45D80M") for q in "abc"]
    recs += [gc.read("d", 0, 1000, "70M46D79M", flag=0x1 | 0x2 | 0x40 | 0x10, mapq=40), gc.read("d", 0, 1039, "30M45D120M", flag=0x1 | 0x2 | 0x80)]
    recs += [gc.read("e", 0, 1059, "10M30I110M", mapq=30), gc.read("f", 0, 1060, "9M45D141M"), gc.read("g", 0, 999, "70M45N80M")]
    return gc.dataset(CONTIGS[:1], recs).to_soa()


def test_hand_example():
    """the header's: one contig of 1 000 000 bases, mapq_min 20, min_len 20, anchor 10, tol 2, min_reads 1"""
    cols = hand_example()
    rows, counts = gc.both(cols, TLEN[:1])
    assert counts == dict(records=8, eligible=8, events=6, beyond=0, exact=3, loci=2, calls=2, written=2)
    assert [tuple(int(v) for v in r) for r in rows] == [(0, 1069, 45, 0, 4, 5, 2, 4, 1069, 1070, 45, 46, 4, 1, 280), (0, 1069, 30, 1, 1, 1, 1, 1, 1069, 1069, 30, 30, 1, 0, 30)]
    why = [gc.why_dropped(cols, i, TLEN[:1], 20, 20, 10) for i in range(8)]
    assert sorted(w for w in why if w) == ["anchor", "short"] and why.count(None) == 6
    assert gc.both(cols, TLEN[:1], tol=0)[1]["calls"] == 3
    only, counts = gc.both(cols, TLEN[:1], min_reads=2)
    assert len(only) == 1 and only[0].tobytes() == rows[0].tobytes() and counts["calls"] == 2 and counts["written"] == 1
    assert gc.both(cols, TLEN[:1], mapq_min=61)[1]["eligible"] == 0
    assert len(gc.both(cols, TLEN[:1], min_len=46)[0]) == 1 and len(gc.both(cols, TLEN[:1], anchor=9)[0]) == 2


def test_designed_inputs():
    """what the GPU tests design, small: the walk over every operation, the bounds of min_len and anchor, beyond, the bridge"""
    def one(cigar, pos=1000, tid=0):
        return gc.both(gc.dataset(CONTIGS, [gc.read("q", tid, pos, cigar)]).to_soa(), TLEN)
    rows, _ = one("5H5S12M3I2P4=6X30N20D15M5S")
    assert [(int(r["start"]), int(r["len"]), int(r["kind"])) for r in rows] == [(1000 + 12 + 4 + 6 + 30, 20, 0)]
    assert len(one("30M20D30M")[0]) == 1 and len(one("30M19D30M")[0]) == 0
    assert len(one("10M20D30M")[0]) == 1 and len(one("9M20D30M")[0]) == 0 and len(one("30M20D10M")[0]) == 1 and len(one("30M20D9M")[0]) == 0
    assert len(one("5=5X20I10=")[0]) == 1 and len(one("5M3I5M40N20D10M")[0]) == 1 and len(one("20D30M")[0]) == 0 and len(one("30M20I")[0]) == 0
    assert len(one("5S20D30M")[0]) == 0 and len(one("5H30M20D5M5S")[0]) == 0
    rows, counts = one("30M25D25I30M", pos=0)
    assert [(int(r["kind"]), int(r["start"]), int(r["len"])) for r in rows] == [(0, 30, 25), (1, 55, 25)] and counts["events"] == 2
    # chr2 has 5000 bases: a deletion whose right end is 5001 is beyond, 5000 is kept; an insertion behind the last base is beyond
    assert one("30M20D30M", pos=4980 - 30, tid=1)[1]["beyond"] == 1 and len(one("30M20D30M", pos=4979 - 30, tid=1)[0]) == 1
    assert one("30M20I30M", pos=5000 - 30, tid=1)[1]["beyond"] == 1 and len(one("30M20I30M", pos=4999 - 30, tid=1)[0]) == 1
    # the bridge: starts 2 tol apart with equal len are one call when a third length stands between them
    reads = [gc.read("a", 0, 1000, "30M40D30M"), gc.read("b", 0, 1004, "30M40D30M")]
    assert gc.both(gc.dataset(CONTIGS, reads).to_soa(), TLEN)[1]["calls"] == 2
    rows, counts = gc.both(gc.dataset(CONTIGS, reads + [gc.read("c", 0, 1002, "30M41D30M")]).to_soa(), TLEN)
    assert counts["loci"] == 1 and counts["calls"] == 1 and (int(rows[0]["lo_start"]), int(rows[0]["hi_start"]), int(rows[0]["n_exact"])) == (1030, 1034, 3)
    rows, counts = gc.both(gc.dataset(CONTIGS, reads + [gc.read("c", 0, 1002, "30M60D30M")]).to_soa(), TLEN)
    assert counts["loci"] == 1 and counts["calls"] == 2 and int(rows[0]["n_exact"]) == 2  # one locus; the bridge's own length is a call of its own


def test_the_two_statements_agree_and_reach_every_shape():
    """300 seeded tables of up to 60 records on three short contigs under tol 0, 2 and 25"""
    rng = np.random.default_rng(30)
    tlen = [400, 90, 2000]
    seen = dict(unmapped=0, flag=0, mapq=0, no_cigar=0, short=0, anchor=0, beyond=0, kept=0, multi_event=0, multi_exact=0, shared_reads=0, tie=0, ins=0, dele=0, below_min=0,
                two_calls_one_locus=0)
    for case in range(300):
        cols = gc.random_cols(rng, int(rng.integers(1, 60)), tlen)
        for i in range(len(cols["tid"])):
            why = gc.why_dropped(cols, i, tlen, 20, 20, 10)
            seen[why or "kept"] += 1
            seen["multi_event"] += why is None and len(gc.walk(cols, i, tlen, 20, 10)[0]) > 1
        for tol in (0, 2, 25):
            info = {}
            a, counts = gc.both(cols, tlen, tol=tol, info=info)
            assert np.all(a["n_reads"] <= a["n_rows"]) and np.all(a["top_reads"] <= a["n_reads"]) and np.all(a["n_fwd"] + a["n_rev"] == a["n_rows"]) and np.all(a["n_exact"] <= a["n_rows"])
            assert np.all(a["lo_start"] <= a["start"]) and np.all(a["start"] <= a["hi_start"]) and np.all(a["lo_len"] <= a["len"]) and np.all(a["len"] <= a["hi_len"])
            assert int(a["n_rows"].sum()) == counts["events"] and int(a["n_exact"].sum()) == counts["exact"] and len(a) == counts["calls"] >= counts["loci"]
            if tol == 0:
                assert np.all(a["n_exact"] == 1) and counts["calls"] == counts["exact"]
            seen["multi_exact"] += int((a["n_exact"] > 1).sum())
            seen["shared_reads"] += int((a["n_reads"] < a["n_rows"]).sum())
            seen["tie"] += int(((a["n_exact"] > 1) & (a["top_reads"] * a["n_exact"] == a["n_reads"])).sum())
            seen["ins"] += int((a["kind"] == 1).sum())
            seen["dele"] += int((a["kind"] == 0).sum())
            seen["two_calls_one_locus"] += counts["calls"] > counts["loci"]
            b, cb = gc.both(cols, tlen, tol=tol, min_reads=2)
            seen["below_min"] += len(a) - len(b)
            assert b.tobytes() == a[a["n_reads"] >= 2].tobytes() and cb["calls"] == counts["calls"] and cb["written"] == len(b)
    assert min(seen.values()) >= 10, seen


def test_formatters():
    r = np.zeros((), abi.CIGAR_GAP)
    r["tid"], r["start"], r["len"], r["kind"], r["n_reads"], r["n_rows"], r["n_exact"], r["top_reads"] = 0, 1069, 45, 0, 4, 5, 2, 4
    r["lo_start"], r["hi_start"], r["lo_len"], r["hi_len"], r["n_fwd"], r["n_rev"], r["mapq_sum"] = 1069, 1070, 45, 46, 4, 1, 281
    assert gc.row_fields(7, r, ["chrA"], 30, 31, "G1") == ["gp7", "chrA", "1069", "1115", "deletion", "45", "4", "5", "2", "4", "4", "1", "56.2", "1069-1070", "45-46", "30", "31", "G1",
                                                         "intergenic"]
    assert gc.bedpe_line(7, r, ["chrA"], "run") == "chrA\t1068\t1069\tchrA\t1114\t1115\trun\t4\t+\t-\tgp7\tdeletion\t0\t4"
    r["kind"] = 1
    assert gc.row_fields(0, r, ["chrA"], 1, 2)[:6] == ["gp0", "chrA", "1069", "1070", "insertion", "45"] and len(gc.COLUMNS) == 19
    assert gc.stdout_line(dict(eligible=8, events=6, beyond=1, exact=3, calls=2, written=1)) == "gaps: 8 records eligible, 6 events, 1 beyond a contig's end, 3 exact, 2 calls, 1 written"


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_gaps(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for args in (["-gaps"], ["-gaps", "-mingap", "30", "-gapanchor", "5", "-gaptol", "0", "-gapsupport", "2", "-all", "-fast"], ["-gaps", "-mingap", "1000000", "-gaptol", "100"]):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: -gaps needs the GPU library" in r.stderr and "Usage" not in r.stderr, (args, r.stderr[-2000:])
    need = "Error: -mingap, -gapanchor, -gaptol and -gapsupport need -gaps."
    for args, word in ((["-mingap", "5"], need), (["-gapanchor", "5"], need), (["-gaptol", "1"], need), (["-gapsupport", "1"], need),
                       (["-gaps", "-gpus", "2"], "Error: -gaps cannot be combined with -gpus."),
                       (["-gaps", "-mingap", "0"], "Error: -mingap must be a number from 1 to 1000000."), (["-gaps", "-mingap", "1000001"], "Error: -mingap must be a number from 1 to 1000000."),
                       (["-gaps", "-gapanchor", "0"], "Error: -gapanchor must be a number from 1 to 2147483647."),
                       (["-gaps", "-gaptol", "101"], "Error: -gaptol must be a number from 0 to 100."), (["-gaps", "-gaptol", "-1"], "Error: -gaptol must be a number from 0 to 100."),
                       (["-gaps", "-gapsupport", "0"], "Error: -gapsupport must be a number from 1 to 1000000."),
                       (["-gaps", "-gapsupport", "1000001"], "Error: -gapsupport must be a number from 1 to 1000000."),
                       (["-gaps", "-jtol", "1"], "Error: -jsupport and -jtol need -junctions.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert all(w in r.stderr for w in ("-gaps ", "-mingap", "-gapanchor", "-gaptol", "-gapsupport")) and "Error" not in r.stderr

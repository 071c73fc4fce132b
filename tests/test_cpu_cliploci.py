"""Soft-clip loci without a GPU: the row layout, the exports and the header's text; the hand example of the header; the two statements
of the definition in tests/cliplocicases.py on designed inputs and on a few hundred seeded small tables that reach every kind of dropped
record, hard clips in front of soft clips, both clips on one record, chains, ties of the representative and of the partner, shared
reads, duplicated / blunt / lost offsets and the edges of pair_dist; how the command line prints a row; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import cliplocicases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
CONTIGS = [("chr1", 1_000_000), ("chr2", 5_000)]
TLEN = [l for _, l in CONTIGS]
NONE = lc.NONE
FIELDS = ("tid", "pos", "dir", "flags", "n_reads", "n_rows", "n_exact", "top_reads", "lo_pos", "hi_pos", "n_fwd", "n_rev", "max_clip", "n_orphan", "clip_sum", "mapq_sum", "n_improper",
          "claim", "mate", "mate_pos", "mate_reads", "mate_off")


def test_row_layout_and_exports():
    d = abi.CLIP_LOCUS
    assert d.itemsize == 96 and tuple(d.names) == FIELDS
    assert [d.fields[f][1] for f in d.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64, 72, 76, 80, 84, 88, 92]
    assert d.fields["tid"][0] == np.dtype("<i4") and d.fields["mate_off"][0] == np.dtype("<i4") and d.fields["clip_sum"][0] == d.fields["mapq_sum"][0] == np.dtype("<u8")
    assert abi.CLIPLOCI_MAX_TOL == lc.MAX_TOL == 100 and abi.CLIPLOCI_MAX_PAIR == lc.MAX_PAIR == 100_000
    for name in ("bk_clip_loci", "bk_clip_locus_counts"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert hasattr(capi.Context, "clip_loci") and hasattr(capi.Context, "clip_locus_counts")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert ("int bk_clip_loci(bk_ctx *records, bk_ctx *calls, int mapq_min, int min_clip, uint32_t tol, uint32_t pair_dist, uint32_t min_reads, const struct bk_clip_locus **out,\n"
            "                 uint64_t *count);") in header
    assert "int bk_clip_locus_counts(bk_ctx *records, uint64_t out[8]);" in header
    assert "#define BK_CLIPLOCI_MAX_TOL 100u\n" in header and "#define BK_CLIPLOCI_MAX_PAIR 100000u\n" in header
    for line in ("  int32_t tid; uint32_t pos; uint32_t dir;", "  uint32_t n_reads, n_rows, n_exact;", "  uint32_t lo_pos, hi_pos;", "  uint64_t clip_sum, mapq_sum;", "  int32_t mate_off;",
                 "struct bk_clip_locus {"):
        assert line in header, line
    assert "scope `clip_loci`" in header and "`clip_loci_records`" in header and "`clip_loci_calls`" in header
    assert "Nothing is capped" in header and "No atomic anywhere" in header and "The host reads a count three times" in header
    assert "exactly what bk_clip_support (above) defines" in header and "typedef struct bk_clip_locus" not in header
    # one statement of the event rule on the device, used by both translation units
    csrc = os.path.join(ROOT, "breakid_amd", "csrc")
    assert open(os.path.join(csrc, "clip.h")).read().count("void clip_events(") == 1
    for f in ("clip.hip", "cliploci.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "clip_events(" in text and "void clip_events(" not in text and "bool cigar_op_ref(" not in text, f
    # the shim of the CPU build does not have the call
    shim = open(os.path.join(ROOT, "oracle", "Makefile")).read() + "".join(open(os.path.join(ROOT, "oracle", f)).read() for f in os.listdir(os.path.join(ROOT, "oracle")) if f.endswith((".cc", ".h")))
    assert "bk_clip_loci" not in shim


def hand_cols():
    contigs, recs = lc.hand_example()
    return lc.dataset(contigs, recs).to_soa()


def test_hand_example():
    """the header's: one contig of 1 000 000 bases, mapq_min 20, min_clip 10, tol 2, pair_dist 50, min_reads 1"""
    cols = hand_cols()
    rows, counts = lc.both(cols, TLEN[:1])
    assert counts == dict(records=10, eligible=8, events=7, beyond=0, exact=4, loci=3, mutual=2, written=3)
    assert [tuple(int(v) for v in r) for r in rows] == [
        (0, 999, 0, 3, 4, 4, 2, 3, 999, 1001, 3, 1, 50, 0, 199, 220, 0, NONE, 1, 990, 2, -9),
        (0, 990, 1, 3, 2, 2, 1, 2, 990, 990, 2, 0, 50, 0, 100, 120, 0, NONE, 0, 999, 4, -9),
        (0, 5001, 1, 0, 1, 1, 1, 1, 5001, 5001, 1, 0, 30, 1, 30, 60, 0, NONE, NONE, 0, 0, 0)]
    why = [lc.why_dropped(cols, i, TLEN[:1], 20, 10) for i in range(10)]
    assert sorted(w for w in why if w) == ["aux", "mapq", "short"] and why.count(None) == 7
    # the numbers of the header's text
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "Counts: 10 records, 8 eligible, 7 events, 0 beyond, 4 exact, 3 loci, 2 with a mutual partner, 3 returned." in header
    assert "max_clip 50, clip_sum 199, mapq_sum 220, mate 1," in header and "mate_off -9 (ten bases duplicated), flags 3." in header
    # tol 1 splits the LEFT locus; min_reads 2 drops the orphan locus and keeps the others' bytes; pair_dist 9 ends the facing
    assert lc.both(cols, TLEN[:1], tol=1)[1]["loci"] == 4
    only, counts = lc.both(cols, TLEN[:1], min_reads=2)
    assert only.tobytes() == rows[:2].tobytes() and counts["loci"] == 3 and counts["written"] == 2
    assert lc.both(cols, TLEN[:1], pair_dist=10)[1]["mutual"] == 2 and lc.both(cols, TLEN[:1], pair_dist=9)[1]["mutual"] == 0
    assert lc.both(cols, TLEN[:1], mapq_min=61)[1]["eligible"] == 0 and lc.both(cols, TLEN[:1], min_clip=50)[1]["events"] == 5


def test_designed_inputs():
    """what the GPU tests design, small"""
    def one(cigar, pos=1000, tid=0, **kw):
        return lc.both(lc.dataset(CONTIGS, [lc.read("q", tid, pos, cigar)]).to_soa(), TLEN, **kw)
    ev = lambda rows: [(int(r["dir"]), int(r["pos"]), int(r["max_clip"])) for r in rows]  # noqa: E731
    assert ev(one("5H30S65M")[0]) == [(1, 1001, 30)] and ev(one("30S5I100M")[0]) == [(1, 1001, 30)] and ev(one("65M30S5H")[0]) == [(0, 1065, 30)]
    assert ev(one("3H2H12S60M13S5H")[0]) == [(0, 1060, 13), (1, 1001, 12)]
    for cigar in ("30S5I", "5H30S", "5H", "*", "100M", "9S91M", "30M30S30M"):
        rows, counts = one(cigar)
        assert len(rows) == 0 and counts["events"] == 0 and counts["eligible"] == (cigar in ("100M", "9S91M", "30M30S30M")), cigar
    assert len(one("25S50M25S", min_clip=25)[0]) == 2 and len(one("25S50M25S", min_clip=26)[0]) == 0
    # chr2 has 5000 bases: a trailing event at its last base is kept, one beyond it is dropped and counted
    assert ev(one("60M40S", pos=4940, tid=1)[0]) == [(0, 5000, 40)] and one("60M40S", pos=4941, tid=1)[1] == dict(records=1, eligible=1, events=1, beyond=1, exact=0, loci=0, mutual=0, written=0)
    rows, counts = one("40S60M40S", pos=4941, tid=1)
    assert ev(rows) == [(1, 4942, 40)] and counts["events"] == 2 and counts["beyond"] == 1
    # facing: the offsets -pair_dist - 1 .. pair_dist + 1 around blunt
    for pair_dist in (0, 3, 50):
        for off in range(-pair_dist - 1, pair_dist + 2):
            recs = [lc.left_clip("l", 0, 2000), lc.right_clip("r", 0, 2001 + off)]
            rows, counts = lc.both(lc.dataset(CONTIGS, recs).to_soa(), TLEN, pair_dist=pair_dist)
            inside = abs(off) <= pair_dist
            assert counts["mutual"] == (2 if inside else 0)
            assert [(int(r["flags"]), int(r["mate"]), int(r["mate_off"])) for r in rows] == ([(3, 1, off + 1), (3, 0, off + 1)] if inside else [(0, NONE, 0)] * 2)
    # the partner: most reads, then the smaller distance, then the smaller position; a partner need not be mutual
    recs = [lc.left_clip("l", 0, 2000)] + [lc.right_clip("a", 0, 2001 + 7), lc.right_clip("b", 0, 2001 - 7), lc.right_clip("c", 0, 2001 + 9), lc.right_clip("c2", 0, 2001 + 9)]
    rows, _ = lc.both(lc.dataset(CONTIGS, recs).to_soa(), TLEN, tol=0)
    assert (int(rows[0]["mate_pos"]), int(rows[0]["mate_reads"])) == (2010, 2)
    rows, _ = lc.both(lc.dataset(CONTIGS, recs[:3] + [lc.right_clip("d", 0, 2001 + 6)]).to_soa(), TLEN, tol=0)
    assert (int(rows[0]["mate_pos"]), int(rows[0]["mate_off"])) == (2007, 7)
    rows, _ = lc.both(lc.dataset(CONTIGS, recs[:3]).to_soa(), TLEN, tol=0)
    assert (int(rows[0]["mate_pos"]), int(rows[0]["mate_off"]), int(rows[0]["flags"])) == (1994, -6, 3) and [int(r["flags"]) for r in rows[1:]] == [3, 1]
    # a partner that min_reads drops
    rows, _ = lc.both(lc.dataset(CONTIGS, [lc.left_clip("l1", 0, 2000), lc.left_clip("l2", 0, 2000), lc.right_clip("r", 0, 2001)]).to_soa(), TLEN, min_reads=2)
    assert [tuple(int(rows[0][f]) for f in ("flags", "mate", "mate_pos", "mate_reads", "mate_off"))] == [(3, NONE, 2001, 1, 1)] and len(rows) == 1
    # the claim: the smallest voted row within 2 of the span
    cl = np.zeros(4, abi.CLUSTER)
    cl["flags"] = [2, 0, 2, 2]
    cl["p1_tid"], cl["p1_exact"], cl["p2_tid"], cl["p2_exact"] = [1, 0, 0, 0], [9, 1998, 2003, 1997], [0, 0, 1, 0], [2100, 2000, 2002, 2002]
    claim = lambda p: int(lc.both(lc.dataset(CONTIGS, [lc.left_clip("l", 0, p)]).to_soa(), TLEN, cl=cl)[0][0]["claim"])  # noqa: E731
    assert [claim(p) for p in (1994, 1995, 2000, 2001, 2005, 2006, 2098, 2102, 2103)] == [NONE, 3, 3, 2, 2, NONE, 0, 0, NONE]


def test_the_two_statements_agree_and_reach_every_shape():
    """300 seeded tables of up to 60 records on three short contigs under three settings"""
    rng = np.random.default_rng(31)
    tlen = [400, 320, 2000]
    seen = dict(unmapped=0, flag=0, mapq=0, aux=0, no_ref=0, no_clip=0, short=0, beyond=0, kept=0, two_events=0, behind_hard=0, multi_exact=0, shared_reads=0, tie=0, left=0, right=0,
                below_min=0, duplicated=0, blunt=0, lost=0, not_mutual=0, mate_dropped=0, at_pair_dist=0, past_pair_dist=0, partner_tie=0, orphan=0, improper=0, claimed=0)
    for case in range(300):
        cols = lc.random_cols(rng, int(rng.integers(1, 60)), tlen)
        for i in range(len(cols["tid"])):
            why = lc.why_dropped(cols, i, tlen, 20, 10)
            seen[why or "kept"] += 1
            if why is None:
                seen["two_events"] += len(lc.record_events(cols, i, tlen, 10)[1]) > 1
                seen["behind_hard"] += lc.record_ops(cols, i)[0][0] == lc.OP_H
        cl = np.zeros(3, abi.CLUSTER)
        cl["flags"], cl["p1_tid"], cl["p2_tid"] = [2, 2, 0], rng.integers(0, 3, 3), rng.integers(0, 3, 3)
        cl["p1_exact"], cl["p2_exact"] = 200 + rng.integers(0, 90, 3), 200 + rng.integers(0, 90, 3)
        for tol, pair_dist in ((0, 0), (2, 20), (100, 3)):
            a, counts = lc.both(cols, tlen, tol=tol, pair_dist=pair_dist, cl=cl)
            assert np.all(a["n_reads"] <= a["n_rows"]) and np.all(a["top_reads"] <= a["n_reads"]) and np.all(a["n_fwd"] + a["n_rev"] == a["n_rows"]) and np.all(a["n_exact"] <= a["n_rows"])
            assert np.all(a["lo_pos"] <= a["pos"]) and np.all(a["pos"] <= a["hi_pos"]) and np.all(a["max_clip"] * a["n_rows"] >= a["clip_sum"]) and np.all(a["max_clip"] >= 10)
            assert int(a["n_rows"].sum()) == counts["events"] - counts["beyond"] and int(a["n_exact"].sum()) == counts["exact"] and len(a) == counts["loci"]
            assert int(((a["flags"] & 2) != 0).sum()) == counts["mutual"] and np.all((a["flags"] & 1) | ((a["flags"] & 2) == 0))
            order = [(int(r["dir"]), int(r["tid"]), int(r["lo_pos"])) for r in a]
            assert order == sorted(order)
            if tol == 0:
                assert np.all(a["n_exact"] == 1) and counts["loci"] == counts["exact"]
            facing = a[(a["flags"] & 1) != 0]
            assert np.all(np.abs(facing["mate_off"].astype(np.int64) - 1) <= pair_dist)
            for k, r in enumerate(a):
                if int(r["flags"]) & 1:
                    m = a[int(r["mate"])]
                    assert (int(m["pos"]), int(m["n_reads"]), int(m["dir"]), int(m["tid"])) == (int(r["mate_pos"]), int(r["mate_reads"]), 1 - int(r["dir"]), int(r["tid"]))
                    assert bool(int(r["flags"]) & 2) == (int(m["mate"]) == k)
            seen["multi_exact"] += int((a["n_exact"] > 1).sum())
            seen["shared_reads"] += int((a["n_reads"] < a["n_rows"]).sum())
            seen["tie"] += int(((a["n_exact"] > 1) & (a["top_reads"] * a["n_exact"] == a["n_reads"])).sum())
            seen["left"] += int((a["dir"] == 0).sum())
            seen["right"] += int((a["dir"] == 1).sum())
            seen["duplicated"] += int((facing["mate_off"] <= 0).sum())
            seen["blunt"] += int((facing["mate_off"] == 1).sum())
            seen["lost"] += int((facing["mate_off"] > 1).sum())
            seen["not_mutual"] += int((facing["flags"] == 1).sum())
            seen["at_pair_dist"] += int((np.abs(facing["mate_off"].astype(np.int64) - 1) == pair_dist).sum())
            seen["orphan"] += int((a["n_orphan"] > 0).sum())
            seen["improper"] += int((a["n_improper"] > 0).sum())
            seen["claimed"] += int((a["claim"] != NONE).sum())
            # a locus just outside pair_dist, and partners that tie on reads
            for r in a[(a["flags"] & 1) == 0]:
                other = a[(a["dir"] != r["dir"]) & (a["tid"] == r["tid"])]
                centre = int(r["pos"]) + (1 if int(r["dir"]) == 0 else -1)
                seen["past_pair_dist"] += bool(np.any(np.abs(other["pos"].astype(np.int64) - centre) == pair_dist + 1))
            for r in facing:
                other = a[(a["dir"] != r["dir"]) & (a["tid"] == r["tid"]) & (a["n_reads"] == r["mate_reads"])]
                centre = int(r["pos"]) + (1 if int(r["dir"]) == 0 else -1)
                seen["partner_tie"] += int((np.abs(other["pos"].astype(np.int64) - centre) <= pair_dist).sum()) > 1
            b, cb = lc.both(cols, tlen, tol=tol, pair_dist=pair_dist, min_reads=2, cl=cl)
            seen["below_min"] += len(a) - len(b)
            kept = a[a["n_reads"] >= 2]
            assert cb["loci"] == counts["loci"] and cb["mutual"] == counts["mutual"] and cb["written"] == len(b) == len(kept)
            for f in FIELDS:
                if f != "mate":
                    assert np.array_equal(b[f], kept[f]), f
            seen["mate_dropped"] += int((((b["flags"] & 1) != 0) & (b["mate"] == NONE)).sum())
    assert min(seen.values()) >= 10, seen


def test_formatters():
    rows = np.zeros(3, abi.CLIP_LOCUS)
    r = rows[0]
    r["tid"], r["pos"], r["dir"], r["flags"], r["n_reads"], r["n_rows"], r["n_exact"], r["top_reads"] = 0, 999, 0, 3, 4, 4, 2, 3
    r["lo_pos"], r["hi_pos"], r["n_fwd"], r["n_rev"], r["max_clip"], r["n_orphan"], r["clip_sum"], r["mapq_sum"], r["n_improper"] = 999, 1001, 3, 1, 50, 1, 199, 221, 2
    r["claim"], r["mate"], r["mate_pos"], r["mate_reads"], r["mate_off"] = NONE, 1, 990, 2, -9
    rows[1]["pos"], rows[1]["dir"], rows[1]["flags"], rows[1]["n_reads"], rows[1]["n_rows"], rows[1]["claim"], rows[1]["mate"] = 990, 1, 3, 2, 2, NONE, 0
    rows[2]["pos"], rows[2]["dir"], rows[2]["n_reads"], rows[2]["n_rows"], rows[2]["claim"], rows[2]["mate"] = 5001, 1, 1, 1, 7, NONE
    assert lc.row_fields(0, rows[0], rows, ["chrA"], 30, "G1") == ["cl0", "chrA", "999", "L", "4", "4", "2", "3", "3", "1", "55.2", "999-1001", "50", "49.8", "1", "2", "cl1", "990", "2", "-9",
                                                                   "1", "30", "G1"]
    assert lc.row_fields(2, rows[2], rows, ["chrA"], 5)[16:] == [".", ".", ".", ".", "0", "5", "intergenic"] and len(lc.COLUMNS) == 23
    assert lc.written(rows) == [0, 1] and lc.bedpe_pairs(rows) == [(0, 1)]
    assert lc.bedpe_line(0, 1, rows, ["chrA"], "run") == "chrA\t998\t999\tchrA\t989\t990\trun\t6\t+\t-\tcl0\tinsertion_site\t0\t6"
    rows[1]["claim"] = 3  # a claimed mate is not named, and its pair is not a BEDPE line
    assert lc.row_fields(0, rows[0], rows, ["chrA"], 30)[16:20] == [".", "990", "2", "-9"] and lc.bedpe_pairs(rows) == [] and lc.written(rows) == [0]
    counts = dict(eligible=8, events=7, beyond=1, exact=4, loci=3, mutual=2)
    assert lc.stdout_line(counts, rows) == "cliploci: 8 records eligible, 7 events, 1 beyond a contig's end, 4 exact, 3 loci, 2 with a mutual partner, 2 claimed by a voted call, 1 written"


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_cliploci(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for args in (["-cliploci"], ["-cliploci", "-locitol", "0", "-locipair", "0", "-locisupport", "1", "-minclip", "5", "-all", "-fast"],
                 ["-cliploci", "-locitol", "100", "-locipair", "100000", "-locisupport", "1000000"]):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: -cliploci needs the GPU library" in r.stderr and "Usage" not in r.stderr, (args, r.stderr[-2000:])
    need = "Error: -locitol, -locipair and -locisupport need -cliploci."
    for args, word in ((["-locitol", "1"], need), (["-locipair", "5"], need), (["-locisupport", "1"], need),
                       (["-minclip", "5"], "Error: -minclip and -clipsupport need -clip."),
                       (["-cliploci", "-clipsupport", "5"], "Error: -minclip and -clipsupport need -clip."),
                       (["-cliploci", "-gpus", "2"], "Error: -cliploci cannot be combined with -gpus."),
                       (["-cliploci", "-minclip", "0"], "Error: -minclip must be a number from 1 to 2147483647."),
                       (["-cliploci", "-locitol", "101"], "Error: -locitol must be a number from 0 to 100."), (["-cliploci", "-locitol", "-1"], "Error: -locitol must be a number from 0 to 100."),
                       (["-cliploci", "-locipair", "100001"], "Error: -locipair must be a number from 0 to 100000."),
                       (["-cliploci", "-locipair", "-1"], "Error: -locipair must be a number from 0 to 100000."),
                       (["-cliploci", "-locisupport", "0"], "Error: -locisupport must be a number from 1 to 1000000."),
                       (["-cliploci", "-locisupport", "1000001"], "Error: -locisupport must be a number from 1 to 1000000."),
                       (["-cliploci", "-gaptol", "1"], "Error: -mingap, -gapanchor, -gaptol and -gapsupport need -gaps.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert all(w in r.stderr for w in ("-cliploci ", "-locitol", "-locipair", "-locisupport")) and "Error" not in r.stderr
    assert r.stderr.index("-gapsupport") < r.stderr.index("-cliploci ")

"""Split junctions without a GPU: the row layout, the exports and the header's text; the two statements of the definition in
tests/junctioncases.py on seeded small cases that reach every kind of dropped tuple, chains, ties and both kinds of claimed row; the
hand example of the header; how the command line names a junction's type and size; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import junctioncases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layout_and_exports():
    d = abi.SPLIT_JUNCTION
    assert d.itemsize == 72 and list(d.names) == list(jc.FIELDS)
    assert [d.fields[f][1] for f in d.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 52, 60, 64, 65, 66, 67, 68]
    assert d.fields["tid1"][0] == np.dtype("<i4") and d.fields["call"][0] == np.dtype("<i4") and d.fields["pos2"][0] == np.dtype("<u4")
    assert d.fields["n_own"][0] == np.dtype(("<u4", (2,))) and d.fields["mapq_sum"][0] == np.dtype(("<u4", (2,))) and d.fields["call_crossed"][0] == np.dtype("u1")
    assert abi.SJ_MAX_TOL == jc.MAX_TOL == 100
    for name in ("bk_split_junctions", "bk_split_junction_counts", "bk_debug_split_junctions"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert hasattr(capi.Context, "split_junctions") and hasattr(capi.Context, "split_junction_counts")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "int bk_split_junctions(bk_ctx *ctx, int mapq_min, uint32_t tol, uint32_t min_reads, const struct bk_split_junction **out, uint64_t *count);" in header
    assert "int bk_split_junction_counts(bk_ctx *ctx, uint64_t out[6]);" in header and "#define BK_SJ_MAX_TOL 100u\n" in header
    for line in ("  int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2;", "  uint32_t n_reads, n_tuples, n_exact;", "  uint32_t lo1, hi1, lo2, hi2;", "  uint32_t n_own[2];",
                 "  uint32_t mapq_sum[2];", "  int32_t call;", "  uint8_t right1, right2, call_crossed, reserved;", "  uint32_t top_reads;"):
        assert line in header, line
    assert "scope `split_junctions`" in header and "Single linkage can chain" in header and "Nothing is capped" in header and "costs k * k" in header
    assert "2^30 eligible tuples" in header and "No atomics on results" in header and "more than 2^30 sequences" in header
    # the shim of the CPU build does not have the call
    shim = open(os.path.join(ROOT, "oracle", "Makefile")).read() + "".join(open(os.path.join(ROOT, "oracle", f)).read() for f in os.listdir(os.path.join(ROOT, "oracle")) if f.endswith((".cc", ".h")))
    assert "bk_split_junctions" not in shim


TLEN = [1000, 2000, 500]


def test_the_two_statements_agree_and_reach_every_shape():
    """24 seeded cases of up to 120 tuples on three short contigs under tol 0, 2 and 25, with and without voted rows"""
    rng = np.random.default_rng(28)
    seen = dict(poison=0, own_contig=0, other_contig=0, position=0, unmapped=0, qcfail=0, mapq=0, identical=0, eligible=0, own_second=0, same_position=0, multi_exact=0,
                shared_reads=0, tie=0, straight=0, crossed=0, unclaimed=0, below_min=0)
    for case in range(24):
        splits, flag, mapq = jc.random_case(rng, int(rng.integers(1, 120)), TLEN)
        cl = jc.random_clusters(rng, 12, TLEN) if case % 4 else None
        for s in splits:
            why = jc.why_dropped(s, flag, mapq, TLEN, 20)
            seen[why or "eligible"] += 1
            if why is None:
                e1, e2, own_end = jc.canonical(s)
                assert e1 < e2
                seen["own_second"] += own_end
                seen["same_position"] += e1[:2] == e2[:2]
        for tol in (0, 2, 25):
            info = {}
            a = jc.expected(splits, flag, mapq, TLEN, 20, tol, 1, cl, info)
            assert a.tobytes() == jc.expected_sweep(splits, flag, mapq, TLEN, 20, tol, 1, cl).tobytes(), (case, tol)
            assert np.all(a["reserved"] == 0) and np.all(a["n_reads"] <= a["n_tuples"]) and np.all(a["n_own"].sum(axis=1) == a["n_tuples"]) and np.all(a["top_reads"] <= a["n_reads"])
            assert np.all(a["lo1"] <= a["pos1"]) and np.all(a["pos1"] <= a["hi1"]) and np.all(a["lo2"] <= a["pos2"]) and np.all(a["pos2"] <= a["hi2"])
            assert int(a["n_tuples"].sum()) == info["eligible"] and int(a["n_exact"].sum()) == info["exact"] and len(a) == info["calls"]
            if tol == 0:
                assert np.all(a["n_exact"] == 1)
            keys, table = info["keys"], jc.exact_table(splits, flag, mapq, TLEN, 20)
            for r, members in zip(a, info["members"]):
                reads = [len({q for q, _, _ in table[keys[j]]}) for j in members]
                seen["tie"] += len(members) > 1 and reads.count(max(reads)) > 1
                seen["shared_reads"] += int(r["n_reads"]) < sum(reads)
            seen["multi_exact"] += int((a["n_exact"] > 1).sum())
            seen["straight"] += int(((a["call"] >= 0) & (a["call_crossed"] == 0)).sum())
            seen["crossed"] += int(a["call_crossed"].sum())
            seen["unclaimed"] += int((a["call"] < 0).sum())
            if cl is None:
                assert np.all(a["call"] == -1) and np.all(a["call_crossed"] == 0)
            b = jc.expected(splits, flag, mapq, TLEN, 20, tol, 3, cl)
            seen["below_min"] += len(a) - len(b)
            assert b.tobytes() == a[a["n_reads"] >= 3].tobytes() == jc.expected_sweep(splits, flag, mapq, TLEN, 20, tol, 3, cl).tobytes()
    assert min(seen.values()) >= 10, seen


def hand_example():
    rows = [(k, 100 + k, (0, 5000, 0), (0, 5250, 1), 0) for k in range(3)]                       # reads a, b, c
    rows += [(3, 200, (0, 5251, 1), (0, 5001, 0), 0), (4, 200, (0, 5001, 0), (0, 5251, 1), 0)]  # read d, two alignments
    rows += [(5, 300, (1, 700, 1), (0, 5000, 0), 0)]                                             # read e
    return jc.make_splits(rows), np.zeros(6, np.uint16), np.full(6, 60, np.uint8), [1_000_000, 1_000_000]


def test_hand_example():
    """the header's: chr1 = 0, chr2 = 1, tol 2, min_reads 1"""
    splits, flag, mapq, tlen = hand_example()
    assert [jc.canonical(s)[2] for s in splits] == [0, 0, 0, 1, 0, 1]
    a = jc.expected(splits, flag, mapq, tlen, 20, 2, 1)
    assert a.tobytes() == jc.expected_sweep(splits, flag, mapq, tlen, 20, 2, 1).tobytes() and len(a) == 2
    r = a[0]
    assert (int(r["tid1"]), int(r["pos1"]), int(r["tid2"]), int(r["pos2"]), int(r["right1"]), int(r["right2"])) == (0, 5000, 0, 5250, 0, 1)
    assert (int(r["n_reads"]), int(r["n_tuples"]), int(r["n_exact"]), int(r["top_reads"]), int(r["call"])) == (4, 5, 2, 3, -1)
    assert (int(r["lo1"]), int(r["hi1"]), int(r["lo2"]), int(r["hi2"]), list(r["n_own"]), list(r["mapq_sum"])) == (5000, 5001, 5250, 5251, [4, 1], [240, 60])
    r = a[1]
    assert (int(r["tid1"]), int(r["pos1"]), int(r["tid2"]), int(r["pos2"]), int(r["right1"]), int(r["right2"])) == (0, 5000, 1, 700, 0, 1)
    assert (int(r["n_reads"]), int(r["n_tuples"]), int(r["n_exact"]), int(r["top_reads"]), list(r["n_own"]), list(r["mapq_sum"])) == (1, 1, 1, 1, [0, 1], [0, 60])
    assert len(jc.expected(splits, flag, mapq, tlen, 20, 0, 1)) == 3 and len(jc.expected(splits, flag, mapq, tlen, 20, 1, 1)) == 2
    only = jc.expected(splits, flag, mapq, tlen, 20, 2, 3)
    assert len(only) == 1 and only[0].tobytes() == a[0].tobytes()
    # a voted row at the deletion, both ways round, and 3 bp off
    for p1, p2, call, crossed in (((0, 5002), (0, 5252), 0, 0), ((0, 5252), (0, 5002), 0, 1), ((0, 5004), (0, 5250), -1, 0), ((1, 700), (0, 5000), -1, 0)):
        cl = np.zeros(1, abi.CLUSTER)
        cl["p1_tid"], cl["p1_exact"], cl["p2_tid"], cl["p2_exact"], cl["flags"] = p1[0], p1[1], p2[0], p2[1], 3
        r = jc.expected(splits, flag, mapq, tlen, 20, 2, 1, cl)[0]
        assert (int(r["call"]), int(r["call_crossed"])) == (call, crossed), (p1, p2)
    cl["flags"] = 1  # the row is not voted
    assert int(jc.expected(splits, flag, mapq, tlen, 20, 2, 1, cl)[1]["call"]) == -1
    # mapq_min above the reads' 60: nothing is eligible
    assert len(jc.expected(splits, flag, mapq, tlen, 61, 2, 1)) == 0


def test_type_and_size():
    def row(t1, p1, r1, t2, p2, r2):
        r = np.zeros((), abi.SPLIT_JUNCTION)
        r["tid1"], r["pos1"], r["right1"], r["tid2"], r["pos2"], r["right2"] = t1, p1, r1, t2, p2, r2
        return r
    assert jc.type_size(row(0, 100, 0, 0, 350, 1)) == ("deletion", "250")
    assert jc.type_size(row(0, 100, 1, 0, 350, 0)) == ("duplication", "250")
    assert jc.type_size(row(0, 100, 0, 0, 350, 0)) == ("inversion", "250") and jc.type_size(row(0, 100, 1, 0, 350, 1)) == ("inversion", "250")
    assert jc.type_size(row(0, 100, 0, 0, 100, 1)) == (".", "0")
    assert jc.type_size(row(0, 100, 0, 1, 50, 1)) == ("translocation", ".") and jc.type_size(row(2, 7, 1, 3, 7, 1)) == ("translocation", ".")
    r = row(0, 100, 0, 0, 350, 1)
    r["n_reads"], r["n_tuples"], r["n_exact"], r["top_reads"], r["n_own"], r["mapq_sum"] = 5, 6, 2, 4, (6, 0), (301, 0)
    r["lo1"], r["hi1"], r["lo2"], r["hi2"] = 99, 100, 350, 352
    assert jc.row_fields(7, r, ["chrA"], 30, 31, "G1", "intergenic") == ["sj7", "chrA", "100", "L", "chrA", "350", "R", "deletion", "250", "5", "6", "2", "4", "6", "0", "50.2", ".",
                                                                        "99-100", "350-352", "30", "31", "G1", "intergenic"]
    assert len(jc.COLUMNS) == 23
    assert jc.bedpe_line(7, r, ["chrA"], "run") == "chrA\t99\t100\tchrA\t349\t350\trun\t5\t+\t-\tsj7\tdeletion\t0\t5"


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_junctions(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for args in (["-junctions"], ["-junctions", "-jsupport", "2", "-jtol", "0", "-all", "-fast"], ["-junctions", "-jsupport", "1000000", "-jtol", "100"]):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: -junctions needs the GPU library" in r.stderr and "Usage" not in r.stderr, (args, r.stderr[-2000:])
    # the usage refusals stand behind the help text, in the order of the table: the new rows behind every older row
    for args, word in ((["-jtol", "1"], "Error: -jsupport and -jtol need -junctions."), (["-jsupport", "5"], "Error: -jsupport and -jtol need -junctions."),
                       (["-junctions", "-gpus", "2"], "Error: -junctions cannot be combined with -gpus."),
                       (["-junctions", "-gpus", "2", "-jtol", "101"], "Error: -junctions cannot be combined with -gpus."),
                       (["-junctions", "-jtol", "101"], "Error: -jtol must be a number from 0 to 100."), (["-junctions", "-jtol", "-1"], "Error: -jtol must be a number from 0 to 100."),
                       (["-junctions", "-jsupport", "0"], "Error: -jsupport must be a number from 1 to 1000000."),
                       (["-junctions", "-jsupport", "0", "-jtol", "101"], "Error: -jsupport must be a number from 1 to 1000000."),
                       (["-junctions", "-jsupport", "1000001"], "Error: -jsupport must be a number from 1 to 1000000."),
                       (["-junctions", "-ctxflank", "5"], "Error: -ctxflank needs -context."),
                       (["-bedpe", "-junctions", "-fragsize"], None)):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        if word is None:  # (an earlier row of the table)
            assert r.returncode == 1 and errors == ["Error: -fragsize needs the GPU library"], (args, r.stderr[-2000:])
        else:
            assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-junctions " in r.stderr and "-jsupport" in r.stderr and "-jtol" in r.stderr and "Error" not in r.stderr

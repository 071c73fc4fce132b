"""Locus similarity without a GPU: the row layouts and the exports, the fast Python definition (tests/similarcases.py) against a brute
force over every segment, designed forward and reverse-complement copies, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import homologycases as hc
from tests import similarcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.LOCUS_PAIR.itemsize == 16 and abi.LOCUS_SIM.itemsize == 32
    assert list(abi.LOCUS_PAIR.names) == ["tid_a", "pos_a", "tid_b", "pos_b"]
    assert list(abi.LOCUS_SIM.names) == ["score", "len", "mism", "run", "diag", "start", "orient", "found"]
    assert [abi.LOCUS_PAIR.fields[f][1] for f in abi.LOCUS_PAIR.names] == list(range(0, 16, 4))
    assert [abi.LOCUS_SIM.fields[f][1] for f in abi.LOCUS_SIM.names] == list(range(0, 32, 4))
    assert abi.LOCUS_PAIR.fields["tid_a"][0] == np.dtype("<i4") and abi.LOCUS_PAIR.fields["tid_b"][0] == np.dtype("<i4")
    assert abi.LOCUS_SIM.fields["diag"][0] == np.dtype("<i4") and abi.LOCUS_SIM.fields["score"][0] == np.dtype("<u4")
    assert "bk_locus_similarity" in capi.EXPORTS and hasattr(capi.lib(), "bk_locus_similarity") and hasattr(capi.Context, "locus_similarity")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_locus_pair { int32_t tid_a; uint32_t pos_a; int32_t tid_b; uint32_t pos_b; };" in header
    assert "struct bk_locus_sim  { uint32_t score, len, mism, run; int32_t diag; uint32_t start, orient, found; };" in header
    assert "int bk_locus_similarity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_locus_pair *pairs, uint64_t n, uint32_t flank, const struct bk_locus_sim **out);" in header


def test_definition_equals_a_brute_force_over_every_segment():
    """300 seeded cases with R <= 4: alphabets of 2 to 5 symbols (the fifth is N), two contigs or one, and on one contig the two
    positions so near that the excluded diagonal lies inside the search"""
    rng = np.random.default_rng(20)
    same = excl = found = 0
    for case in range(300):
        R = int(rng.integers(1, 5))
        symbols = int(rng.integers(2, 6))
        size = 30
        contigs = [rng.integers(0, symbols, size), rng.integers(0, symbols, size)]
        if case % 3 == 0:  # one contig, the windows overlap or nearly
            pa = int(rng.integers(1, size + 1))
            pair = (0, pa, 0, max(1, min(size, pa + int(rng.integers(-2 * R - 1, 2 * R + 2)))))
            same += 1
            excl += abs(pair[1] - pair[3]) <= 2 * R
        else:
            pair = (int(rng.integers(0, 2)), int(rng.integers(1, size + 1)), int(rng.integers(0, 2)), int(rng.integers(1, size + 1)))
        ref = sc.codes_to_ref(contigs)
        fast = sc.expected_sim(ref, sc.as_pairs([pair]), R)[0]
        slow = sc.brute_force(ref, pair, R)
        assert fast.tobytes() == slow.tobytes(), (case, R, pair, fast, slow)
        assert int(fast["found"]) == int(int(fast["run"]) >= 1)
        found += int(fast["found"])
    assert same == 100 and excl > 60 and 200 < found < 300


def designed():
    """two contigs of 1000 random bases; an 80-base stretch of contig 0 copied forward into contig 1 with 3 substitutions, and a
    60-base stretch reverse-complemented with none"""
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 4, 1000), rng.integers(0, 4, 1000)
    # forward: a[200 .. 279] (0-based) lies at b[330 .. 409]; substitutions at copy offsets 20, 40, 60
    sc.plant(a, 200, b, 330, 80, reverse=False, subs=(20, 40, 60))
    # reverse: a[700 .. 759] lies reverse-complemented at b[800 .. 859]
    sc.plant(a, 700, b, 800, 60, reverse=True)
    return sc.codes_to_ref([a, b])


def test_designed_copies_give_their_planted_values():
    ref = designed()
    R = 100
    # forward: window A around 1-based 250 = columns for 150 .. 350; the copy starts at 1-based 201: start = 201 - 150 = 51;
    # window B around 361: its column of 1-based 331 is 331 - 261 = 70: diag = 70 - 51 = 19
    pairs = sc.as_pairs([(0, 250, 1, 361), (0, 730, 1, 840)])
    rows = sc.expected_sim(ref, pairs, R)
    f = rows[0]
    assert (int(f["found"]), int(f["score"]), int(f["len"]), int(f["mism"]), int(f["orient"]), int(f["start"]), int(f["diag"])) == (1, 80 - 3 * 3, 80, 3, 0, 51, 19), f
    assert int(f["run"]) >= 20  # the longest clean part of the copy: 20, 19, 19 and 19 bases (or longer by chance)
    assert sc.twin_fields(pairs[0], R, f) == ["71", "80", "3", str(int(f["run"])), "+", "201", "331"]
    # reverse: window A around 730 = 630 .. 830, the stretch 701 .. 760 starts in column 71; it lies at 801 .. 860 of contig 1
    r = rows[1]
    assert (int(r["found"]), int(r["score"]), int(r["len"]), int(r["mism"]), int(r["orient"]), int(r["start"])) == (1, 60, 60, 0, 1, 71), r
    assert int(r["run"]) == 60
    # b1[j] = comp(ref(1, 840 + 100 - j)); column 71 of A meets 1-based 860: j = 80, diag = 9
    assert int(r["diag"]) == 9
    assert sc.twin_fields(pairs[1], R, r) == ["60", "60", "0", "60", "-", "701", "801"]
    # the roles exchanged find the same stretches
    back = sc.expected_sim(ref, sc.as_pairs([(1, 361, 0, 250), (1, 840, 0, 730)]), R)
    assert [int(x) for x in back["score"]] == [71, 60] and [int(x) for x in back["orient"]] == [0, 1]
    assert sc.twin_fields(sc.as_pairs([(1, 361, 0, 250)])[0], R, back[0])[5:] == ["331", "201"]
    assert sc.twin_fields(sc.as_pairs([(1, 840, 0, 730)])[0], R, back[1])[5:] == ["801", "701"]
    # nothing to find: a tid below 0, a contig without a segment, an empty table
    none = sc.expected_sim(ref, sc.as_pairs([(-1, 250, 1, 361), (0, 250, 5, 361)]), R)
    assert not none.tobytes().strip(b"\0")
    assert not sc.expected_sim(hc.make_refseq([]), pairs, R).tobytes().strip(b"\0")
    assert sc.twin_fields(pairs[0], R, none[0]) == ["0", "0", "0", "0", ".", ".", "."]


def test_excluded_diagonal_and_background():
    rng = np.random.default_rng(8)
    ref = sc.codes_to_ref([rng.integers(0, 4, 2000), rng.integers(0, 4, 2000)])
    R = 50
    L = 2 * R + 1
    same = sc.expected_sim(ref, sc.as_pairs([(0, 1000, 0, 1000)]), R)[0]
    assert 0 < int(same["score"]) < 20 and not (int(same["orient"]) == 0 and int(same["diag"]) == 0)  # background, not L
    # the same bases on another contig: the whole window
    twin = sc.codes_to_ref([rng.integers(0, 4, 2000)] * 2)
    full = sc.expected_sim(twin, sc.as_pairs([(0, 1000, 1, 1000)]), R)[0]
    assert (int(full["score"]), int(full["len"]), int(full["diag"]), int(full["start"]), int(full["orient"]), int(full["run"])) == (L, L, 0, 0, 0, L)
    # a dinucleotide repeat: the excluded diagonal's neighbours at |d| = 2 win, d >= 0 first
    di, _ = hc.repeat_ref("AC", 2000)
    r = sc.expected_sim(di, sc.as_pairs([(0, 1000, 0, 1000)]), R)[0]
    assert (int(r["diag"]), int(r["orient"]), int(r["score"]), int(r["len"]), int(r["start"])) == (2, 0, L - 2, L - 2, 0)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_similar(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-similar"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -similar needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-similar", "-simflank", "100", "-all", "-fast", "-vcf"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -vcf needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    r = subprocess.run(base + ["-similar", "-simflank", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -similar needs the GPU library" in r.stderr, r.stderr[-2000:]  # (the library row stands before the range)
    # the usage refusals stand behind the help text
    for args, word in ((["-simflank", "100"], "Error: -simflank needs -similar."), (["-similar", "-gpus", "2"], "Error: -similar cannot be combined with -gpus."),
                       (["-simflank", "100", "-gpus", "2"], "Error: -simflank needs -similar.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-similar" in r.stderr and "-simflank" in r.stderr and "Error" not in r.stderr

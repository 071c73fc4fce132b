"""Known junctions without a GPU: the row layouts, the exports and the header's text; the two statements of the definition in
tests/knowncases.py on seeded small cases that reach every kind of hit and every tie rule; the hand example of the header; the BEDPE
reader with each kind of skipped, counted and fatal line; how the command line prints a row; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import knowncases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.KNOWN_ENTRY.itemsize == 40 and abi.KNOWN_SITE.itemsize == 24 and abi.KNOWN_CALL.itemsize == 40
    assert list(abi.KNOWN_ENTRY.names) == ["tid1", "beg1", "end1", "tid2", "beg2", "end2", "name", "score", "strand1", "strand2", "reserved"]
    assert [abi.KNOWN_ENTRY.fields[f][1] for f in abi.KNOWN_ENTRY.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 33, 34]
    assert abi.KNOWN_ENTRY.fields["score"][0] == np.dtype("<i4") and abi.KNOWN_ENTRY.fields["name"][0] == np.dtype("<u4")
    assert abi.KNOWN_SITE == abi.FRAME_SITE  # (as bk_frame_site)
    assert [abi.KNOWN_SITE.fields[f][1] for f in abi.KNOWN_SITE.names] == [0, 4, 8, 12, 16, 17, 18]
    assert list(abi.KNOWN_CALL.names) == ["n_hits", "n_oriented", "n_opposed", "n_names", "n_side", "best", "best_score", "best_dist", "best_crossed", "best_oriented", "reserved"]
    assert [abi.KNOWN_CALL.fields[f][1] for f in abi.KNOWN_CALL.names] == [0, 4, 8, 12, 16, 24, 28, 32, 36, 37, 38]
    assert abi.KNOWN_CALL.fields["n_side"][0] == np.dtype(("<u4", (2,))) and abi.KNOWN_CALL.fields["best"][0] == np.dtype("<i4")
    assert abi.KNOWN_MAX_SLOP == 1000000 and abi.KNOWN_NO_SCORE == -(1 << 31) and (abi.STRAND_NONE, abi.STRAND_LEFT, abi.STRAND_RIGHT) == (0, 1, 2)
    assert "bk_known_calls" in capi.EXPORTS and hasattr(capi.lib(), "bk_known_calls")
    assert hasattr(capi.Context, "known_calls")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert ("struct bk_known_entry { int32_t tid1; uint32_t beg1, end1; int32_t tid2; uint32_t beg2, end2; uint32_t name; int32_t score; uint8_t strand1, strand2; "
            "uint8_t reserved[6]; };") in header
    assert "struct bk_known_site  { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };" in header
    assert ("struct bk_known_call  { uint32_t n_hits, n_oriented, n_opposed, n_names, n_side[2]; int32_t best, best_score; uint32_t best_dist; uint8_t best_crossed, best_oriented; "
            "uint8_t reserved[2]; };") in header
    assert ("int bk_known_calls(bk_ctx *ctx, const struct bk_known_entry *entries, uint64_t n_entries, const struct bk_known_site *sites, uint64_t n, uint32_t slop, "
            "const struct bk_known_call **out);") in header
    for line in ("#define BK_KNOWN_MAX_SLOP 1000000u\n", "#define BK_KNOWN_NO_SCORE INT32_MIN\n", "#define BK_STRAND_NONE 0 ", "#define BK_STRAND_LEFT 1 ", "#define BK_STRAND_RIGHT 2 "):
        assert line in header, line
    assert "scope `known_calls`" in header and "`known_calls_index`" in header and "`known_calls_sites`" in header and "2^30 sites" in header
    assert "nothing is capped" in header and "spans a whole contig" in header


def both_hold(site, entry, slop):
    bk, iv = kc.breakends(site), kc.intervals(entry)
    return all(kc.falls(bk[s], iv[k], slop) is not None for s, k in ((0, 0), (1, 1), (0, 1), (1, 0)))


def test_the_two_statements_agree_and_reach_every_kind_of_hit():
    """48 seeded cases (up to 120 sites and 200 entries on 3 contigs of 50 000 bases, slop 0, 1, 20 and 100): both statements give the
    same bytes, and the cases hold what they are meant to hold"""
    rng = np.random.default_rng(26)
    seen = dict(straight=0, crossed=0, both=0, agree=0, oppose=0, unstated=0, by_score=0, by_dist=0, by_index=0, shared_names=0, side_above=0, no_hit=0, no_score_best=0)
    for case in range(48):
        slop = (0, 1, 20, 100)[case % 4]
        entries, sites = kc.random_case(rng, int(rng.integers(1, 121)), int(rng.integers(0, 201)), slop)
        a, b = kc.expected(entries, sites, slop), kc.expected_sorted(entries, sites, slop)
        assert a.tobytes() == b.tobytes(), (case, slop, np.flatnonzero(a != b)[:5])
        assert np.all(a["reserved"] == 0) and np.all(a["n_oriented"] + a["n_opposed"] <= a["n_hits"]) and np.all(a["n_names"] <= a["n_hits"])
        assert np.all((a["best"] >= 0) == (a["n_hits"] > 0)) and np.all(a["n_side"][:, 0] >= a["n_hits"]) and np.all(a["n_side"][:, 1] >= a["n_hits"])
        seen["shared_names"] += int((a["n_names"] < a["n_hits"]).sum())
        seen["side_above"] += int((a["n_side"].min(axis=1) > a["n_hits"]).sum())
        seen["no_hit"] += int((a["n_hits"] == 0).sum())
        seen["no_score_best"] += int(((a["best"] >= 0) & (a["best_score"] == kc.NO_SCORE)).sum())
        for i, site in enumerate(sites):
            hits = [(e, kc.hit_of(site, entries[e], slop)) for e in range(len(entries))]
            hits = [(e, h) for e, h in hits if h is not None]
            for e, h in hits:
                seen["crossed" if h[0] else "straight"] += 1
                seen["agree" if h[1] else "oppose" if h[2] else "unstated"] += 1
                seen["both"] += both_hold(site, entries[e], slop)
            if len(hits) > 1:
                top = max(int(entries[e]["score"]) for e, _ in hits)
                tied = [(e, h) for e, h in hits if int(entries[e]["score"]) == top]
                near = [e for e, h in tied if h[3] == min(h[3] for _, h in tied)]
                seen["by_score"] += len(tied) == 1
                seen["by_dist"] += len(tied) > 1 and len(near) == 1 and near[0] != tied[0][0]
                seen["by_index"] += len(near) > 1
                assert int(a[i]["best"]) == near[0]
    assert min(seen.values()) >= 10, seen


def hand_example():
    entries = kc.as_entries([(0, 299950, 300050, 1, 699900, 700100, 0, 12, kc.LEFT, kc.RIGHT), (1, 700050, 700060, 0, 299000, 299990, 1, 40, kc.RIGHT, kc.LEFT),
                             (0, 299990, 300010, 0, 100, 200, 0, kc.NO_SCORE, 0, 0), (1, 699000, 701000, 1, 699500, 700500, 2, kc.NO_SCORE, 0, 0)])
    return entries, kc.as_sites([(0, 300000, 0, 1, 700000, 1)])


def test_hand_example():
    """the header's: chr1 = 0, chr2 = 1, slop 100"""
    entries, sites = hand_example()
    site = sites[0]
    assert kc.hit_of(site, entries[0], 100) == (0, True, False, 0)
    assert kc.hit_of(site, entries[1], 100) == (1, True, False, 61)
    bk = kc.breakends(site)
    assert kc.falls(bk[1], kc.intervals(entries[1])[0], 100) == 51 and kc.falls(bk[0], kc.intervals(entries[1])[1], 100) == 10
    assert kc.hit_of(site, entries[2], 100) is None and kc.hit_of(site, entries[3], 100) is None
    a = kc.expected(entries, sites, 100)
    assert a.tobytes() == kc.expected_sorted(entries, sites, 100).tobytes()
    r = a[0]
    assert (int(r["n_hits"]), int(r["n_oriented"]), int(r["n_opposed"]), int(r["n_names"]), list(r["n_side"])) == (2, 2, 0, 2, [3, 3])
    assert (int(r["best"]), int(r["best_score"]), int(r["best_dist"]), int(r["best_crossed"]), int(r["best_oriented"])) == (1, 40, 61, 1, 1)
    # one base less of slop and e1 is no hit: its distance on chr2 is 51
    r = kc.expected(entries, sites, 50)[0]
    assert (int(r["n_hits"]), int(r["best"]), int(r["best_score"]), list(r["n_side"])) == (1, 0, 12, [3, 2])
    # the other side at breakend 0 and e0 opposes, e1 too
    flipped = kc.as_sites([(0, 300000, 1, 1, 700000, 1)])
    r = kc.expected(entries, flipped, 100)[0]
    assert (int(r["n_hits"]), int(r["n_oriented"]), int(r["n_opposed"]), int(r["best_oriented"])) == (2, 0, 2, 0)
    # without entries: the no-hit row
    r = kc.expected(entries[:0], sites, 100)[0]
    assert (int(r["n_hits"]), int(r["best"]), int(r["best_score"]), int(r["best_dist"]), list(r["n_side"])) == (0, -1, kc.NO_SCORE, 0, [0, 0])
    # dist at both ends of the range
    assert kc.dist(0, 0, 1) == 0 and kc.dist(-1, 0, 1) == 1 and kc.dist(0xFFFFFFFE, 0, 0xFFFFFFFF) == 0 and kc.dist(0xFFFFFFFE, 0, 1) == 0xFFFFFFFE
    assert kc.dist(5, 5, 6) == 0 and kc.dist(6, 5, 6) == 1 and kc.dist(4, 5, 6) == 1


CONTIGS = [("chr1", 1000), ("chr2", 2000), ("chr3", 500)]


def test_bedpe_reader():
    text = "\n".join([
        "# a comment", "track name=x", "browser position chr1:1-2", "", "   ",
        "chr1 10 20 chr2 30 40",                                  # six fields: name ".", no score, no strands
        "chr1\t10\t20\tchr2\t30\t40\tfusA\t7.9\t+\t-\textra\tcolumns",
        "chr2 5 9 chr1 1 2 fusB -3.99 - +",
        "chr1 10 20 chr2 30 40 fusA 1e3 * .",                    # a name again; strands that state nothing
        "chrX 10 20 chr2 30 40 fusC x + +",                      # a contig the header lacks: counted, the other interval stays
        ". -1 -1 chr3 1 2 . . . .",                              # '.' with the -1 of an unknown end: counted, no error
        "chr1 990 5000 chr2 2000 2100 fusD 99999999999 + +",     # clamped to the length; the second lies behind the contig's end
        "chr3 0 1 chr3 499 500 fusE nan + -",
        "chr3 0 1 chr3 499 500 fusE -inf + -",
        "chr3 0 1 chr3 499 500 fusE 12abc + -",
    ]) + "\n"
    entries, names, unknown = kc.read_bedpe(text, CONTIGS)
    assert names == [".", "fusA", "fusB", "fusC", "fusD", "fusE"] and unknown == 2 and len(entries) == 10
    rows = [tuple(int(e[f]) for f in ("tid1", "beg1", "end1", "tid2", "beg2", "end2", "name", "score", "strand1", "strand2")) for e in entries]
    N = kc.NO_SCORE
    assert rows == [(0, 10, 20, 1, 30, 40, 0, N, 0, 0), (0, 10, 20, 1, 30, 40, 1, 7, 1, 2), (1, 5, 9, 0, 1, 2, 2, -3, 2, 1), (0, 10, 20, 1, 30, 40, 1, 1000, 0, 0),
                    (-1, 0, 0, 1, 30, 40, 3, N, 1, 1), (-1, 0, 0, 2, 1, 2, 0, N, 0, 0), (0, 990, 1000, -1, 0, 0, 4, 2147483647, 1, 1),
                    (2, 0, 1, 2, 499, 500, 5, N, 1, 2), (2, 0, 1, 2, 499, 500, 5, -2147483648, 1, 2), (2, 0, 1, 2, 499, 500, 5, N, 1, 2)]
    assert np.all(entries["reserved"] == 0)
    for bad, line, why in (("chr1 10 20 chr2 30", 1, "fewer than six"), ("#c\nchr1 10 20 chr2 30 4x", 2, "not a number"), ("chr1 1.5 20 chr2 30 40", 1, "not a number"),
                           ("chrX 10 b chr2 30 40", 1, "not a number"), ("\n\nchr1 -1 20 chr2 30 40", 3, "negative"), ("chr1 10 20 chr2 40 40", 1, "end <= start"),
                           ("chr1 10 20 chr2 40 30", 1, "end <= start")):
        with pytest.raises(kc.BedpeError) as e:
            kc.read_bedpe(bad, CONTIGS)
        assert e.value.line == line and why in e.value.why, bad
    assert kc.read_bedpe("", CONTIGS)[1:] == ([], 0) and len(kc.read_bedpe("chrX 9 3 chrY -5 -7\n", CONTIGS)[0]) == 1
    for text, score in (("7", 7), ("-7.99", -7), ("+.5e1", 5), ("0x10", 16), ("1e99", 2147483647), ("-1e99", -2147483648), ("inf", 2147483647), ("", N), (".", N), ("1,5", N), ("e5", N)):
        assert kc.score_of(text) == score, text


def test_printed_fields():
    entries, sites = hand_example()
    names = ["pon", "COSF1", "other"]
    r = kc.expected(entries, sites, 100)[0]
    assert kc.call_fields(r, entries, names) == ["2", "2", "2", "0", "COSF1", "40", "61", "crossed", "3", "3"]
    assert len(kc.KNOWN_COLUMNS) == 10 and kc.info_fields(r, entries, names) == ";KNOWN=2;KNAMES=2;KBEST=COSF1"
    r = kc.expected(entries, sites, 50)[0]
    assert kc.call_fields(r, entries, names) == ["1", "1", "1", "0", "pon", "12", "0", "straight", "3", "2"]
    r = kc.expected(entries[2:], sites, 100)[0]
    assert kc.call_fields(r, entries[2:], names) == ["0", "0", "0", "0", ".", ".", "0", ".", "1", "1"] and kc.info_fields(r, entries[2:], names) == ";KNOWN=0;KNAMES=0"
    noscore = entries[:1].copy()
    noscore["score"] = kc.NO_SCORE
    r = kc.expected(noscore, sites, 100)[0]
    assert kc.call_fields(r, noscore, ["a name;x=1"])[4:6] == ["a name;x=1", "."] and kc.info_fields(r, noscore, ["a name;x=1"]).endswith(";KBEST=a_name_x_1")
    assert kc.bedpe_line("chr1", 300000, "chr2", 700000, "run7", 12, 5, "+", "-", 3, "Translocation") == \
        "chr1\t299999\t300000\tchr2\t699999\t700000\trun7\t17\t+\t-\tbk3\tTranslocation\t12\t5"
    assert [kc.strand_text(r, s) for r, s in ((0, 2), (1, 1), (0, 0), (1, 0))] == ["+", "-", ".", "."]
    # a line of -bedpe read back is an entry that holds its own call at slop 0, straight, agreeing
    back, names, unknown = kc.read_bedpe(kc.bedpe_line("chr1", 300, "chr2", 700, "run7", 12, 5, "+", "-", 3, "Translocation") + "\n", CONTIGS)
    assert kc.hit_of(kc.as_sites([(0, 300, 0, 1, 700, 1)])[0], back[0], 0) == (0, True, False, 0) and names == ["run7"] and int(back[0]["score"]) == 17
    # the byte model: four entries on tids 0 and 1 (34 key bits, 5 passes), 8 intervals; one site (no site bits), names up to 2 (1 pass)
    assert kc.touched(entries, sites, 2) == (4 * (64 + 48 * 5) + 16 * 8, 80 + 2 * (12 + 24), 4 * (64 + 48 * 5) + 16 * 8 + 80 + 2 * 36)
    assert kc.touched(entries[:0], sites, 0) == (0, 80, 80)
    lone = kc.as_entries([(-1, 0, 0, -1, 0, 0, 0x10000, 0, 0, 0)])
    assert kc.touched(lone, kc.as_sites([(0, 5, 0, 0, 9, 1)] * 257), 3) == (64, 257 * 80 + 3 * (12 + 24 * (3 + 2)), 64 + 257 * 80 + 3 * 132)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_known(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    panel = tmp_path / "panel.bedpe"
    panel.write_text("chr1 1 2 chr2 3 4\n")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for args, option in ((["-known", str(panel)], "-known"), (["-known", str(panel), "-knownslop", "0", "-all", "-fast"], "-known"), (["-bedpe"], "-bedpe"),
                         (["-known", str(tmp_path / "missing"), "-bedpe"], "-known"), (["-bedpe", "-known", str(panel), "-fragsize"], "-fragsize")):  # (an earlier row of the table)
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: %s needs the GPU library" % option in r.stderr and "Usage" not in r.stderr, (args, r.stderr[-2000:])
    # the usage refusals stand behind the help text, in the order of the table: the new rows behind every older row
    for args, word in ((["-knownslop", "5"], "Error: -knownslop needs -known."), (["-known", str(panel), "-gpus", "2"], "Error: -known cannot be combined with -gpus."),
                       (["-known", str(panel), "-knownslop", "1000001"], "Error: -knownslop must be a number from 0 to 1000000."),
                       (["-known", str(panel), "-knownslop", "-1"], "Error: -knownslop must be a number from 0 to 1000000."),
                       (["-known", str(panel), "-gpus", "2", "-knownslop", "1000001"], "Error: -known cannot be combined with -gpus."),
                       (["-bedpe", "-gpus", "2"], "Error: -bedpe cannot be combined with -gpus."),
                       (["-bedpe", "-knownslop", "5", "-gpus", "2"], "Error: -knownslop needs -known."),
                       (["-known", str(panel), "-linkdist", "100"], "Error: -linkdist needs -link."),
                       (["-known", str(panel), "-gpus", "2", "-fragsize"], "Error: -fragsize cannot be combined with -gpus.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-known " in r.stderr and "-knownslop" in r.stderr and "-bedpe " in r.stderr and "KBEST" in r.stderr and "Error" not in r.stderr

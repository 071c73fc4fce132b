"""Linked calls without a GPU: the row layouts, the exports and the header's text; the two statements of the definition in
tests/linkcases.py (every pair of sites against the sorted runs) on seeded small cases that reach every relation and every tie rule of
the mate; the hand example of the header; how the command line prints a row; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import linkcases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.LINK_SITE.itemsize == 24 and abi.CALL_LINK.itemsize == 40
    assert list(abi.LINK_SITE.names) == ["tid1", "pos1", "tid2", "pos2", "right1", "right2", "reserved"]
    assert [abi.LINK_SITE.fields[f][1] for f in abi.LINK_SITE.names] == [0, 4, 8, 12, 16, 17, 18]
    assert abi.LINK_SITE == abi.FRAME_SITE  # (as bk_frame_site)
    assert list(abi.CALL_LINK.names) == ["n_dup", "n_recip", "n_adj", "dup_of", "mate", "off", "event", "event_size", "mate_crossed", "reserved"]
    assert [abi.CALL_LINK.fields[f][1] for f in abi.CALL_LINK.names] == [0, 4, 8, 12, 16, 20, 28, 32, 36, 37]
    assert abi.CALL_LINK.fields["off"][0] == np.dtype(("<i4", (2,))) and abi.CALL_LINK.fields["dup_of"][0] == np.dtype("<i4")
    assert abi.LINK_RELATIONS == ["none", "duplicate", "reciprocal", "adjacent"] and abi.LINK_MAX_DIST == 1000000
    assert "bk_link_calls" in capi.EXPORTS and hasattr(capi.lib(), "bk_link_calls")
    assert hasattr(capi.Context, "link_calls")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_link_site { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };" in header
    assert ("struct bk_call_link { uint32_t n_dup, n_recip, n_adj; int32_t dup_of, mate; int32_t off[2]; uint32_t event, event_size; uint8_t mate_crossed; "
            "uint8_t reserved[3]; };") in header
    assert "int bk_link_calls(bk_ctx *ctx, const struct bk_link_site *sites, uint64_t n, uint32_t max_dist, const struct bk_call_link **out);" in header
    for k, name in enumerate(abi.LINK_RELATIONS):
        assert "#define BK_LINK_%s %d\n" % (name.upper(), k) in header
    assert "#define BK_LINK_MAX_DIST %du\n" % abi.LINK_MAX_DIST in header
    assert "scope `link_calls`" in header and "2^30 sites" in header and "blunt break" in header and "(0,0) (0,1) (1,0)" in header


def mate_rules(sites, res, D):
    """which of the mate's tie rules decided at some site: [two partners with the smallest sum, one partner with both mappings opposite
    and different sums, one partner with both mappings opposite and the same sum]"""
    seen = [0, 0, 0]
    for i in np.flatnonzero(res["mate"] >= 0):
        cands = lc.mate_candidates(sites, int(i), D)
        best = min(c[0] for c in cands)
        seen[0] += len({c[1] for c in cands if c[0] == best}) > 1
        own = [c for c in cands if c[1] == int(res[i]["mate"])]
        seen[1] += len(own) == 2 and own[0][0] != own[1][0]
        seen[2] += len(own) == 2 and own[0][0] == own[1][0]
    return seen


def test_the_two_statements_agree_and_reach_every_relation():
    """40 seeded cases (up to 300 sites on 3 contigs of 50 000 bases, D = 0, 1, 100 and 1000): both statements give the same bytes,
    every relation occurs, as do a mate by each of its tie rules, a crossed mate, duplicates whose dup_of is a later row, events of
    more than two sites and sites alone"""
    rng = np.random.default_rng(23)
    rel, rules, crossed, later, big, alone = [0] * 4, [0] * 3, 0, 0, 0, 0
    for case in range(40):
        D = (0, 1, 100, 1000)[case % 4]
        n = int(rng.integers(2, 301))
        sites = lc.random_sites(rng, n, D=max(D, 1))
        a, b = lc.expected(sites, D), lc.expected_runs(sites, D)
        assert a.tobytes() == b.tobytes(), (case, D, np.flatnonzero(a != b)[:5])
        for k, name in enumerate(("n_dup", "n_recip", "n_adj")):
            rel[k + 1] += int(a[name].sum())
        rel[0] += n * (n - 1) - int(a["n_dup"].sum() + a["n_recip"].sum() + a["n_adj"].sum())
        for i, s in enumerate(mate_rules(sites, a, D)):
            rules[i] += s
        crossed += int(a["mate_crossed"].sum())
        later += int((a["dup_of"] > np.arange(n)).sum())
        big += int((a["event_size"] > 2).sum())
        alone += int((a["event_size"] == 1).sum())
        assert np.all(a["event"] <= np.arange(n)) and np.all((a["event_size"] == 1) == (a["n_dup"] + a["n_recip"] + a["n_adj"] == 0))
        assert np.all(a["reserved"] == 0) and np.all((a["mate"] >= 0) == (a["n_recip"] > 0))
        # symmetric: what i counts, its partners count back
        for i in range(0, n, 17):
            for j in range(n):
                assert lc.relation(sites, i, j, D) == lc.relation(sites, j, i, D)
    assert min(rel) >= 50 and min(rules) >= 3 and crossed >= 20 and later >= 20 and big >= 50 and alone >= 50, (rel, rules, crossed, later, big, alone)


def test_hand_example():
    """the header's: chr1 = 0, chr2 = 1, chr3 = 2, D = 1000"""
    two = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0)])
    assert lc.relation(two, 0, 1, 1000) == lc.RECIPROCAL
    a = lc.expected(two, 1000)
    assert (int(a[0]["mate"]), list(a[0]["off"]), int(a[0]["event"]), int(a[0]["event_size"]), int(a[0]["mate_crossed"])) == (1, [21, -10], 0, 2, 0)
    assert (int(a[1]["mate"]), list(a[1]["off"]), int(a[1]["event"]), int(a[1]["n_recip"])) == (0, [-21, 10], 0, 1)
    three = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0), (1, 700400, 0, 2, 5000, 1)])
    assert [lc.relation(three, 2, j, 1000) for j in (0, 1)] == [lc.ADJACENT, lc.ADJACENT]
    a = lc.expected(three, 1000)
    assert a.tobytes() == lc.expected_runs(three, 1000).tobytes()
    assert list(a["event_size"]) == [3, 3, 3] and list(a["event"]) == [0, 0, 0] and list(a["n_adj"]) == [1, 1, 2] and list(a["mate"]) == [1, 0, -1]
    # the same junction the other way round is the crossed mapping of the same partner
    swapped = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (1, 699990, 0, 0, 300021, 1)])
    a = lc.expected(swapped, 1000)
    assert (int(a[0]["mate"]), int(a[0]["mate_crossed"]), list(a[0]["off"])) == (1, 1, [21, -10])
    assert (int(a[1]["mate"]), int(a[1]["mate_crossed"]), list(a[1]["off"])) == (0, 1, [10, -21])
    # a 300-base deletion is not its own partner; called twice it is a duplicate; D = 0 needs exact coincidence
    a = lc.expected(lc.as_sites([(0, 5000, 0, 0, 5300, 1)]), 1000)
    assert (int(a[0]["n_dup"]), int(a[0]["n_recip"]), int(a[0]["n_adj"]), int(a[0]["event_size"]), int(a[0]["dup_of"]), int(a[0]["mate"])) == (0, 0, 0, 1, -1, -1)
    twice = lc.as_sites([(0, 5000, 0, 0, 5300, 1), (0, 5003, 0, 0, 5300, 1)])
    assert lc.relation(twice, 0, 1, 1000) == lc.DUPLICATE and lc.relation(twice, 0, 1, 0) == lc.ADJACENT and lc.relation(twice, 0, 1, 2) == lc.ADJACENT
    assert lc.relation(twice, 0, 1, 3) == lc.DUPLICATE
    a = lc.expected(twice, 1000)
    assert list(a["dup_of"]) == [1, 0] and list(a["n_dup"]) == [1, 1] and list(a["event"]) == [0, 0]


def test_printed_fields():
    three = lc.as_sites([(0, 300000, 0, 1, 700000, 1), (0, 300021, 1, 1, 699990, 0), (1, 700400, 0, 2, 5000, 1), (2, 90, 0, 2, 900, 1), (2, 91, 0, 2, 901, 1)])
    a = lc.expected(three, 1000)
    rows = [7, 4, 9, 12, 30]  # the BK_STAGE_CLUSTERS rows of the five sites
    assert lc.call_fields(a[0], rows) == ["ev7", "3", "0", "1", "1", ".", "bk4", "straight", "21", "-10"]
    assert lc.call_fields(a[2], rows) == ["ev7", "3", "0", "0", "2", ".", ".", ".", ".", "."]
    assert lc.call_fields(a[3], rows) == ["ev12", "2", "1", "0", "0", "bk30", ".", ".", ".", "."]
    assert len(lc.LINK_COLUMNS) == len(lc.call_fields(a[0], rows))
    everywhere, nowhere = (lambda row: True), (lambda row: False)
    assert lc.info_fields(a[0], rows, 0, everywhere) == ";EVENT=ev7;PARID=bk4_1" and lc.info_fields(a[0], rows, 1, everywhere) == ";EVENT=ev7;PARID=bk4_2"
    assert lc.info_fields(a[0], rows, 0, nowhere) == ";EVENT=ev7" and lc.info_fields(a[2], rows, 1, everywhere) == ";EVENT=ev7"
    swapped = lc.expected(lc.as_sites([(0, 300000, 0, 1, 700000, 1), (1, 699990, 0, 0, 300021, 1)]), 1000)
    assert lc.info_fields(swapped[0], [3, 5], 0, everywhere) == ";EVENT=ev3;PARID=bk5_2" and lc.info_fields(swapped[0], [3, 5], 1, everywhere) == ";EVENT=ev3;PARID=bk5_1"
    assert lc.info_fields(lc.expected(three[3:4], 1000)[0], [12], 0, everywhere) == ""
    assert lc.touched(three) == 5 * 64 + 10 * (24 + 24 * 5) and lc.touched(lc.as_sites([(-1, 5, 0, -1, 9, 1)])) == 64


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_link(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-link"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -link needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-link", "-linkdist", "0", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -link needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-link", "-frame"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -frame needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    # the usage refusals stand behind the help text, in the order of the table: -link's own behind every older row
    for args, word in ((["-linkdist", "5"], "Error: -linkdist needs -link."), (["-link", "-gpus", "2"], "Error: -link cannot be combined with -gpus."),
                       (["-link", "-linkdist", "1000001"], "Error: -linkdist must be a number from 0 to 1000000."),
                       (["-link", "-linkdist", "-1"], "Error: -linkdist must be a number from 0 to 1000000."),
                       (["-link", "-gpus", "2", "-linkdist", "1000001"], "Error: -link cannot be combined with -gpus."),
                       (["-link", "-covflank", "100"], "Error: -covflank needs -coverage."), (["-link", "-gpus", "2", "-frame"], "Error: -frame cannot be combined with -gpus.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-link " in r.stderr and "-linkdist" in r.stderr and "PARID" in r.stderr and "Error" not in r.stderr

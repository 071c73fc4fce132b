"""Partner loci without a GPU: the row layouts, the exports and the header's text; the two statements of the definition in
tests/partnercases.py (a brute-force pass per site against the sorted index and the sorted runs) on seeded small cases that reach every
branch; the hand example of the header; the rule of bk_call_partner_sites; how the command line prints a call; the byte model; and the
CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import partnercases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
NAMES = ["chr1", "chr2", "chr3"]


def test_row_layouts_and_exports():
    assert abi.PARTNER_SITE.itemsize == 32 and abi.LOCUS_PARTNERS.itemsize == 32
    assert list(abi.PARTNER_SITE.names) == ["tid", "beg", "end", "mtid", "mbeg", "mend", "reserved"]
    assert [abi.PARTNER_SITE.fields[f][1] for f in abi.PARTNER_SITE.names] == [0, 4, 8, 12, 16, 20, 24]
    assert abi.PARTNER_SITE.fields["tid"][0] == np.dtype("<i4") and abi.PARTNER_SITE.fields["mtid"][0] == np.dtype("<i4")
    assert abi.PARTNER_SITE.fields["reserved"][0] == np.dtype(("<u4", (2,)))
    assert list(abi.LOCUS_PARTNERS.names) == ["ends", "to_partner", "loci", "top_n", "top_tid", "top_beg", "top_end", "reserved"]
    assert [abi.LOCUS_PARTNERS.fields[f][1] for f in abi.LOCUS_PARTNERS.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert abi.LOCUS_PARTNERS.fields["top_tid"][0] == np.dtype("<i4") and abi.LOCUS_PARTNERS.fields["top_n"][0] == np.dtype("<u4")
    for name in ("bk_locus_partners", "bk_call_partner_sites"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert hasattr(capi.Context, "locus_partners") and hasattr(capi, "call_partner_sites")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert ("struct bk_partner_site { int32_t tid; uint32_t beg, end; int32_t mtid; uint32_t mbeg, mend; uint32_t reserved[2]; };   "
            "/* 32 bytes; 1-based, inclusive; reserved = 0 */") in header
    assert "struct bk_locus_partners { uint32_t ends, to_partner, loci, top_n; int32_t top_tid; uint32_t top_beg, top_end, reserved; }; /* 32 bytes */" in header
    assert "int bk_locus_partners(bk_ctx *ctx, const struct bk_partner_site *sites, uint64_t n, uint32_t max_gap, const struct bk_locus_partners **out);" in header
    assert "int bk_call_partner_sites(const bk_cluster *c, double w, struct bk_partner_site out[2]);   /* pure host function */" in header
    for words in ("All arithmetic is signed 64-bit", "tid -1 sorts first", "a tie goes to the first in sorted order", 'top_n == 0 is the "none" signal',
                  "chr3:9000, 9100, 9500", "(0, 800, 1300 | 1, 4800, 5300)", "(1, 4800, 5300 | 0, 800, 1300)", "chr3:9000-9100", "chr3:9000-9500",
                  "scope `locus_partners`", "`locus_partners_index`", "`locus_partners_sites`", "2^30 sites", "2^32 - 16 rows", "[max(1, ps_min - W), ps_max + W]",
                  "56 bytes per pair row", "12 bytes per end of the index", "64 bytes per site", "12 bytes per elsewhere row"):
        assert words in header, words


def test_the_two_statements_agree_and_reach_every_branch():
    """40 seeded cases (up to 2000 pairs on 3 contigs of 50 000 bases, max_gap = 0, 1, 100 and 0xFFFFFFFF): both statements give the same
    bytes, and the cases reach every branch at least 20 times"""
    rng = np.random.default_rng(24)
    seen, rows_total = {}, 0
    for case in range(40):
        gap = (0, 1, 100, pc.U32)[case % 4]
        pairs, sites = pc.random_case(rng, gap)
        assert len(pairs) <= 2000
        a = pc.expected(pairs, sites, gap, 3)
        b, n_rows = pc.expected_runs(pairs, sites, gap, 3, with_rows=True)
        assert a.tobytes() == b.tobytes(), (case, gap, [(k, a[k], b[k]) for k in range(len(a)) if a[k] != b[k]][:3])
        assert n_rows == int(a["ends"].astype(np.int64).sum() - a["to_partner"].astype(np.int64).sum())
        rows_total += n_rows
        assert np.all(a["reserved"] == 0) and np.all(a["to_partner"] <= a["ends"]) and np.all(a["top_n"] <= a["ends"] - a["to_partner"])
        assert np.all((a["top_n"] == 0) == (a["loci"] == 0)) and np.all((a["top_n"] == 0) == (a["ends"] == a["to_partner"]))
        none = a[a["top_n"] == 0]
        assert np.all(none["top_tid"] == -1) and np.all(none["top_beg"] == 0) and np.all(none["top_end"] == 0)
        assert int(a[-1]["ends"]) == int((pairs["p1_tid"] == 0).sum() + (pairs["p2_tid"] == 0).sum())  # the whole of contig 0
        for name, n in pc.branches(pairs, sites, gap, 3).items():
            seen[name] = seen.get(name, 0) + int(n)
    assert min(seen.values()) >= 20 and rows_total > 10_000, (seen, rows_total)


@pytest.mark.parametrize("gap,loci,top,top_n", [(200, 4, (2, 9000, 9100), 2), (399, 4, (2, 9000, 9100), 2), (400, 3, (2, 9000, 9500), 3)])
def test_hand_example(gap, loci, top, top_n):
    """the header's: chr1 = 0, chr2 = 1, chr3 = 2, ten pairs"""
    pairs = pc.as_pairs(pc.HAND_PAIRS)
    site = pc.HAND_SITE
    sites = pc.as_sites([site, site[3:] + site[:3]])
    a = pc.expected(pairs, sites, gap, 3)
    assert a.tobytes() == pc.expected_runs(pairs, sites, gap, 3).tobytes()
    assert (int(a[0]["ends"]), int(a[0]["to_partner"]), int(a[0]["loci"]), int(a[0]["top_n"])) == (10, 5, loci, top_n)
    assert (int(a[0]["top_tid"]), int(a[0]["top_beg"]), int(a[0]["top_end"])) == top
    assert (int(a[1]["ends"]), int(a[1]["to_partner"]), int(a[1]["loci"]), int(a[1]["top_n"]), int(a[1]["top_tid"])) == (5, 5, 0, 0, -1)
    _, _, mates = pc.elsewhere_of(pairs, sites[0], 3)
    assert mates == [(0, 80000), (1, 5600), (2, 9000), (2, 9100), (2, 9500)]
    # the other way round, the pairs given as (p2 -> p1): the ends are the same
    swapped = pc.as_pairs([(t2, p2, t1, p1) for t1, p1, t2, p2 in pc.HAND_PAIRS])
    assert pc.expected(swapped, sites, gap, 3).tobytes() == a.tobytes()


def test_definition_edges():
    pairs = pc.as_pairs([(0, 100, 1, 500), (0, 100, 1, 500), (0, 101, -1, 0), (0, 102, -1, 7), (0, 103, 0, 100), (0, 104, 2, 50), (0, 105, 2, 60)])
    # T < 0, T >= n_targets, b < a: zero rows; MT < 0 and mb < ma: nobody goes to the partner, even the unmapped mates
    sites = pc.as_sites([(-1, 1, 200, 1, 1, 900), (3, 1, 200, 1, 1, 900), (0, 200, 100, 1, 1, 900), (0, 100, 105, -1, 0, 900), (0, 100, 105, 1, 900, 1)])
    a = pc.expected(pairs, sites, 5, 3)
    assert a.tobytes() == pc.expected_runs(pairs, sites, 5, 3).tobytes()
    for k in range(3):
        assert a[k].tobytes() == pc.none_row().tobytes()
    # the pair chr1:103 -> chr1:100 has both ends in the window: eight ends.  tid -1 sorts first; (-1, 0) and (-1, 7) are 7 apart: two
    # loci at gap 5.  chr1:100-103 and chr2:500-500 have two mates each: the tie goes to chr1, the first in sorted order
    assert [int(a[3][f]) for f in ("ends", "to_partner", "loci", "top_n", "top_tid", "top_beg", "top_end")] == [8, 0, 6, 2, 0, 100, 103]
    assert a[4].tobytes() == a[3].tobytes()
    # an end elsewhere whose mate lies inside the site's own window (0, 103 -> 0, 100) is a locus; its other end (0, 100 -> 0, 103) too
    b = pc.expected(pairs, pc.as_sites([(0, 100, 105, 1, 1, 900)]), 10, 3)
    assert [int(b[0][f]) for f in ("ends", "to_partner", "loci", "top_n", "top_tid", "top_beg", "top_end")] == [8, 2, 3, 2, -1, 0, 7]
    # a tie goes to the first in sorted order: at gap 10 (-1: 0-7), (0: 100-103) and (2: 50-60) have two each
    c = pc.expected(pairs[2:], pc.as_sites([(0, 100, 105, 1, 1, 900)]), 10, 3)
    assert [int(c[0][f]) for f in ("loci", "top_n", "top_tid")] == [3, 2, -1]
    # max_gap = 0xFFFFFFFF joins a whole contig and never another
    d = pc.expected(pairs, pc.as_sites([(0, 100, 105, -1, 0, 0)]), pc.U32, 3)
    assert [int(d[0][f]) for f in ("loci", "top_n", "top_tid", "top_beg", "top_end")] == [4, 2, -1, 0, 7]
    assert pc.expected_runs(pairs, pc.as_sites([(0, 100, 105, -1, 0, 0)]), pc.U32, 3).tobytes() == d.tobytes()


def cluster(**fields):
    c = np.zeros(1, abi.CLUSTER)[0]
    for k, v in fields.items():
        c[k] = v
    return c


def test_call_partner_sites_rule():
    """bk_call_partner_sites against its Python mirror: a plain call across two contigs, ps_min <= W (the clamp to 1), and the upper end
    of the range"""
    plain = cluster(p1_tid=0, p1_min=300_000, p1_max=300_250, p2_tid=1, p2_min=700_000, p2_max=700_300)
    got = capi.call_partner_sites(plain, 1234.9)
    assert got.tobytes() == pc.call_sites(plain, 1234.9).tobytes()
    assert [tuple(int(got[s][f]) for f in ("tid", "beg", "end", "mtid", "mbeg", "mend")) for s in (0, 1)] == \
        [(0, 298_766, 301_484, 1, 698_766, 701_534), (1, 698_766, 701_534, 0, 298_766, 301_484)]
    assert np.all(got["reserved"] == 0)
    for lo in (1, 900, 1000, 1001):  # W = 1000: ps_min - W is -999, -100, 0 and 1
        c = cluster(p1_tid=2, p1_min=lo, p1_max=lo + 40, p2_tid=2, p2_min=5000, p2_max=5100)
        got = capi.call_partner_sites(c, 1000.5)
        assert got.tobytes() == pc.call_sites(c, 1000.5).tobytes()
        assert (int(got[0]["beg"]), int(got[0]["end"]), int(got[1]["mbeg"]), int(got[1]["mend"])) == (1, lo + 1040, 1, lo + 1040)
        assert (int(got[1]["tid"]), int(got[1]["beg"]), int(got[1]["end"])) == (2, 4000, 6100)
    top = cluster(p1_tid=0, p1_min=pc.U32 - 5, p1_max=pc.U32, p2_tid=-1, p2_min=10, p2_max=20)
    got = capi.call_partner_sites(top, 100.0)
    assert got.tobytes() == pc.call_sites(top, 100.0).tobytes()
    assert (int(got[0]["beg"]), int(got[0]["end"]), int(got[0]["mtid"]), int(got[1]["tid"])) == (pc.U32 - 105, pc.U32, -1, -1)
    assert capi.lib().bk_call_partner_sites(None, 5.0, got.ctypes.data) == abi.BK_ERR_ARG
    c = np.zeros(1, abi.CLUSTER)
    assert capi.lib().bk_call_partner_sites(c.ctypes.data, 5.0, None) == abi.BK_ERR_ARG


def test_printed_fields():
    pairs = pc.as_pairs(pc.HAND_PAIRS + [(0, 1210, -1, 0), (0, 1211, -1, 3), (0, 1212, -1, 5)])
    site = pc.HAND_SITE
    two = pc.expected(pairs, pc.as_sites([site, site[3:] + site[:3]]), 200, 3)
    assert pc.call_fields(two, NAMES) == ["13", "5", "5", "*:0-5", "3", "5", "5", "0", ".", "0", "0.556"]
    assert len(pc.call_fields(two, NAMES)) == len(pc.PARTNER_NAMES) == 11
    two = pc.expected(pc.as_pairs(pc.HAND_PAIRS), pc.as_sites([site, site[3:] + site[:3]]), 400, 3)
    assert pc.call_fields(two, NAMES) == ["10", "5", "3", "chr3:9000-9500", "3", "5", "5", "0", ".", "0", "0.667"]
    assert pc.info_fields(two[0]) == ";PTN=10;PTP=5;PTL=3" and pc.info_fields(two[1]) == ";PTN=5;PTP=5;PTL=0"
    none = pc.expected(pc.as_pairs([]), pc.as_sites([site, site]), 400, 3)
    assert pc.call_fields(none, NAMES) == ["0", "0", "0", ".", "0", "0", "0", "0", ".", "0", "."]
    one = pc.expected(pc.as_pairs([(0, 900, 1, 5000), (0, 901, 2, 7), (0, 902, 2, 8)]), pc.as_sites([site, site[3:] + site[:3]]), 1, 3)
    assert pc.call_fields(one, NAMES)[-1] == "0.500" and pc.call_fields(one, NAMES)[3] == "chr3:7-8"


def test_byte_model():
    """the pair rows read, 12 bytes per end of the index, 64 bytes per site, 12 bytes per elsewhere row per sort pass"""
    # 3 contigs: the mate key has 32 + 3 bits, five passes; up to 256 sites one more, up to 65 536 two
    assert [pc.row_passes(3, n) for n in (0, 1, 2, 256, 257, 65_536, 65_537)] == [5, 5, 6, 6, 7, 7, 8]
    assert [pc.row_passes(nt, 1) for nt in (0, 1, 2, 3, 254, 255, 65_534, 65_535)] == [5, 5, 5, 5, 5, 6, 6, 7]
    assert pc.touched(10, 3, 2, 5) == 10 * 56 + 20 * 12 + 2 * 64 + 5 * 12 * 6 == pc.touched_index(10) + pc.touched_sites(3, 2, 5)
    assert pc.touched(0, 3, 0, 0) == 0 and pc.touched(0, 3, 4, 0) == 256


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_partners(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-partners"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -partners needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-partners", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -partners needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-partners", "-link"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -link needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    # the usage refusals stand behind the help text, in the order of the table: -partners' own behind every older row
    for args, word in ((["-partners", "-gpus", "2"], "Error: -partners cannot be combined with -gpus."),
                       (["-partners", "-linkdist", "5"], "Error: -linkdist needs -link."),
                       (["-partners", "-gpus", "2", "-link"], "Error: -link cannot be combined with -gpus."),
                       (["-partners", "-link", "-linkdist", "1000001"], "Error: -linkdist must be a number from 0 to 1000000."),
                       (["-partners", "-covflank", "100"], "Error: -covflank needs -coverage.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-partners " in r.stderr and "PTN / PTP / PTL" in r.stderr and "Error" not in r.stderr

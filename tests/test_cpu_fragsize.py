"""Fragment sizes without a GPU: the row layouts, the exports and the header's text; the two statements of the definition in
tests/fragcases.py (a linear scan per row against the lexsorted table) on seeded small cases that reach every branch; the hand example of
the header; bk_fragment_bounds; how the command line prints a call; and the CPU build's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import fragcases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.FRAG_SITE.itemsize == 16 and abi.FRAG_SIZES.itemsize == 48
    assert list(abi.FRAG_SITE.names) == ["pos1", "pos2", "right1", "right2", "skip", "reserved"]
    assert [abi.FRAG_SITE.fields[f][1] for f in abi.FRAG_SITE.names] == [0, 4, 8, 9, 10, 11]
    assert abi.FRAG_SITE.fields["reserved"][0] == np.dtype(("u1", (5,))) and abi.FRAG_SITE.fields["pos1"][0] == np.dtype("<u4")
    assert list(abi.FRAG_SIZES.names) == ["n_used", "n_off", "n_lost", "n_short", "n_long", "min", "max", "reserved", "sum", "abs_dev"]
    assert [abi.FRAG_SIZES.fields[f][1] for f in abi.FRAG_SIZES.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert abi.FRAG_SIZES.fields["min"][0] == np.dtype("<i4") and abi.FRAG_SIZES.fields["sum"][0] == np.dtype("<i8") and abi.FRAG_SIZES.fields["abs_dev"][0] == np.dtype("<u8")
    for name in ("bk_fragment_sizes", "bk_fragment_bounds"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert hasattr(capi.Context, "fragment_sizes") and hasattr(capi, "fragment_bounds")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert ("struct bk_frag_site  { uint32_t pos1, pos2; uint8_t right1, right2, skip; uint8_t reserved[5]; };   "
            "/* 16 bytes; pos 1-based; reserved = 0 */") in header
    assert ("struct bk_frag_sizes { uint32_t n_used, n_off, n_lost, n_short, n_long; int32_t min, max; uint32_t reserved; int64_t sum; uint64_t abs_dev; };  "
            "/* 48 bytes */") in header
    assert "int bk_fragment_sizes(bk_ctx *ctx, const struct bk_frag_site *sites, uint64_t n, int32_t lo, int32_t hi, const struct bk_frag_sizes **out);" in header
    assert "int bk_fragment_bounds(double mean, double sd, int32_t *lo, int32_t *hi);   /* pure host function */" in header
    for words in ("All arithmetic is signed 64-bit", "n must equal the number of BK_STAGE_CLUSTERS rows", "skip != 0 gives an all-zero row",
                  "((F_s & 0x10) != 0) != (right_s != 0)", "An off row is never looked up", "the smallest index i", "lost and counted, never guessed",
                  "a_s = site.pos_s - P_s + 1", "a_s = E_s - site.pos_s + 1", "clamped to [-2^31 + 1, 2^31 - 1]", "floor((2 sum + n_used) / (2 n_used))",
                  "n_used + n_off + n_lost equals the call's pair rows", "soft-clipped bases are not added back", "scope `fragment_sizes`",
                  "lo = max(0, floor(mean - 3 sd)), hi = ceil(mean + 3 sd)", "centre = floor(1729 / 6) = 288", "abs_dev = 113 + 23 + 137 = 273",
                  "(120 bytes)", "(80 bytes)", "(18 bytes)", "(8 bytes)"):
        assert words in header, words


def test_the_two_statements_agree_and_reach_every_branch():
    """40 seeded cases: both statements give the same bytes, the counts add up, and the cases reach every branch at least 20 times"""
    rng = np.random.default_rng(25)
    seen = {}
    for case in range(40):
        ev, off, cols, sites, lo, hi = fc.random_case(rng)
        a = fc.expected(ev, off, cols, sites, lo, hi)
        b = fc.expected_sorted(ev, off, cols, sites, lo, hi)
        assert a.tobytes() == b.tobytes(), (case, [(k, a[k], b[k]) for k in range(len(a)) if a[k] != b[k]][:3])
        n_pair = np.asarray([int((ev["kind"][int(off[c]):int(off[c + 1])] == abi.EV_PAIR).sum()) for c in range(len(sites))])
        total = a["n_used"].astype(np.int64) + a["n_off"] + a["n_lost"]
        assert np.all(total[sites["skip"] == 0] == n_pair[sites["skip"] == 0]) and np.all(total[sites["skip"] != 0] == 0)
        assert np.all(a["reserved"] == 0) and np.all(a["min"] <= a["max"]) and np.all(a["n_short"] + a["n_long"] <= a["n_used"])
        none = a[a["n_used"] == 0]
        assert not none["min"].any() and not none["max"].any() and not none["sum"].any() and not none["abs_dev"].any()
        for name, n in fc.branches(ev, off, cols, sites, lo, hi).items():
            seen[name] = seen.get(name, 0) + int(n)
    assert set(seen) == set(fc.BRANCHES) and min(seen.values()) >= 20, seen


def test_hand_example():
    """the header's: a library of 350 +- 40, the site (10000 L | 50000 R), four pairs"""
    ev, off, cols, sites = fc.hand_case()
    lo, hi = fc.bounds(fc.HAND_MEAN, fc.HAND_SD)
    assert (lo, hi) == (230, 470) == capi.fragment_bounds(fc.HAND_MEAN, fc.HAND_SD)
    detail = []
    a = fc.expected(ev, off, cols, sites, lo, hi, detail)
    assert a.tobytes() == fc.expected_sorted(ev, off, cols, sites, lo, hi).tobytes()
    assert [(kind, L, s) for _, kind, L, s in detail] == [("used", 401, (200, 201)), ("used", 311, (150, 161)), ("used", 151, (100, 51)), ("off", 0, None)]
    assert fc.rec_endpos(cols)[cols["tid"] == 1].tolist() == [50050, 50160, 50200, 50300]
    r = a[0]
    assert [int(r[f]) for f in ("n_used", "n_off", "n_lost", "n_short", "n_long", "min", "max", "sum", "abs_dev")] == [3, 1, 0, 1, 0, 151, 401, 863, 273]
    assert fc.call_fields(r, fc.HAND_MEAN, fc.HAND_SD) == ["3", "1", "287.7", "91.0", "151", "401", "1", "0", "-1.56"]
    assert fc.info_fields(r, fc.HAND_MEAN, fc.HAND_SD) == ";FGN=3;FGMEAN=287.7;FGZ=-1.56"
    # the other sides: every read stands against the site
    flipped = fc.as_sites([(10000, 50000, 1, 0, 0)])
    assert int(fc.expected(ev, off, cols, flipped, lo, hi)[0]["n_off"]) == 4
    # a skipped site, and the floor of a negative centre: lengths -3 and -4 have the centre floor(-13 / 4) = -4
    assert fc.expected(ev, off, cols, fc.as_sites([(10000, 50000, 0, 1, 1)]), lo, hi)[0].tobytes() == bytes(48)
    r = fc.row_of([-3, -4], 0, 0, lo, hi)
    assert (int(r["sum"]), int(r["abs_dev"]), int(r["n_short"])) == (-7, 1, 2)


def test_fragment_bounds():
    C = capi.C
    for mean, sd in ((350.0, 40.0), (350.5, 40.25), (300.0, 0.0), (100.0, 50.0), (100.0, 33.4), (0.0, 0.0), (-5.5, 1.0), (1e12, 1.0), (1e300, 1e300), (2147483647.0, 0.0),
                     (2147483646.5, 0.0), (349.99999999999994, 0.0), (1.0, 1.0 / 3.0)):
        assert capi.fragment_bounds(mean, sd) == fc.bounds(mean, sd), (mean, sd)
    assert capi.fragment_bounds(350.0, 40.0) == (230, 470)          # exact
    assert capi.fragment_bounds(350.5, 40.25) == (229, 472)         # fractional: floor(229.75), ceil(471.25)
    assert capi.fragment_bounds(100.0, 50.0) == (0, 250)            # a negative low end is 0
    assert capi.fragment_bounds(-5.5, 1.0) == (0, -2)               # (lo > hi: bk_fragment_sizes refuses it)
    assert capi.fragment_bounds(1e12, 1.0) == (fc.I32_MAX, fc.I32_MAX) and capi.fragment_bounds(1e300, 1e300)[1] == fc.I32_MAX
    for mean, sd in ((float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("inf")), (float("-inf"), 0.0), (350.0, -1.0), (350.0, -1e-300)):
        with pytest.raises(capi.BreakIDError) as e:
            capi.fragment_bounds(mean, sd)
        assert e.value.code == abi.BK_ERR_ARG
    lo, hi = C.c_int32(), C.c_int32()
    assert capi.lib().bk_fragment_bounds(350.0, 40.0, None, C.byref(hi)) == abi.BK_ERR_ARG
    assert capi.lib().bk_fragment_bounds(350.0, 40.0, C.byref(lo), None) == abi.BK_ERR_ARG


def test_printed_fields():
    assert len(fc.FRAG_NAMES) == 9
    none = np.zeros(1, abi.FRAG_SIZES)[0]
    none["n_off"] = 4
    assert fc.call_fields(none, 350.0, 40.0) == ["0", "4", ".", ".", ".", ".", "0", "0", "."] and fc.info_fields(none, 350.0, 40.0) == ";FGN=0"
    r = fc.row_of([300, 301], 1, 0, 230, 470)
    assert fc.call_fields(r, 350.0, 40.0) == ["2", "1", "300.5", "0.5", "300", "301", "0", "0", "-1.24"]
    assert fc.call_fields(r, 350.0, 0.0)[-1] == "." and fc.info_fields(r, 350.0, 0.0) == ";FGN=2;FGMEAN=300.5"
    r = fc.row_of([-10, -11, 2500], 0, 0, 230, 470)
    assert fc.call_fields(r, 350.0, 40.0) == ["3", "0", "826.3", "1115.7", "-11", "2500", "2", "1", "11.91"]
    r = fc.row_of([fc.I32_MAX, fc.I32_MAX], 0, 0, 230, 470)
    assert fc.call_fields(r, 350.0, 40.0)[2:6] == ["2147483647.0", "0.0", "2147483647", "2147483647"]


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_fragsize(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-fragsize"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -fragsize needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-fragsize", "-all", "-fast", "-vcf"], capture_output=True, text=True)
    assert r.returncode == 1 and "needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-fragsize", "-partners"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -partners needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    # the usage refusals stand behind the help text, in the order of the table: -fragsize's own behind every older row
    for args, word in ((["-fragsize", "-gpus", "2"], "Error: -fragsize cannot be combined with -gpus."),
                       (["-fragsize", "-gpus", "2", "-partners"], "Error: -partners cannot be combined with -gpus."),
                       (["-fragsize", "-linkdist", "5"], "Error: -linkdist needs -link.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-fragsize " in r.stderr and "FGN / FGMEAN / FGZ" in r.stderr and "Error" not in r.stderr

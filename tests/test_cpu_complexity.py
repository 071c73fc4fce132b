"""Site complexity without a GPU: the row layouts and the exports, the numpy definition (tests/complexitycases.py) against a naive brute
force, designed homopolymer, dinucleotide, breakpoint-touch and tie cases, the shares of the random cases, and the command line's
refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import complexitycases as xc
from tests import homologycases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.REF_SITE.itemsize == 8 and abi.SITE_CPLX.itemsize == 64
    assert list(abi.REF_SITE.names) == ["tid", "pos"]
    assert list(abi.SITE_CPLX.names) == ["covered", "valid", "gc", "masked", "mask_run", "tri_total", "tri_pairs", "tri_distinct", "bp_period", "bp_len", "bp_start",
                                         "max_period", "max_len", "max_start", "reserved"]
    assert [abi.REF_SITE.fields[f][1] for f in abi.REF_SITE.names] == [0, 4]
    assert [abi.SITE_CPLX.fields[f][1] for f in abi.SITE_CPLX.names] == list(range(0, 60, 4))
    assert abi.REF_SITE.fields["tid"][0] == np.dtype("<i4") and abi.REF_SITE.fields["pos"][0] == np.dtype("<u4")
    assert all(abi.SITE_CPLX.fields[f][0] == np.dtype("<u4") for f in abi.SITE_CPLX.names[:-1]) and abi.SITE_CPLX.fields["reserved"][0].shape == (2,)
    assert "bk_site_complexity" in capi.EXPORTS and hasattr(capi.lib(), "bk_site_complexity") and hasattr(capi.Context, "site_complexity")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_ref_site   { int32_t tid; uint32_t pos; };                       /* 8 bytes, pos 1-based */" in header
    assert ("struct bk_site_cplx  { uint32_t covered, valid, gc, masked, mask_run,\n"
            "                       tri_total, tri_pairs, tri_distinct,\n"
            "                       bp_period, bp_len, bp_start,\n"
            "                       max_period, max_len, max_start, reserved[2]; };     /* 64 bytes, reserved = 0 */") in header
    assert ("int bk_site_complexity(bk_ctx *ctx, const bk_refseq *ref, const struct bk_ref_site *sites, uint64_t n, uint32_t flank, uint32_t max_period, "
            "const struct bk_site_cplx **out);") in header


def test_definition_equals_a_brute_force():
    """300 seeded cases with R <= 4: alphabets of 2 to 5 symbols (the fifth is N), periods up to 4, soft-masked bases, one contig in
    one or two segments, sites inside, at and beyond its ends"""
    rng = np.random.default_rng(29)
    tracts = at_bp = masked = partly = 0
    for case in range(300):
        R = int(rng.integers(1, 5))
        symbols = int(rng.integers(2, 6))
        size = 24
        nib = hc.NIB_OF[rng.integers(0, symbols, size)] | (8 * (rng.random(size) < 0.4)).astype(np.uint8)
        if case % 4 == 0:
            ref = hc.make_refseq([(1, 0, nib[:10]), (1, 13, nib[13:])])
        else:
            ref = hc.make_refseq([(1, 0, nib)])
        site = (1 if case % 17 else int(rng.choice([-1, 0, 2])), int(rng.integers(0, size + 4)))
        max_period = int(rng.integers(1, 5))
        fast = xc.expected_cplx(ref, xc.as_sites([site]), R, max_period)[0]
        slow = xc.brute_force(ref, site, R, max_period)
        assert fast.tobytes() == slow.tobytes(), (case, R, site, max_period, fast, slow)
        tracts += int(fast["max_len"]) > 0
        at_bp += int(fast["bp_len"]) > 0
        masked += int(fast["mask_run"]) > 0
        partly += 0 < int(fast["covered"]) < 2 * R + 1
        assert int(fast["bp_len"]) <= int(fast["max_len"]) and int(fast["mask_run"]) <= int(fast["masked"]) <= int(fast["covered"])
    assert tracts > 150 and at_bp > 100 and masked > 60 and partly > 30, (tracts, at_bp, masked, partly)


def row_of(text, R, max_period, pos=None):
    ref = xc.text_ref([text])
    return xc.expected_cplx(ref, xc.as_sites([(0, R + 1 if pos is None else pos)]), R, max_period)[0]


def tract(row, name):
    return tuple(int(row[name + f]) for f in ("_len", "_period", "_start"))


def test_designed_values():
    # a 65-column homopolymer and a 65-column dinucleotide repeat
    r = row_of("A" * 65, 32, 6)
    assert (int(r["tri_pairs"]), int(r["tri_total"]), int(r["tri_distinct"])) == (1953, 63, 1) and tract(r, "max") == tract(r, "bp") == (65, 1, 0)
    assert (int(r["covered"]), int(r["valid"]), int(r["gc"]), int(r["masked"]), int(r["mask_run"])) == (65, 65, 0, 0, 0)
    assert xc.twin_fields(xc.text_ref(["A" * 65]), xc.as_sites([(0, 33)])[0], 32, r) == ["65", "0.000", "31.50", "1", "0.000", "0", "A", "65", "1", "A", "65", "1"]
    r = row_of(("CA" * 33)[:65], 32, 6)
    assert (int(r["tri_pairs"]), int(r["tri_total"]), int(r["tri_distinct"])) == (961, 63, 2) and tract(r, "max") == tract(r, "bp") == (65, 2, 0)
    assert int(r["gc"]) == 33
    assert xc.twin_fields(xc.text_ref([("CA" * 33)[:65]]), xc.as_sites([(0, 33)])[0], 32, r)[:4] == ["65", "0.508", "15.50", "2"]
    # the header's hand example
    r = row_of("GTACACA", 3, 6)
    assert tract(r, "max") == tract(r, "bp") == (5, 2, 2) and (int(r["tri_total"]), int(r["tri_pairs"]), int(r["tri_distinct"]), int(r["gc"])) == (5, 1, 4, 3)
    # the breakpoint: R = 10, filler without two equal neighbours, period 1 alone.  A run over the columns 3 .. R - 2 does not touch
    # [R - 1, R + 1]; one column more and it does; likewise from R + 2 and from R + 1 on
    R = 10
    filler = ("CGT" * 7)
    for a, b, touches in ((3, R - 2, False), (3, R - 1, True), (R + 2, 17, False), (R + 1, 17, True)):
        text = filler[:a] + "A" * (b - a + 1) + filler[b + 1:]
        r = row_of(text, R, 1)
        assert tract(r, "max") == (b - a + 1, 1, a) and tract(r, "bp") == ((b - a + 1, 1, a) if touches else (0, 0, 0)), (a, b, r)
    # soft-mask: lower case from column 4 to 14 around R = 10, and a run that leaves the window at both ends
    r = row_of(filler[:4] + filler[4:15].lower() + filler[15:], R, 1)
    assert (int(r["masked"]), int(r["mask_run"])) == (11, 11)
    r = row_of(filler[:4] + filler[4:10].lower() + filler[10:], R, 1)
    assert (int(r["masked"]), int(r["mask_run"])) == (6, 0)  # column R itself is not masked
    r = row_of(("CGT" * 20).lower(), R, 1, pos=30)
    assert (int(r["masked"]), int(r["mask_run"]), int(r["covered"])) == (21, 21, 21)
    # N and masked N count as covered, not as valid
    ref = hc.make_refseq([(0, 0, np.asarray([2, 4, 5, 6, 7, 12, 13, 14, 15, 2, 9], np.uint8))])
    r = xc.expected_cplx(ref, xc.as_sites([(0, 6)]), 5, 6)[0]
    assert (int(r["covered"]), int(r["valid"]), int(r["masked"]), int(r["mask_run"]), int(r["tri_total"]), int(r["max_len"])) == (11, 3, 5, 4, 0, 0)


def test_tie_rules():
    # the length first: a dinucleotide tract of 6 beats a homopolymer of 4 that stands before it
    r = row_of("TAAAATCGCGCGT", 6, 6)
    assert tract(r, "max") == (6, 2, 6)
    # then the period: a homopolymer of 6 is also a tract of period 2 and of period 3, each 6 long
    r = row_of("CGTAAAAAACGTC", 6, 6)
    assert tract(r, "max") == tract(r, "bp") == (6, 1, 3)
    r = row_of("CGTAAAAAACGTC", 6, 3)
    assert tract(r, "max") == (6, 1, 3)
    # then the start: two homopolymers of 4
    r = row_of("CAAAAGCGTTTTC", 6, 1)
    assert tract(r, "max") == (4, 1, 1) and tract(r, "bp") == (0, 0, 0)  # (columns 1 .. 4 and 8 .. 11: neither reaches 5 .. 7)
    r = row_of("CGTAAAATTTTGC", 6, 1)
    assert tract(r, "max") == tract(r, "bp") == (4, 1, 3)  # (columns 3 .. 6 and 7 .. 10: both touch)
    # at the breakpoint the first tract that touches it wins, not the window's first: AAAAAA far left, CC at the breakpoint
    r = row_of("AAAAAAGTGTCCTGTGTGAC"[:19], 9, 1)
    assert tract(r, "max") == (6, 1, 0) and tract(r, "bp") == (2, 1, 10)
    # a period at or above L has no tract
    r = row_of("AAA", 1, 64)
    assert tract(r, "max") == (3, 1, 0)
    assert xc.expected_cplx(xc.text_ref(["AAA"]), xc.as_sites([(0, 2)]), 1, 64).tobytes() == xc.expected_cplx(xc.text_ref(["AAA"]), xc.as_sites([(0, 2)]), 1, 2).tobytes()


@pytest.mark.parametrize("flank", [1, 2, 31, 32, 64, 96, 255])
def test_random_cases_meet_their_shares(flank):
    n = 200 if flank <= 64 else 48
    ref, sites, plan = xc.random_case(flank, n)
    L = 2 * flank + 1
    xc.assert_plan(plan, L)
    exp = xc.expected_cplx(ref, sites, flank, 6)
    clean = plan["clean"]
    assert (exp["max_len"][clean] >= plan["length"][clean]).all()
    at = clean & plan["covers"]
    assert (exp["bp_len"][at] >= plan["length"][at]).all()
    if L > 64:
        cross = plan["masked_cross"] & ~plan["contig_end"] & ~plan["gap"]
        assert (exp["mask_run"][cross] >= 2).all() and cross.any()


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_complexity(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-complexity"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -complexity needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-complexity", "-cplxflank", "100", "-cplxperiod", "4", "-all", "-fast", "-vcf"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -vcf needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    r = subprocess.run(base + ["-complexity", "-cplxflank", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -complexity needs the GPU library" in r.stderr, r.stderr[-2000:]  # (the library row stands before the range)
    # the usage refusals stand behind the help text
    for args, word in ((["-cplxflank", "100"], "Error: -cplxflank needs -complexity."), (["-cplxperiod", "4"], "Error: -cplxperiod needs -complexity."),
                       (["-complexity", "-gpus", "2"], "Error: -complexity cannot be combined with -gpus."),
                       (["-cplxflank", "100", "-gpus", "2"], "Error: -cplxflank needs -complexity.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-complexity" in r.stderr and "-cplxflank" in r.stderr and "-cplxperiod" in r.stderr and "Error" not in r.stderr

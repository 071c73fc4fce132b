"""CPU: the host side of the VCF breakend output (`-vcf`, `bk_junctions`, `bk_junction_sides`, `bk_vcf_breakend_alt`): the numpy mirror
of the row, the side rule of the library against the rule written out in Python, the ALT text of a breakend, and the command line
built over the CPU oracle (oracle/cpu_shim.cc), which has no `bk_junctions` and must refuse `-vcf` cleanly."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def rule(splits, pairs):
    """(right1, right2, source) as include/breakid_hip.h states it: the largest bin, the smallest index on a tie"""
    for v, source in ((splits, 2), (pairs, 1)):
        if any(v):
            idx = max(range(4), key=lambda i: (v[i], -i))
            return idx >> 1, idx & 1, source
    return 0, 1, 0


def row(splits=(0, 0, 0, 0), pairs=(0, 0, 0, 0), mapq=(0, 0)):
    a = np.zeros(1, abi.JUNCTION)
    a["splits"][0] = splits
    a["pairs"][0] = pairs
    a["mapq_sum1"], a["mapq_sum2"] = mapq
    return a[0]


def test_junction_row_layout():
    assert abi.JUNCTION.itemsize == 48
    assert [abi.JUNCTION.fields[f][1] for f in ("pairs", "splits", "mapq_sum1", "mapq_sum2")] == [0, 16, 32, 40]
    assert abi.JUNCTION.fields["pairs"][0].shape == (4,) and abi.JUNCTION.fields["splits"][0].shape == (4,)
    assert abi.JUNCTION.fields["pairs"][0].base == np.dtype("<u4") and abi.JUNCTION.fields["mapq_sum1"][0] == np.dtype("<u8")
    for name in ("bk_junctions", "bk_junction_sides", "bk_vcf_breakend_alt"):
        assert name in capi.EXPORTS


def test_exports_are_in_the_library():
    L = capi.lib()
    for name in ("bk_junctions", "bk_junction_sides", "bk_vcf_breakend_alt"):
        assert hasattr(L, name)


def test_junction_sides_equals_the_rule():
    zero = (0, 0, 0, 0)
    bad = []
    for v in itertools.product((0, 1, 2, 7), repeat=4):
        for splits, pairs in ((v, zero), (zero, v)):
            got, exp = capi.junction_sides(row(splits, pairs, (5, 9))), rule(splits, pairs)
            if got != exp:
                bad.append((splits, pairs, got, exp))
    assert not bad, bad[:5]
    assert capi.junction_sides(row()) == (0, 1, 0)


def test_junction_sides_mixed_rows_and_ties():
    M = 2 ** 32 - 1
    cases = [((0, 0, 16, 0), (10, 0, 0, 0)),  # split reads overrule the pairs
             ((0, 0, 0, 1), (M, M, M, M)),
             ((3, 3, 3, 3), (0, 0, 0, 9)),    # a tie: the smallest index
             ((0, 5, 5, 0), (0, 0, 9, 0)),
             ((0, 0, 5, 5), (9, 0, 0, 0)),
             ((0, 0, 0, 0), (0, 4, 0, 4)),
             ((0, 0, 0, 0), (0, 0, 4, 4)),
             ((M, M - 1, 0, 0), (0, 0, 0, 0)),
             ((M - 1, M, 0, 0), (1, 2, 3, 4)),
             ((0, 0, 0, 0), (M - 1, 0, 0, M))]
    for splits, pairs in cases:
        assert capi.junction_sides(row(splits, pairs, (2 ** 40, 7))) == rule(splits, pairs), (splits, pairs)
    assert capi.junction_sides(row((0, 0, 16, 0), (10, 0, 0, 0))) == (1, 0, 2)
    assert capi.junction_sides(row((3, 3, 3, 3), (0, 0, 0, 9))) == (0, 0, 2)
    assert capi.junction_sides(row((0, 0, 0, 0), (0, 4, 0, 4))) == (0, 1, 1)
    L = capi.lib()
    assert L.bk_junction_sides(None, None, None, None) == abi.BK_ERR_ARG


def test_vcf_breakend_alt():
    left, right = 0, 1
    assert capi.vcf_breakend_alt("G", left, "chr2", 321681, right) == "G[chr2:321681["
    assert capi.vcf_breakend_alt("G", left, "chr2", 321681, left) == "G]chr2:321681]"
    assert capi.vcf_breakend_alt("T", right, "chr13", 123456, left) == "]chr13:123456]T"
    assert capi.vcf_breakend_alt("T", right, "chr13", 123456, right) == "[chr13:123456[T"
    long_name = "HLA-DRB1*15:01:01:01_" + "x" * 300
    assert capi.vcf_breakend_alt("N", left, long_name, 2 ** 32 - 1, right) == "N[" + long_name + ":4294967295["
    assert capi.vcf_breakend_alt("A", right, long_name, 2 ** 32 - 1, left, cap=len(long_name) + 15) == "]" + long_name + ":4294967295]A"
    # "A]chr1:5]" is 9 characters: 10 bytes with its NUL
    assert capi.vcf_breakend_alt("A", left, "chr1", 5, left, cap=10) == "A]chr1:5]"
    for cap in (9, 1, 0):
        with pytest.raises(capi.BreakIDError) as e:
            capi.vcf_breakend_alt("A", left, "chr1", 5, left, cap=cap)
        assert e.value.code == abi.BK_ERR_ARG
    L = capi.lib()
    assert L.bk_vcf_breakend_alt(b"A", 0, b"chr1", 5, 0, None, 64) == abi.BK_ERR_ARG
    assert L.bk_vcf_breakend_alt(b"A", 0, None, 5, 0, None, 64) == abi.BK_ERR_ARG


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_vcf(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-vcf"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -vcf needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-vcf", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -vcf needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-vcf", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-vcf cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-vcf" in r.stderr

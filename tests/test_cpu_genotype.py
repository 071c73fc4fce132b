"""CPU: the host side of genotyping (`-genotype`, `bk_ref_support`, `bk_genotype_call`): the numpy mirror of the row, the genotype
model of the library against its formula in Python floats, and the command line built over the CPU oracle (oracle/cpu_shim.cc),
which has no `bk_ref_support` and must refuse `-genotype` cleanly."""
import math
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")

# log10 of 0.05, 0.5, 0.95: the model's constants, as hex floats (include/breakid_hip.h)
C10 = (float.fromhex("-0x1.4d104d427de80p+0"), float.fromhex("-0x1.34413509f79ffp-2"), float.fromhex("-0x1.6cf9f8b075bd8p-6"))


def model(k, r):
    """(gt, gq, vaf as float32) of the formula, in Python floats (IEEE double, every product and sum rounded on its own)"""
    if k + r == 0:
        return 255, 0, np.float32(np.nan)
    L = [k * C10[g] + r * C10[2 - g] for g in range(3)]
    best = 0
    for g in (1, 2):
        if L[g] > L[best]:
            best = g
    second = max(L[g] for g in range(3) if g != best)
    gq = min(99, math.floor(10 * (L[best] - second) + 0.5))
    vaf = np.float32(k) / np.float32(k + r)  # (float) k / (float) (k + r): both conversions and the division round to float32
    return best, gq, vaf


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2].dtype == b[2].dtype == np.float32 and (a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2])))


def test_ref_support_row_layout():
    assert abi.REF_SUPPORT.itemsize == 16
    assert [abi.REF_SUPPORT.fields[f][1] for f in ("ref_pairs1", "ref_pairs2", "ref_reads1", "ref_reads2")] == [0, 4, 8, 12]
    assert "bk_ref_support" in capi.EXPORTS and "bk_genotype_call" in capi.EXPORTS


def test_model_constants_are_the_logarithms():
    for c, p in zip(C10, (0.05, 0.5, 0.95)):
        assert abs(c - math.log10(p)) <= 2 ** -52 * abs(c)


PINNED = {(10, 10): (1, 72), (10, 12): (1, 67), (10, 2): (2, 8), (10, 4): (1, 12), (4, 112): (0, 99), (2, 0): (2, 6), (0, 7): (0, 20), (1, 1): (1, 7)}


def test_genotype_call_pinned_values():
    for (k, r), (gt, gq) in PINNED.items():
        got = capi.genotype_call(k, r)
        assert got[:2] == (gt, gq), ((k, r), got)
        assert model(k, r)[:2] == (gt, gq), ((k, r), model(k, r))
    gt, gq, vaf = capi.genotype_call(0, 0)
    assert (gt, gq) == (255, 0) and np.isnan(vaf)


def test_genotype_call_equals_the_formula():
    bad = []
    for k in range(301):
        for r in range(301):
            got, exp = capi.genotype_call(k, r), model(k, r)
            if not same(got, exp):
                bad.append(((k, r), got, exp))
    assert not bad, bad[:5]
    M = 2 ** 32 - 1
    big = [(M, M), (M, 0), (0, M), (M, 1), (1, M), (M, M - 1), (2 ** 31, 2 ** 31), (2 ** 24 + 1, 3), (3, 2 ** 24 + 1), (123_456_789, 987_654_321),
           (2 ** 32 - 2, 2 ** 31 + 7), (1_000_000, 999_999), (16_777_217, 16_777_217)]
    for k, r in big:
        got, exp = capi.genotype_call(k, r), model(k, r)
        assert same(got, exp), ((k, r), got, exp)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_genotype(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-genotype"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -genotype needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-genotype", "-anchor", "25"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -genotype needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-genotype", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-genotype cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-anchor", "10"], capture_output=True, text=True)
    assert r.returncode == 1 and "-anchor needs -genotype" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-genotype", "-anchor", "-3"], capture_output=True, text=True)
    assert r.returncode == 1 and "-anchor must be a number from 0 to 2147483647" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())

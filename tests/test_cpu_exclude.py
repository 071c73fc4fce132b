"""CPU: the command line built over the CPU oracle (oracle/cpu_shim.cc) has no `bk_exclude_regions` and must refuse `-x` cleanly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_exclude(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    bed = tmp_path / "x.bed"
    bed.write_text("chr1\t0\t100\n")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for extra in ([], ["-gpus", "2"]):
        r = subprocess.run(base + ["-x", str(bed)] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: -x needs the GPU library" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())

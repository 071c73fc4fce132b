"""CPU: the host side of the matched normal (`-normal`, `bk_normal_support`): the numpy mirror of the row, and the command line
built over the CPU oracle (oracle/cpu_shim.cc), which has no `bk_normal_support` and must refuse `-normal` cleanly."""
import os
import subprocess

import pytest

from breakid_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_normal_support_row_layout():
    assert abi.NORMAL_SUPPORT.itemsize == 16
    assert [abi.NORMAL_SUPPORT.fields[f][1] for f in ("n_drp", "n_sr", "depth1", "depth2")] == [0, 4, 8, 12]


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_normal(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-normal", str(bam)], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -normal needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-normal", str(bam), "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-normal cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())

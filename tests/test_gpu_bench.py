"""bench.py end to end at a small size: a plain run prints the headline line alone, `--full` adds the side measurements."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_line(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--records", "3000000", "--steps", "2", "--warmup", "1"] + extra,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.strip().split("\n") if l.startswith("{")][-1])


def test_plain_run_prints_the_headline_line_alone():
    line = _bench_line([])
    assert line["metric"] == "M reads/s clustered+split-scanned" and line["unit"] == "M records/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert line["config"]["valid_clusters"] > 100 and line["roofline"]["path_frac"] > 0
    assert "cpu_baseline" not in line and "from_bam" not in line and "from_bam_big" not in line


def test_full_run_adds_the_side_measurements():
    line = _bench_line(["--full", "--cpu-sample", "1000000", "--from-bam", "200000"])
    assert line["value"] > 0 and line["config"]["valid_clusters"] > 100
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["sample"].endswith("GPU result on the sample bit-identical: True"), cb
    fb = line["from_bam"]
    assert fb["records"] == 400000 and fb["reps"] == 5 and fb["file_to_calls_M_records_per_s"] > 0, fb
    assert "from_bam_big" not in line

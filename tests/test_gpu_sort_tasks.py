"""std::sort replays as ONE task dispatch on the caller's stream (sortsvc.inc, k_sort_job): the launch path's form at ROCm's
default of four hardware queues, where the resident sort service is not started.  Every case checks the permutation against
libstdc++'s (the oracle) and which form ran (Context.sort_forms: service jobs, task dispatches, and a third word that is always 0).  The unit
sorts (bk_debug_std_sort) start the service on one stream whenever they can: BREAKID_SORT_SERVICE=0 sends them to the launch
path, where the task dispatch runs.  Own processes: the runtime reads GPU_MAX_HW_QUEUES when it starts, the switches are read once."""
import os
import subprocess
import sys

import pytest

from tests import bigcases

pytestmark = pytest.mark.gpu
ROOT_DIR = bigcases.ROOT

PRELUDE = """
import sys
sys.path.insert(0, %r)
import numpy as np
from breakid_amd import capi
from oracle import pyoracle
from tests.test_gpu_parity import _median3_killer, _triangular
""" % ROOT_DIR


def _run(code, **env_extra):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4", **env_extra)
    for k in ("BREAKID_QUIET", "BREAKID_GROUP_LANES", "BREAKID_SORT_SERVICE", "BK_DEBUG"):
        if k not in env_extra:
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", PRELUDE + code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT_DIR)
    assert r.returncode == 0 and "ST_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_every_heap_size_class_as_a_task_dispatch():
    """Heaps of at most 1024, 2048 and 4096 elements (narrow teams), ranked ones up to the LDS (40 947) and beyond it up to
    65 534 (wide workgroups), median-of-3 killers with and without ties, runs of equal keys, many small groups."""
    code = """
rng = np.random.default_rng(31)
cases = {
    "killer_1024": [_median3_killer(1500, 1), _median3_killer(1200, 2)],
    "killer_2048": [_median3_killer(2500, 1), _median3_killer(3000, 3)],
    "killer_4096": [_median3_killer(6000, 1), _median3_killer(5000, 2)],
    "killer_ranked": [_median3_killer(30000, 1), _median3_killer(40000, 2)],
    "killer_beyond_lds": [_median3_killer(90000, 1), _median3_killer(120000, 3)],
    "equal_runs": [np.repeat(rng.integers(0, 50, 400), 300).astype(np.uint32), np.full(70000, 9, np.uint32)],
    "triangular": [_triangular(rng, 400_000), _triangular(rng, 90_000) // 30],
    "many_groups": [rng.integers(0, 300, int(s)).astype(np.uint32) for s in rng.integers(0, 400, 3000)],
}
ctx = capi.Context([("chr1", 1000)])
done = 0
for name, parts in cases.items():
    key = np.concatenate(parts)
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    got = ctx.debug_std_sort(key, off)
    exp = pyoracle.unit_std_sort(key, off)
    assert np.array_equal(got, exp), (name, int((got != exp).sum()))
    done += 1
forms = ctx.sort_forms()
assert forms == (0, done, 0), forms
ctx.close()
print("ST_OK")
"""
    _run(code, BREAKID_SORT_SERVICE="0")


def test_big_sort_gives_the_same_permutation_twenty_times():
    code = """
rng = np.random.default_rng(5)
parts = [_median3_killer(233512, 3)[:233512], _triangular(rng, 600_000), rng.integers(0, 4000, 300_000).astype(np.uint32)]
key = np.concatenate(parts)
off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
exp = pyoracle.unit_std_sort(key, off)
ctx = capi.Context([("chr1", 1000)])
for rep in range(20):
    got = ctx.debug_std_sort(key, off)
    assert np.array_equal(got, exp), (rep, int((got != exp).sum()))
assert ctx.sort_forms() == (0, 20, 0), ctx.sort_forms()
ctx.close()
print("ST_OK")
"""
    _run(code, BREAKID_SORT_SERVICE="0")


@pytest.mark.parametrize("tasks", ["1"])  # (the case "0", the sort as a chain of launches, went with that form)
def test_wgs_table_both_forms_match_the_oracle(tasks):
    """The 6 M-record WGS-shape table through the lanes at four queues, every sort a task dispatch."""
    code = """
import torch
from breakid_amd import abi, synth_gpu
dev = torch.device("cuda", 0)
contigs, cols = synth_gpu.make_wgs(6_000_000, 4711, dev, disc_frac=0.3)
ctx = capi.Context(contigs)
ctx.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
w, nv = ctx.run(qual=20, fast=True)
forms = ctx.sort_forms()
o = pyoracle.Oracle(contigs, synth_gpu.to_numpy_cols(cols))
ow, rc = o.run(20, fast=True)
assert rc == 0 and w == ow
for st in (abi.STAGE_GROUP_KEYS, abi.STAGE_SCAN, abi.STAGE_ISO, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS):
    a, ao = ctx.fetch(st)
    b, bo = o.fetch(st)
    assert np.array_equal(a, b), st
    if ao is not None: assert np.array_equal(ao, bo), st
print("FORMS", *forms)
print("ST_OK")
"""
    r = _run(code, BK_DEBUG="lanes", BREAKID_LANES_MIN_PAIRS="1000")
    forms = [int(v) for v in r.stdout.split("FORMS", 1)[1].split()[:3]]
    assert forms[0] == 0, forms
    assert forms[1] > 0 and forms[2] == 0, forms
    assert "[lanes] sorts as task dispatches on the lane streams" in r.stderr, r.stderr[-3000:]
    assert "[lanes] launch path: 3 lanes, 1 stream each, 4 hardware queues" in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name", ["deep", "deepw"])
def test_deep_goldens_as_task_dispatches(name):
    """deep / deepw: heap segments of up to ~300 000 elements (beyond the LDS), against the reference's outputs."""
    fx, meta = bigcases.load(name)
    if fx is None or not os.path.exists(os.path.join(bigcases.GOLD, "%s.fast.digest.json" % name)):
        pytest.skip("golden %s not generated" % name)
    code = """
from tests import bigcases
fx, meta = bigcases.load(%r)
ctx = capi.Context(fx.contigs)
ctx.upload(fx.cols)
mean, sd = ctx.isize_stats()
w = capi.w_from(mean, sd)
ctx.discordant_pairs(20, w)
ctx.mask_and_cluster(w, True)
ctx.split_evidence()
ctx.cluster_summary(w)
ctx.split_breakpoints(w)
bigcases.check(%r, "fast", ctx.fetch, mean, sd, w)
forms = ctx.sort_forms()
assert forms[0] == 0 and forms[1] > 0 and forms[2] == 0, forms
ctx.close()
print("ST_OK")
""" % (name, name)
    _run(code, BREAKID_SORT_SERVICE="0")  # (one pass on one stream: the service would serve it)

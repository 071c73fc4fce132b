"""The lane stage of bk_mask_and_cluster at ROCm's default of four hardware queues: the resident sort service needs seven (four lane
streams, two persistent kernels, a copy stream), so nothing of it is started; the launch path runs three lanes (one queue stays
with the process's first stream) with one stream each, and every sort of a lane is one task dispatch on the lane's own stream
(k_sort_job, no side stream).  Results must not change.  Own processes: the runtime reads GPU_MAX_HW_QUEUES when
it starts."""
import os
import subprocess
import sys

import pytest

from tests import bigcases

pytestmark = pytest.mark.gpu
ROOT_DIR = bigcases.ROOT


def _run(code, **env_extra):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4", BK_DEBUG="lanes", BREAKID_LANES_MIN_PAIRS="1000", **env_extra)
    for k in ("BREAKID_QUIET", "BREAKID_GROUP_LANES", "BREAKID_SORT_SERVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT_DIR)
    assert r.returncode == 0 and "QB_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_four_queues_launch_path_one_stream_per_lane_matches_the_oracle():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from breakid_amd import abi, capi, synth_gpu
from oracle import pyoracle
dev = torch.device("cuda", 0)
contigs, cols = synth_gpu.make_wgs(6_000_000, 4711, dev, disc_frac=0.3)
ctx = capi.Context(contigs)
ctx.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
ctx.timing_enable(True)
w, nv = ctx.run(qual=20, fast=True)
names = [t[0] for t in ctx.timing()]
assert "mask_and_cluster_lanes" in names, names
o = pyoracle.Oracle(contigs, synth_gpu.to_numpy_cols(cols))
ow, rc = o.run(20, fast=True)
assert rc == 0 and w == ow
for st in (abi.STAGE_GROUP_KEYS, abi.STAGE_SCAN, abi.STAGE_ISO, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS):
    a, ao = ctx.fetch(st)
    b, bo = o.fetch(st)
    assert np.array_equal(a, b), st
    if ao is not None: assert np.array_equal(ao, bo), st
print("QB_OK", nv)
""" % ROOT_DIR
    r = _run(code)
    assert "[lanes] launch path: 3 lanes, 1 stream each, 4 hardware queues" in r.stderr, r.stderr[-3000:]
    assert "the sort service needs 7: not started" in r.stderr, r.stderr[-3000:]
    assert "sort service started" not in r.stderr and "sort service probe" not in r.stderr, r.stderr[-3000:]
    assert "shares a hardware queue" in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("name", ["deep", "deepw"])
def test_big_heaps_on_the_lane_stream_match_the_reference(name):
    """deep / deepw: inputs whose sorts heapsort segments of up to ~300 000 elements (beyond the LDS), here in the one heap
    dispatch of a lane beside the mid-size heaps and the finisher's."""
    fx, meta = bigcases.load(name)
    if fx is None or not os.path.exists(os.path.join(bigcases.GOLD, "%s.fast.digest.json" % name)):
        pytest.skip("golden %s not generated" % name)
    code = """
import sys
sys.path.insert(0, %r)
from breakid_amd import capi
from tests import bigcases
fx, meta = bigcases.load(%r)
ctx = capi.Context(fx.contigs)
ctx.upload(fx.cols)
ctx.timing_enable(True)
mean, sd = ctx.isize_stats()
w = capi.w_from(mean, sd)
ctx.discordant_pairs(20, w)
ctx.mask_and_cluster(w, True)
ctx.split_evidence()
ctx.cluster_summary(w)
ctx.split_breakpoints(w)
bigcases.check(%r, "fast", ctx.fetch, mean, sd, w)
print("LANES_RAN", "mask_and_cluster_lanes" in [t[0] for t in ctx.timing()])
ctx.close()
print("QB_OK")
""" % (ROOT_DIR, name, name)
    r = _run(code)
    if "LANES_RAN True" in r.stdout:
        assert "1 stream each" in r.stderr, r.stderr[-3000:]

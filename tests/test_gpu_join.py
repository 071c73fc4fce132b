"""The mate join (csrc/join.hip) on the designed candidate tables of tests/joincases.py (tests/test_cpu_join.py pins them on their
edges and the model against the oracle): BK_STAGE_SCAN and its group offsets against the oracle and the plain Python model, byte
for byte, under the join's three attempts.  BK_JOIN_ATTEMPT is read once per process, so attempts 1 and 2 run this module as a
program in a process of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from breakid_amd import abi, capi
from oracle import pyoracle
from tests import joincases as jc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = jc.table_cases()


def oracle_pairs(case):
    o = pyoracle.Oracle(case.contigs, case.cols)
    try:
        o.discordant_pairs(jc.QUAL, case.w)
        return o.fetch(abi.STAGE_SCAN)
    finally:
        o.close()


def same_table(got, goff, exp, eoff, name):
    assert got.dtype == exp.dtype and len(got) == len(exp), (name, len(got), len(exp))
    for f in abi.PAIR.names:
        assert np.array_equal(got[f], exp[f]), (name, f)
    assert got.tobytes() == exp.tobytes(), name
    if len(exp):
        assert np.array_equal(goff, eoff), name
    else:
        assert goff is None or list(goff) == [0], name


def run_case(case):
    ctx = capi.Context(case.contigs)
    try:
        ctx.upload(case.cols)
        n, ng = ctx.discordant_pairs(jc.QUAL, case.w)
        got, goff = ctx.fetch(abi.STAGE_SCAN)
    finally:
        ctx.close()
    exp, eoff = oracle_pairs(case)
    mod, moff = jc.model(case.contigs, case.cols, jc.QUAL, case.w)
    assert n == len(exp) and ng == (len(eoff) - 1 if len(exp) else 0), (case.name, n, ng)
    same_table(got, goff, exp, eoff, case.name)
    same_table(got, goff, mod, moff, case.name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_table_case(case):
    assert os.environ.get("BK_JOIN_ATTEMPT", "0") == "0"  # the suite's own process starts at the first attempt
    run_case(case)


@pytest.mark.parametrize("attempt", [0, 1, 2])
def test_every_table_case_under_attempt(attempt):
    """0: sorted by the upper hash half, mixed runs put right; 1: by the whole hash; 2: by record and then stably by the hash, every
    run walked as it lies"""
    env = dict(os.environ, BK_JOIN_ATTEMPT=str(attempt))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_join"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "JOIN_OK %d" % len(CASES) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- measured record bits ------------------------------------------------------------------------------------------------------------------
def sharded_pairs(case, rec_base):
    ctx = capi.Context(case.contigs)
    try:
        ctx.upload(case.cols)
        ctx.shard_begin(rec_base, jc.QUAL)
        ctx.discordant_pairs(jc.QUAL, case.w)
        return ctx.fetch(abi.STAGE_SCAN)
    finally:
        ctx.close()


@pytest.mark.parametrize("rec_base", jc.REC_BASES)
def test_measured_record_bits(rec_base):
    """a shard's candidates carry the record indices of the whole sample: the bits of the pair sort key follow the largest index at
    hand.  The pairs are those of rec_base 0 with rec shifted; the group order does not move."""
    case = jc.rec_bits_case()
    got, goff = sharded_pairs(case, rec_base)
    exp, eoff = oracle_pairs(case)
    assert len(exp) >= 300 and len(eoff) - 1 >= 30  # (test_cpu_join pins the same)
    exp["rec"] += np.uint64(rec_base)
    same_table(got, goff, exp, eoff, "rec_base %d" % rec_base)
    mod, moff = jc.model(case.contigs, case.cols, jc.QUAL, case.w, rec_base=rec_base)
    same_table(got, goff, mod, moff, "rec_base %d" % rec_base)


def test_record_bits_beyond_the_sort_key_are_refused():
    case = jc.rec_bits_case()
    with pytest.raises(capi.BreakIDError) as e:
        sharded_pairs(case, jc.REC_BASE_LIMIT)
    assert e.value.code == abi.BK_ERR_LIMIT and "64 bits" in str(e.value)


if __name__ == "__main__":
    for c in CASES:
        run_case(c)
    print("JOIN_OK %d" % len(CASES))

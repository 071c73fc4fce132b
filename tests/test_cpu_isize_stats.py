"""The inputs of test_gpu_isize_stats, pinned without a GPU: the plain-Python definition (isizecases.reference_sd) and the C++
`long += double` of the CPU oracle agree on every designed table, and the tables have the properties that let the GPU test fail -
enough increments that differ from floor(d), an sd that a sum of floors does not give, an sd that depends on the record order,
and (below 2^52) an sd that moves when the total is off by one."""
import math

import numpy as np
import pytest

from oracle import pyoracle
from tests import isizecases as ic


def oracle_stats(flag, isize):
    contigs, cols, _ = ic.table(flag, isize)
    o = pyoracle.Oracle(contigs, cols)
    try:
        return o.isize_stats()
    finally:
        o.close()


def check_oracle(flag, isize, exp):
    mean, sd = oracle_stats(flag, isize)
    assert ic.same(mean, exp.mean) and ic.same(sd, exp.sd), (mean, exp.mean, sd, exp.sd)


@pytest.mark.parametrize("name,order,variant", ic.ALL_RECIPES)
def test_oracle_equals_the_python_definition(name, order, variant):
    check_oracle(*ic.recipe(name, order, variant), ic.expected(name, order, variant))


@pytest.mark.parametrize("name,variant,n", ic.PLACED)
def test_oracle_equals_the_python_definition_on_placed_tables(name, variant, n):
    f, z, pos, exp = ic.placed(name, variant, n)
    check_oracle(f, z, exp)
    # a permutation: the same records, the same mean
    f0, z0 = ic.recipe(name, "front", variant, n)
    assert sorted(zip(f.tolist(), z.tolist())) == sorted(zip(f0.tolist(), z0.tolist())) and exp.mean == ic.reference_sd(f0, z0).mean
    # the records put at the chosen places still differ from floor(d) there (record 0 cannot: the total before it is 0)
    assert [p for p in pos if p and not exp.differs[p]] == []
    assert all(ic.eligible(int(f[p])) for p in pos)
    if n % 8:
        assert sorted(p for p in pos if p >= n - n % 8) == list(range(n - n % 8, n))


@pytest.mark.parametrize("n", ic.FALLBACK_SIZES)
def test_oracle_equals_the_python_definition_on_fallback_sizes(n):
    f, z = ic.fallback_table(n)
    check_oracle(f, z, ic.reference_sd(f, z))


@pytest.mark.parametrize("count", [64, 128, 129])
def test_oracle_equals_the_python_definition_on_eligible_counts(count):
    f, z = ic.fallback_with_eligible(count)
    exp = ic.reference_sd(f, z)
    assert exp.n == count and ic.eligible(int(f[0]))
    check_oracle(f, z, exp)


def test_one_and_no_eligible_record():
    f, z = ic.fallback_with_eligible(1)
    exp = ic.reference_sd(f, z)
    assert exp.n == 1 and exp.mean == float(ic.FALLBACK_SPIKE) and exp.sd == 0.0
    check_oracle(f, z, exp)
    f[0] |= 0x400
    exp = ic.reference_sd(f, z)
    assert exp.n == 0 and math.isnan(exp.mean) and math.isnan(exp.sd)
    check_oracle(f, z, exp)


def test_mixed_variant_has_every_reason_and_every_oddity():
    f, z = ic.recipe("40x1.2M", "front", "mixed")
    f = f.astype(np.int64)
    ok = np.asarray([ic.eligible(int(x)) for x in f])
    assert abs(int((~ok).sum()) - len(f) // 4) <= 64
    base = ~ok
    for reason in ((f & 1) == 0, (f & 2) == 0, (f & 0x4) != 0, (f & 0x100) != 0, (f & 0x200) != 0, (f & 0x400) != 0):
        assert int((base & reason).sum()) > 1000
    # one reason each: an ineligible record lacks exactly one of the conditions
    lacking = ((f & 1) == 0).astype(int) + ((f & 2) == 0) + ((f & 0x4) != 0) + ((f & 0x100) != 0) + ((f & 0x200) != 0) + ((f & 0x400) != 0)
    assert set(lacking[base].tolist()) == {1}
    assert int((ok & ((f & 0x800) != 0)).sum()) > 1000 and int((ok & (z < 0)).sum()) > 1000 and int((ok & (z == 0)).sum()) > 50
    count, _ = ic.spikes_of("40x1.2M")
    assert ok[:count].all() and (z[:count] < 0).any() and (z[:count] > 0).any()


# ---- the properties that make the GPU test able to fail -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ic.VARIANTS)
@pytest.mark.parametrize("name", ic.SPIKED)
def test_spiked_front_recipes_round_often(name, variant):
    e = ic.expected(name, "front", variant)
    assert e.round_ups + e.round_downs >= 100 and sum(e.differs) == e.round_ups + e.round_downs
    if name in ic.BEYOND_2_53:
        assert e.T > 1 << 53 and e.round_downs >= 1000


@pytest.mark.parametrize("name,order,variant", ic.ALL_RECIPES)
def test_sum_of_floors_gives_another_sd(name, order, variant):
    e = ic.expected(name, order, variant)
    assert e.sd != math.sqrt(e.floor_sum / float(e.n))


@pytest.mark.parametrize("variant", ic.VARIANTS)
@pytest.mark.parametrize("name", ic.SPIKED)
def test_front_and_back_orders_differ(name, variant):
    a, b = ic.expected(name, "front", variant), ic.expected(name, "back", variant)
    assert a.mean == b.mean and a.floor_sum == b.floor_sum and a.sd != b.sd


@pytest.mark.parametrize("name,order,variant", ic.ALL_RECIPES)
def test_off_by_one_total_shows_in_sd(name, order, variant):
    e = ic.expected(name, order, variant)
    if e.T >= 1 << 52:
        assert name in ic.BEYOND_2_53  # (there (double) T itself rounds: a unit is below its resolution)
        return
    assert math.sqrt((e.T + 1) / float(e.n)) != e.sd and math.sqrt((e.T - 1) / float(e.n)) != e.sd


def test_k50_recipe_sits_right_under_the_switch():
    """informational only (the library's own bound comes from a sum of doubles in no fixed order): the names of the cases"""
    c = ic.k50_count()
    assert 1 <= c < ic.SPIKES["6x10M"][0]
    print("k of the recipes:", {nm: ic.expected(nm).k for nm in ic.NAMES}, "k50 spikes:", c)


def test_table_and_slicer():
    f, z = ic.recipe("40x1.2M", "front", "mixed")
    contigs, cols, rows = ic.table(f, z)
    n = len(f)
    assert len(contigs) == 1 and (np.diff(cols["pos"]) > 0).all() and len(np.unique(cols["qhash"])) == n and len(np.unique(cols["qcheck"])) == n
    assert cols["cigar_off"][-1] == n == len(cols["cigar"]) and cols["aux_off"][-1] == 0
    cuts = [0, 1000, 1000, 2048 + 17, n]
    parts = [rows(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [len(p["tid"]) for p in parts] == [1000, 0, 1065, n - 2065]
    for p in parts:
        assert p["cigar_off"][0] == 0 and p["cigar_off"][-1] == len(p["cigar"]) == len(p["tid"]) and len(p["aux_off"]) == len(p["tid"]) + 1
    for k in ("isize", "flag", "qhash", "pos", "cigar"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), cols[k])

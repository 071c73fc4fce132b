"""The bit-exact insert-size sd replay (csrc/stream.hip: k_sd_count / k_sd_emit / k_sd_walk; api.hip: bk_isize_stats, bk_shard_sd_*;
multi_gpu.hip: k_add_l_before) on inputs where the reference's `long += double` rounds - up, and beyond 2^53 down - thousands of
times (tests/isizecases.py; test_cpu_isize_stats pins those inputs).  Every comparison is exact equality of IEEE doubles against
the plain-Python definition, NaN equal to NaN."""
import numpy as np
import pytest
import torch

from breakid_amd import abi, capi
from breakid_amd.sharded import tensor_from_ptr
from tests import callcases as cc
from tests import isizecases as ic

pytestmark = pytest.mark.gpu
WHERE = ("host", "device")  # bk_upload_records from host arrays / device-resident columns used in place


def gpu_stats(flag, isize, where, qcheck=True):
    contigs, cols, _ = ic.table(flag, isize, qcheck=qcheck)
    ctx, keep = cc.make_ctx(contigs, cols, where, qcheck=qcheck)
    try:
        return ctx.isize_stats()
    finally:
        ctx.close()
        del keep


def check(got, exp):
    print("mean", got[0], exp.mean, "sd", got[1], exp.sd, "k", exp.k, "ups", exp.round_ups, "downs", exp.round_downs)
    assert ic.same(got[0], exp.mean) and ic.same(got[1], exp.sd), (got, exp.mean, exp.sd)


# ---- one context -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,order,variant", ic.ALL_RECIPES)
def test_recipe(name, order, variant, where):
    check(gpu_stats(*ic.recipe(name, order, variant), where), ic.expected(name, order, variant))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,variant,n", ic.PLACED)
def test_placed_at_tile_edges(name, variant, n, where):
    """records whose increment differs from floor(d) at records 0, 255, 256, 2047, 2048, 2049 and n - 1, and for n % 8 != 0 in the
    last partial group of eight (the scalar tail of k_sd_count against the strided rows of k_sd_emit)"""
    f, z, _, exp = ic.placed(name, variant, n)
    check(gpu_stats(f, z, where), exp)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n", ic.FALLBACK_SIZES)
def test_sizes_with_every_record_replayed(n, where):
    """the bound beyond 2^51: every eligible record is an exception, so every row and tile path of k_sd_emit writes and k_sd_walk
    takes whole and partial batches of 64"""
    f, z = ic.fallback_table(n)
    check(gpu_stats(f, z, where, qcheck=(n % 2 == 0)), ic.reference_sd(f, z))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("count", [64, 128, 129])
def test_eligible_counts_at_the_batch_of_the_walk(count, where):
    f, z = ic.fallback_with_eligible(count)
    exp = ic.reference_sd(f, z)
    assert exp.n == count
    check(gpu_stats(f, z, where), exp)


@pytest.mark.parametrize("where", WHERE)
def test_one_eligible_record(where):
    f, z = ic.fallback_with_eligible(1)
    exp = ic.reference_sd(f, z)
    assert exp.n == 1
    check(gpu_stats(f, z, where), exp)


@pytest.mark.parametrize("where", WHERE)
def test_no_eligible_record_gives_nan(where):
    f, z = ic.fallback_with_eligible(1)
    f[0] |= 0x400
    exp = ic.reference_sd(f, z)
    assert exp.n == 0 and np.isnan(exp.mean) and np.isnan(exp.sd)
    check(gpu_stats(f, z, where), exp)


# ---- several contexts of one process through the bk_shard_* entry points ----------------------------------------------------------------
def sharded_stats(flag, isize, cuts, where):
    """The statistics steps of sharded.py's sequence without a process group: the table cut at `cuts` into contexts on device 0,
    the sums added and the maxima taken in shard order, the exception lists made global and concatenated in shard order.
    Returns every context's (mean, sd)."""
    contigs, _, rows = ic.table(flag, isize)
    bounds = [0] + list(cuts) + [len(flag)]
    dev = torch.device("cuda", 0)
    ctxs, keep = [], []
    try:
        for a, b in zip(bounds[:-1], bounds[1:]):
            ctx, k = cc.make_ctx(contigs, rows(a, b), where)
            ctxs.append(ctx)
            keep.append(k)
            ctx.shard_begin(a)
        tot = abi.ShardStats()
        for s in (c.shard_get_stats() for c in ctxs):
            tot.isize_sum += s.isize_sum
            tot.isize_n += s.isize_n
            tot.sumsq += s.sumsq
            tot.vmax = max(tot.vmax, s.vmax)
            tot.max_span = max(tot.max_span, s.max_span)
        for c in ctxs:
            c.shard_set_stats(tot)
        parts, offset = [], 0
        for c in ctxs:
            lt, ptr, nex = c.shard_sd_local()
            ex = tensor_from_ptr(ptr, nex * 16, dev).clone()
            if nex and offset:
                ex.view(torch.int64).view(-1, 2)[:, 0] += offset  # l_before: the floor totals of the shards in front
            parts.append(ex)
            offset += lt
        all_ex = torch.cat(parts)
        torch.cuda.synchronize(dev)
        return [c.shard_sd_finish(all_ex.data_ptr() if all_ex.numel() else 0, all_ex.numel() // 16, offset) for c in ctxs]
    finally:
        for c in ctxs:
            c.close()
        del keep


def cut_sets(name):
    count, _ = ic.spikes_of(name)
    n = ic.N_BASE
    return [("mid_tile", [1000]), ("past_a_tile", [2048 + 17]), ("behind_the_spikes", [count]), ("three_mid_tile", [1000, 2048 + 17]),
            ("three_behind_the_spikes", [count, n // 2]), ("a_shard_without_records", [1000, 1000]), ("last_record_alone", [n // 3, n - 1])]


SHARD_CASES = [(nm, tag, cuts) for nm in ("40x1.2M", "8x60M") for tag, cuts in cut_sets(nm)]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,tag,cuts", SHARD_CASES, ids=["%s-%s" % (c[0], c[1]) for c in SHARD_CASES])
def test_shards_of_one_process(name, tag, cuts, where):
    """2 and 3 contexts; cuts inside a tile, right behind the spikes, and one that leaves a shard with no record at all (the library
    takes an empty table).  Every context must give the statistics of the WHOLE table."""
    exp = ic.expected(name, "front", "mixed")
    for got in sharded_stats(*ic.recipe(name, "front", "mixed"), cuts, where):
        check(got, exp)


@pytest.mark.parametrize("name", ["40x1.2M", "8x60M"])
def test_shard_without_an_eligible_record(name):
    f, z = (np.array(a) for a in ic.recipe(name, "front", "mixed"))
    f[5000:5100] |= 0x400
    exp = ic.reference_sd(f, z)
    assert not any(ic.eligible(int(x)) for x in f[5000:5100]) and exp.round_ups + exp.round_downs >= 100
    for got in sharded_stats(f, z, [5000, 5100], "host"):
        check(got, exp)


@pytest.mark.parametrize("cuts", [[1000], [1000, 2048 + 17]])
def test_shards_without_any_eligible_record_give_nan(cuts):
    f, z = (np.array(a[:5000]) for a in ic.recipe("8x60M", "front", "mixed"))
    f |= 0x400
    exp = ic.reference_sd(f, z)
    assert exp.n == 0
    for got in sharded_stats(f, z, cuts, "host"):
        check(got, exp)


# ---- bk_multi_run, local transport: the C++ orchestration and its k_add_l_before --------------------------------------------------------
@pytest.mark.parametrize("n_ctx", [2, 3])
@pytest.mark.parametrize("name", ["40x1.2M", "8x60M"])
def test_multi_run_local_transport(name, n_ctx):
    """bk_multi_run -> bk_multi_stats -> bk_multi_free with 2 and 3 contexts on the one GPU.  The table has no discordant pair: the run
    ends cleanly with no call."""
    contigs, cols, _ = ic.table(*ic.recipe(name, "front", "mixed"))
    r = capi.multi_run(contigs, cols, n_ctx, transport=capi.TRANSPORT_LOCAL, qual=20, fast=True)
    exp = ic.expected(name, "front", "mixed")
    check((r["mean"], r["sd"]), exp)
    assert r["w"] == capi.w_from(exp.mean, exp.sd) and r["n_clustered"] == 0 and len(r["clusters"]) == 0

"""Shared cases of the insert-size sd tests (test_cpu_isize_stats, test_gpu_isize_stats, shard_worker): the definition of the
statistic in plain Python, small record tables that carry nothing but a flag and an insert size per record, and the designed
inputs on which the reference's `long += double` accumulation rounds up (and, beyond 2^53, down) often enough that a replay
with a wrong order, a wrong prefix or a wrong correction gives another sd."""
import functools
import math
from collections import namedtuple

import numpy as np

NOT_ELIGIBLE = 0x4 | 0x100 | 0x200 | 0x400  # (0x800 does not exclude a record)

SdRef = namedtuple("SdRef", "mean sd T floor_sum n round_ups round_downs differs k")


def eligible(f):
    return bool((f & 1) and (f & 2) and not (f & NOT_ELIGIBLE))


def library_k(s, sumsq, vmax, n):
    """The exponent of the library's bound on the final total (api.hip: bk_isize_stats), from exact sums.  The library's own sum
    of squares is a sum of doubles in no fixed order, so this names cases and is never asserted on."""
    nf = float(n)
    m = float(s) / nf
    sum_d = float(sumsq) - 2.0 * m * float(s) + nf * m * m
    if not sum_d > 0:
        sum_d = 0.0
    da = float(vmax) - m
    dmax = da * da + m * m
    bound = 2.0 * sum_d + 2.0 * nf + 2.0 * dmax + 4.0
    return math.frexp(bound)[1]  # ilogb(bound) + 1


def reference_sd(flag, isize):
    """mean and sd of |isize| over the eligible records as the reference computes them: T = (long) ((double) T + d) in record
    order with d = ((double) v - mean)^2, sd = sqrt(T / (double) n).  Python floats are IEEE doubles, every operation below rounds
    once, and nothing is contracted."""
    flag = np.asarray(flag).tolist()
    isize = np.asarray(isize).tolist()
    idx = [i for i, f in enumerate(flag) if eligible(f)]
    differs = [False] * len(flag)
    n = len(idx)
    if n == 0:
        return SdRef(math.nan, math.nan, 0, 0, 0, 0, 0, differs, None)
    v = [abs(isize[i]) for i in idx]
    s = sum(v)
    mean = float(s) / float(n)
    T = floor_sum = ups = downs = 0
    for i, x in zip(idx, v):
        a = float(x) - mean
        d = a * a
        fl = int(d)  # d >= 0: truncation is floor
        inc = int(float(T) + d) - T
        T += inc
        floor_sum += fl
        if inc != fl:
            differs[i] = True
            if inc > fl:
                ups += 1
            else:
                downs += 1
    return SdRef(mean, math.sqrt(T / float(n)), T, floor_sum, n, ups, downs, differs, library_k(s, sum(x * x for x in v), max(v), n))


def same(a, b):
    """exact equality of two doubles, NaN equal to NaN"""
    return a == b or (math.isnan(a) and math.isnan(b))


# ---- record tables ---------------------------------------------------------------------------------------------------------------------
def table(flag, isize, qcheck=True):
    """(contigs, cols, rows): a coordinate-sorted table that Context.upload accepts - every record on the one contig at ascending
    positions, one CIGAR word (100M), no aux bytes, distinct read-name hashes; rows(a, b) gives records [a, b) as a table of
    their own (offsets rebased)."""
    flag = np.array(flag, np.uint16)  # (copies: the cached recipes are read-only)
    isize = np.array(isize, np.int32)
    n = len(flag)
    assert len(isize) == n
    i = np.arange(n, dtype=np.int64)
    cols = {"tid": np.zeros(n, np.int32), "pos": (1000 + i).astype(np.int32), "mtid": np.zeros(n, np.int32), "mpos": (1000 + i).astype(np.int32), "isize": isize,
            "flag": flag, "mapq": np.full(n, 60, np.uint8), "qhash": np.asarray([((k + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF for k in range(n)], np.uint64),
            "cigar_off": np.arange(n + 1, dtype=np.uint32), "cigar": np.full(n, (100 << 4) | 0, np.uint32), "aux_off": np.zeros(n + 1, np.uint32),
            "aux": np.zeros(0, np.uint8)}
    if qcheck:
        cols["qcheck"] = (i + 1).astype(np.uint32)
    contigs = [("chr1", max(n, 1) + 10_000)]

    def rows(a, b):
        out = {k: np.ascontiguousarray(c[a:b]) for k, c in cols.items() if k not in ("cigar_off", "cigar", "aux_off", "aux")}
        for blob, off in (("cigar", "cigar_off"), ("aux", "aux_off")):
            o = cols[off].astype(np.int64)
            out[off] = (o[a:b + 1] - o[a]).astype(np.uint32)
            out[blob] = np.ascontiguousarray(cols[blob][o[a]:o[b]])
        return out

    return contigs, cols, rows


# ---- the designed recipes --------------------------------------------------------------------------------------------------------------
N_BASE = 40_000
FLAGS_OK = (0x63, 0x93)  # first / second read of a proper pair
MARGIN = 64              # the mixed variant leaves the first records (where the spikes go) and the last ones eligible


def base_isize(n=N_BASE):
    return np.random.default_rng(11).integers(100, 20001, size=n).astype(np.int32)


def with_spikes(isize, count, value, signs=False):
    """the first `count` insert sizes overwritten with the spike value (every other one negative with `signs`)"""
    out = np.array(isize, np.int32)
    if count:
        out[:count] = value
        if signs:
            out[1:count:2] *= -1
    return out


BACK_TAIL = 1000


def to_back(a, count):
    """the same records with the spikes moved behind all but the last BACK_TAIL: what follows them is too little to round often,
    and enough for the sum of floors to give another sd even where (double) T has lost its low bits"""
    a = np.asarray(a)
    n = len(a)
    if not count or n <= count + BACK_TAIL:
        return np.array(a)
    return np.concatenate([a[count:n - BACK_TAIL], a[:count], a[n - BACK_TAIL:]])


@functools.lru_cache(maxsize=None)
def k50_count():
    """the largest number of 10 000 000 spikes for which the library's bound stays below 2^50: the selective regime right under
    the switch to replaying everything"""
    best = 0
    for c in range(1, 7):
        v = [int(x) for x in with_spikes(base_isize(), c, 10_000_000)]
        if library_k(sum(v), sum(x * x for x in v), max(v), len(v)) <= 50:
            best = c
    assert best
    return best


# name -> (spike count, spike value); "k50" is filled in from k50_count()
SPIKES = {"none": (0, 0), "40x1.2M": (40, 1_200_000), "k50": (None, 10_000_000), "6x10M": (6, 10_000_000), "30x10M": (30, 10_000_000), "8x60M": (8, 60_000_000),
          "4x500M": (4, 500_000_000)}
NAMES = tuple(SPIKES)
SPIKED = tuple(n for n in NAMES if n != "none")
BEYOND_2_53 = ("8x60M", "4x500M")
ORDERS = ("front", "back")
VARIANTS = ("plain", "mixed")
MIXED_SEED = 5  # (a seed with which the mixed variant of every recipe meets the input conditions of test_cpu_isize_stats)


def spikes_of(name):
    c, v = SPIKES[name]
    return (k50_count() if c is None else c), v


def mixed_flags(n, seed=MIXED_SEED):
    """a seeded quarter of the records not eligible, one record for each single reason in turn; among the others some carry 0x800"""
    rng = np.random.default_rng(seed)
    flag = np.where(np.arange(n) % 2 == 0, FLAGS_OK[0], FLAGS_OK[1]).astype(np.uint16)
    inner = np.arange(MARGIN, n - MARGIN) if n > 4 * MARGIN else np.arange(1, n)
    bad = rng.choice(inner, size=len(inner) // 4, replace=False)
    for j, i in enumerate(bad):
        f = int(flag[i])
        flag[i] = (f & ~1, f & ~2, f | 0x4, f | 0x100, f | 0x200, f | 0x400)[j % 6]
    sup = rng.choice(n, size=n // 10, replace=False)
    flag[sup] |= 0x800
    return flag


def mixed_isize(isize, seed=MIXED_SEED):
    """some insert sizes negative, some zero (the spikes are written over the first records afterwards)"""
    rng = np.random.default_rng(seed + 1000)
    out = np.array(isize, np.int32)
    n = len(out)
    neg = rng.choice(n, size=n // 3, replace=False)
    out[neg] *= -1
    if n > 4 * MARGIN:
        out[rng.choice(np.arange(MARGIN, n - MARGIN), size=n // 200, replace=False)] = 0
    return out


@functools.lru_cache(maxsize=None)
def recipe(name, order="front", variant="plain", n=N_BASE):
    """(flag, isize) of a recipe: the base table with the spikes over its first records (front), or those same records with the
    spikes moved near the end (back, to_back) - a permutation, so the mean and every d are those of the front order"""
    count, value = spikes_of(name)
    isize = base_isize(n)
    if variant == "mixed":
        isize = mixed_isize(isize)
        flag = mixed_flags(n)
    else:
        flag = np.where(np.arange(n) % 2 == 0, FLAGS_OK[0], FLAGS_OK[1]).astype(np.uint16)
    isize = with_spikes(isize, count, value, signs=(variant == "mixed"))
    if order == "back":
        flag, isize = to_back(flag, count), to_back(isize, count)
    flag.setflags(write=False)
    isize.setflags(write=False)
    return flag, isize


@functools.lru_cache(maxsize=None)
def expected(name, order="front", variant="plain", n=N_BASE):
    return reference_sd(*recipe(name, order, variant, n))


ALL_RECIPES = [(nm, o, v) for nm in NAMES for o in ORDERS for v in VARIANTS if not (nm == "none" and o == "back")]


# ---- placement -------------------------------------------------------------------------------------------------------------------------
def place(flag, isize, positions):
    """The same records in another order: records on which the reference's increment differs from floor(d) - the last ones of
    the table - change places with whatever sits at `positions`.  Neither the mean nor any d changes; the expected result belongs
    to the new order and is computed afresh by the caller.  Returns (flag, isize)."""
    flag, isize = np.array(flag, np.uint16), np.array(isize, np.int32)
    positions = [int(p) for p in positions]
    taken = set(positions)
    src = [i for i in np.nonzero(reference_sd(flag, isize).differs)[0][::-1] if int(i) not in taken][:len(positions)]
    assert len(src) == len(positions), "too few records whose increment differs from floor(d)"
    for p, s in zip(positions, src):
        flag[[p, s]] = flag[[s, p]]
        isize[[p, s]] = isize[[s, p]]
    return flag, isize


def placement_positions(n):
    """tile edges of k_sd_emit (256 records a row, 2048 a tile), both ends, and - when n is no multiple of eight - every record of
    the last partial group of eight, which k_sd_count takes one by one"""
    pos = [0, 255, 256, 2047, 2048, 2049, n - 1]
    if n % 8:
        pos += list(range(n - n % 8, n - 1))
    return pos


PLACED = [(nm, v, n) for nm in ("40x1.2M", "8x60M") for v in VARIANTS for n in (N_BASE, N_BASE - 3)]


@functools.lru_cache(maxsize=None)
def placed(name, variant, n):
    """(flag, isize, positions, SdRef of the new order)"""
    flag, isize = recipe(name, "front", variant, n)
    pos = placement_positions(n)
    f, z = place(flag, isize, pos)
    return f, z, pos, reference_sd(f, z)


# ---- sizes in the regime where every eligible record is replayed ---------------------------------------------------------------------------
FALLBACK_SIZES = (1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5)
FALLBACK_SPIKE = 60_000_000


def fallback_table(n):
    """one spike as record 0, the rest ordinary: the library's bound is beyond 2^51, so every eligible record is an exception"""
    flag = np.where(np.arange(n) % 2 == 0, FLAGS_OK[0], FLAGS_OK[1]).astype(np.uint16)
    isize = base_isize(max(n, 1))[:n].copy()
    isize[0] = FALLBACK_SPIKE
    return flag, isize


def fallback_with_eligible(count, n=1000):
    """a mixed table of n records of which exactly `count` are eligible (record 0, the spike, among them)"""
    rng = np.random.default_rng(100 + count)
    flag, isize = fallback_table(n)
    isize = mixed_isize(isize)
    isize[0] = FALLBACK_SPIKE
    keep = set([0] + [int(i) for i in rng.choice(np.arange(1, n), size=count - 1, replace=False)])
    j = 0
    for i in range(n):
        if i not in keep:
            f = int(flag[i])
            flag[i] = (f & ~1, f & ~2, f | 0x4, f | 0x100, f | 0x200, f | 0x400)[j % 6]
            j += 1
    return flag, isize

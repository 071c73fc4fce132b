"""The scan and radix-sort definitions of tests/primcases.py without a GPU: against pure Python (sorted(), int sums) on small cases,
the boundary sizes they derive from the build's tile constants, that the dirty keys really tie inside a range and differ above it,
and that the hooks are exported, bound, declared and documented."""
import os
import re

import numpy as np
import pytest

from breakid_amd import capi
from tests import primcases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")
HOOKS = ("bk_debug_scan", "bk_debug_radix_sort", "bk_debug_prims_info")


def test_hooks_exported_bound_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("Test hooks of the C ABI"):]
    item = item[:item.index("\n* ")]
    for name in HOOKS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in item, name
    assert callable(capi.Context.debug_scan) and callable(capi.Context.debug_radix_sort)


def test_constants_of_the_build_and_the_sizes_they_give():
    c = capi.prims_info()
    assert c == pc.TODAY  # (a change of a tile width moves every boundary below with it: update TODAY and the numbers here)
    src = open(os.path.join(CSRC, "prims.h")).read()
    assert re.search(r"constexpr int BLOCK = %d;" % c["BLOCK"], src)
    scan, sort = pc.scan_sizes(c), pc.sort_sizes(c)
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 32767, 32768, 32769, 36863, 36864, 36865, 524287, 524288, 524289} <= set(scan)
    assert max(scan) > 1.15 * 524288 and max(scan) % c["SCAN_TILE"] and len(scan) == len(set(scan))
    assert {0, 1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 262143, 262144, 262145} <= set(sort)
    assert max(sort) == 262145
    big = pc.sort_big_size(c)
    assert big > 4194304 and 256 * -(-big // c["RS_TILE"]) > c["BLOCK"] * c["SCAN_TILE"]  # its histogram: a second trip
    assert pc.sort_range_sizes(c) == [2049, 262145]
    # the sizes move with the constants
    wide = dict(c, SCAN_TILE=4096, SCAN_ONE_MAX=65536, RS_TILE=4096)
    assert {65536, 65537, 256 * 4096 + 1} <= set(pc.scan_sizes(wide)) and 4096 * 65536 // 256 + 1 in pc.sort_sizes(wide)
    assert pc.sort_big_size(wide) > 4096 * 256 * 4096 // 256


def test_bit_ranges():
    assert pc.BIT_RANGES == [(0, 64), (32, 64), (0, 32), (0, 8), (0, 1), (0, 13), (0, 37), (8, 24), (5, 21), (56, 64), (60, 64), (7, 7), (9, 3)]
    assert pc.IDENTITY_RANGES == [(7, 7), (9, 3)]
    assert pc.UNALIGNED_RANGES == [(0, 1), (0, 13), (0, 37)]
    assert all(r in pc.BIT_RANGES for r in pc.SIZE_RANGES)


# ---- the scan definition ------------------------------------------------------------------------------------------------------------
def python_scan(values, bits):
    out, acc = [0], 0
    for v in values:
        acc = (acc + int(v)) % (1 << bits)
        out.append(acc)
    return out


@pytest.mark.parametrize("pattern", pc.SCAN_PATTERNS)
def test_scan_reference_against_python_ints(pattern):
    for n in (0, 1, 2, 65, 257, 1000):
        v = pc.make_scan_values(pattern, n)
        bits = 8 * v.dtype.itemsize
        assert v.dtype == (np.uint32 if pattern.startswith("u32") else np.uint64) and len(v) == n
        ref = pc.scan_reference(v)
        assert ref.dtype == v.dtype and len(ref) == n + 1
        assert [int(x) for x in ref] == python_scan(v, bits), (pattern, n)


def test_scan_reference_wraps():
    v = np.array([(1 << 64) - 1, 2, (1 << 63), (1 << 63), 5], np.uint64)
    assert [int(x) for x in pc.scan_reference(v)] == [0, (1 << 64) - 1, 1, (1 << 63) + 1, 1, 6]
    v = np.array([(1 << 32) - 1, 2, 1 << 31, 1 << 31, 5], np.uint32)
    assert [int(x) for x in pc.scan_reference(v)] == [0, (1 << 32) - 1, 1, (1 << 31) + 1, 1, 6]
    # the patterns do what their names say at the sizes the GPU test runs
    n = 32769
    assert sum(int(x) for x in pc.make_scan_values("u32_wrap", n)) >> 32 > 1000
    assert sum(int(x) for x in pc.make_scan_values("u64_wrap", n)) >> 64 > 1000
    wide = sum(int(x) for x in pc.make_scan_values("u64_wide", n))
    assert (1 << 40) < wide < (1 << 63)
    for pattern, pos in (("u32_first", 0), ("u32_last", n - 1), ("u32_tile", 32768)):
        assert np.flatnonzero(pc.make_scan_values(pattern, n)).tolist() == [pos]
    assert pc.scan_tile_boundary(2049) == 2048 and pc.scan_tile_boundary(2048) == 1792 and pc.scan_tile_boundary(1) == 0
    assert pc.scan_tile_boundary(524289) == 524288 and pc.scan_tile_boundary(36865) == 36864


# ---- the sort definition ------------------------------------------------------------------------------------------------------------
def python_sort(keys, vals, begin, end):
    width = max(0, end - begin)
    rows = sorted(zip((int(k) for k in keys), (int(v) for v in vals)), key=lambda kv: (kv[0] >> begin) & ((1 << width) - 1))  # sorted() is stable
    return [k for k, _ in rows], [v for _, v in rows]


@pytest.mark.parametrize("pattern", pc.KEY_PATTERNS)
def test_sort_reference_against_python_sorted(pattern):
    for begin, end in pc.BIT_RANGES:
        for n in (0, 1, 2, 67, 300):
            keys, vals = pc.make_keys(pattern, n, begin, end), pc.make_vals(n)
            assert keys.dtype == np.uint64 and vals.dtype == np.uint32 and len(keys) == len(vals) == n
            k, v = pc.sort_reference(keys, vals, begin, end)
            pk, pv = python_sort(keys, vals, begin, end)
            assert [int(x) for x in k] == pk and [int(x) for x in v] == pv, (pattern, begin, end, n)
            if end <= begin:
                assert k.tobytes() == keys.tobytes() and v.tobytes() == vals.tobytes()


def test_width_64_mask_and_high_bits():
    keys = np.array([(1 << 64) - 1, 1 << 63, 0, (1 << 63) - 1, 1 << 63, 1], np.uint64)
    vals = np.arange(6, dtype=np.uint32) + 10
    assert [int(x) for x in pc.range_digits(keys, 0, 64)] == [int(x) for x in keys]
    k, v = pc.sort_reference(keys, vals, 0, 64)
    assert [int(x) for x in k] == [0, 1, (1 << 63) - 1, 1 << 63, 1 << 63, (1 << 64) - 1] and v.tolist() == [12, 15, 13, 11, 14, 10]
    assert [int(x) for x in pc.range_digits(keys, 60, 64)] == [15, 8, 0, 7, 8, 0]
    assert [int(x) for x in pc.range_digits(keys, 32, 64)] == [(1 << 32) - 1, 1 << 31, 0, (1 << 31) - 1, 1 << 31, 0]
    assert pc.range_digits(keys, 9, 3).tolist() == [0] * 6


def test_key_patterns_are_what_they_are_called():
    n = 2049
    for begin, end in [r for r in pc.BIT_RANGES if r[1] > r[0]]:
        top = (1 << (end - begin)) - 1
        d = {p: pc.range_digits(pc.make_keys(p, n, begin, end), begin, end) for p in pc.KEY_PATTERNS}
        assert len(np.unique(d["equal"])) == 1 and not d["digits0"].any() and (d["digits255"] == np.uint64(top)).all()
        assert (np.diff(d["sorted"].astype(object)) >= 0).all() and (np.diff(d["reversed"].astype(object)) <= 0).all()
        assert len(np.unique(d["three"])) <= 3 and len(np.unique(d["one_digit"])) <= 256
        assert len(np.unique(d["uniform"])) == min(top + 1, len(np.unique(d["uniform"]))) and len(np.unique(d["uniform"])) > min(top, 1000)
        if end - begin > 8:
            x = np.bitwise_or.reduce(d["one_digit"] ^ d["one_digit"][0])
            assert int(x) and int(x) == int(x) & (0xFF << (int(x).bit_length() - 1) // 8 * 8)  # one byte of the range varies
        for p in pc.KEY_PATTERNS:
            keys = pc.make_keys(p, n, begin, end)
            above = keys >> np.uint64(end) if end < 64 else np.zeros(n, np.uint64)
            if p == "dirty":
                assert end == 64 or len(np.unique(above)) > n // 2
            elif p == "bit63":
                assert (keys >> np.uint64(63) == 1).all()
            else:
                assert not above.any(), (p, begin, end)
        if begin:
            assert len(np.unique(pc.make_keys("uniform", n, begin, end) & np.uint64((1 << begin) - 1))) > min(1 << begin, n) // 2
    assert not np.array_equal(pc.make_vals(n), np.arange(n)) and len(np.unique(pc.make_vals(n))) > n - 8
    assert pc.make_keys("uniform", n, 0, 64).tobytes() == pc.make_keys("uniform", n, 0, 64).tobytes()  # fixed seeds
    assert pc.make_keys("uniform", n, 0, 64, seed=1).tobytes() != pc.make_keys("uniform", n, 0, 64).tobytes()


def test_dirty_keys_tie_inside_the_range_and_differ_above_it():
    """without this the contract test of test_gpu_prims.py could pass with nothing at stake"""
    for begin, end in pc.UNALIGNED_RANGES:
        for n in pc.sort_range_sizes() + [n for n in pc.sort_sizes() if n >= 63]:
            keys = pc.make_keys("dirty", n, begin, end)
            assert pc.dirty_pairs(keys, begin, end) >= n // 2, (begin, end, n)
            # ... and a sort of the whole last digit, bits beyond end_bit included, would order these keys differently
            whole = begin + -(-(end - begin) // 8) * 8
            a, _ = pc.sort_reference(keys, pc.make_vals(n), begin, end)
            b, _ = pc.sort_reference(keys, pc.make_vals(n), begin, whole)
            assert a.tobytes() != b.tobytes(), (begin, end, n)


def test_nothing_takes_a_device_side_count():
    """the scan kernels take their element count from the host alone (the n_dev form had no caller and went)"""
    for name in os.listdir(CSRC):
        if name.endswith((".h", ".hip", ".inc", ".cc")):
            text = open(os.path.join(CSRC, name)).read()
            assert "exclusive_scan_devn" not in text and not re.search(r"\bn_dev\b", text), name

"""The device-wide scan and radix sort of csrc/prims.h alone (bk_debug_scan, bk_debug_radix_sort) against the numpy definitions of
tests/primcases.py, byte for byte: every size at which they change form (derived from the build's tile constants), both element
types, in place and not, every bit range and key pattern, keys that are not zero outside the sorted range, buffers reused across
calls of different sizes, calls interleaved on one context, repeated calls, and the argument errors.  A failure names the size, the
bit range, the pattern and the first position that differs."""
import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import primcases as pc

pytestmark = pytest.mark.gpu
CONTIGS = [("chr1", 1000)]


@pytest.fixture(scope="module")
def consts():
    return capi.prims_info()


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(CONTIGS)
    yield c
    c.close()


def check_scan(ctx, values, in_place, what):
    got = ctx.debug_scan(values, in_place=in_place)
    exp = pc.scan_reference(values)
    assert got.dtype == exp.dtype
    if got.tobytes() != exp.tobytes():
        i = pc.first_difference(got, exp)
        pytest.fail("scan %s in_place=%s: first difference at %d of %d: got %d, expected %d" % (what, in_place, i, len(values), int(got[i]), int(exp[i])))


def check_sort(ctx, keys, vals, begin, end, what, exp=None):
    gk, gv = ctx.debug_radix_sort(keys, vals, begin, end)
    ek, ev = exp if exp is not None else pc.sort_reference(keys, vals, begin, end)
    if gk.tobytes() != ek.tobytes() or gv.tobytes() != ev.tobytes():
        ik, iv = pc.first_difference(gk, ek), pc.first_difference(gv, ev)
        i = min(x for x in (ik, iv) if x is not None)
        pytest.fail("sort %s n=%d bits [%d, %d): first difference at %d: got (%#x, %d), expected (%#x, %d); keys %s, values %s"
                    % (what, len(keys), begin, end, i, int(gk[i]), int(gv[i]), int(ek[i]), int(ev[i]), "differ" if ik is not None else "equal",
                       "differ" if iv is not None else "equal"))
    return gk, gv


# ---- scan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", pc.SCAN_PATTERNS)
def test_scan_at_every_boundary(ctx, consts, pattern):
    for n in pc.scan_sizes(consts):
        values = pc.make_scan_values(pattern, n, consts)
        for in_place in (False, True):
            check_scan(ctx, values, in_place, "%s n=%d" % (pattern, n))


# ---- sort: sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["uniform", "three"])
def test_sort_at_every_boundary(ctx, consts, pattern):
    for n in pc.sort_sizes(consts):
        vals = pc.make_vals(n)
        for begin, end in pc.SIZE_RANGES:
            check_sort(ctx, pc.make_keys(pattern, n, begin, end), vals, begin, end, pattern)


@pytest.mark.parametrize("pattern", ["uniform", "three"])
def test_sort_whose_histogram_scan_takes_a_second_trip(ctx, consts, pattern):
    n = pc.sort_big_size(consts)
    assert 256 * -(-n // consts["RS_TILE"]) > consts["BLOCK"] * consts["SCAN_TILE"]
    vals = pc.make_vals(n)
    for begin, end in pc.SIZE_RANGES:
        check_sort(ctx, pc.make_keys(pattern, n, begin, end), vals, begin, end, pattern)


# ---- sort: bit ranges and key patterns ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", pc.KEY_PATTERNS)
def test_sort_every_bit_range(ctx, consts, pattern):
    for n in pc.sort_range_sizes(consts):
        vals = pc.make_vals(n)
        for begin, end in pc.BIT_RANGES:
            keys = pc.make_keys(pattern, n, begin, end)
            gk, gv = check_sort(ctx, keys, vals, begin, end, pattern)
            if end <= begin:
                assert gk.tobytes() == keys.tobytes() and gv.tobytes() == vals.tobytes()


@pytest.mark.parametrize("begin,end", pc.UNALIGNED_RANGES)
def test_sort_looks_at_its_bit_range_alone(ctx, consts, begin, end):
    """Keys that tie inside [begin_bit, end_bit) and differ above it keep their order: the last pass sorts the bits below end_bit,
    not its whole 8-bit digit."""
    for n in [63, consts["RS_TILE"] // 4 + 1] + pc.sort_range_sizes(consts):
        keys = pc.make_keys("dirty", n, begin, end)
        assert pc.dirty_pairs(keys, begin, end) >= n // 2
        check_sort(ctx, keys, pc.make_vals(n), begin, end, "dirty")


# ---- one context, many calls --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("begin,end", [(0, 64), (0, 37)])  # eight passes end in the caller's buffers, five in the alternate ones
def test_buffers_reused_across_sizes(consts, begin, end):
    rs, form = consts["RS_TILE"], consts["RS_TILE"] * consts["SCAN_ONE_MAX"] // 256 + 1
    sizes = [2 * rs + 1, form, rs // 4 + 1, form]
    calls = [(pc.make_keys("uniform", n, begin, end, seed=i), pc.make_vals(n, seed=i)) for i, n in enumerate(sizes)]
    assert calls[1][0].tobytes() != calls[3][0].tobytes()
    one = capi.Context(CONTIGS)
    try:
        got = [check_sort(one, k, v, begin, end, "call %d of one context" % i) for i, (k, v) in enumerate(calls)]
    finally:
        one.close()
    for i in (1, 3):  # a grown histogram and stale alternate buffers leak nothing: as on a context that never ran anything else
        fresh = capi.Context(CONTIGS)
        try:
            fk, fv = fresh.debug_radix_sort(calls[i][0], calls[i][1], begin, end)
        finally:
            fresh.close()
        assert fk.tobytes() == got[i][0].tobytes() and fv.tobytes() == got[i][1].tobytes(), i


def test_scan_between_two_sorts_changes_neither(ctx, consts):
    n = consts["RS_TILE"] * consts["SCAN_ONE_MAX"] // 256 + 1
    for begin, end in [(0, 37), (8, 24)]:
        ka, va = pc.make_keys("uniform", n, begin, end, seed=5), pc.make_vals(n, seed=5)
        kb, vb = pc.make_keys("bit63", n - 777, begin, end, seed=6), pc.make_vals(n - 777, seed=6)
        check_sort(ctx, ka, va, begin, end, "before the scan")
        for pattern in ("u32_wrap", "u64_wrap"):
            for in_place in (False, True):
                check_scan(ctx, pc.make_scan_values(pattern, consts["SCAN_ONE_MAX"] + 3 * consts["SCAN_TILE"] + 5, consts), in_place, "between sorts, " + pattern)
        check_sort(ctx, kb, vb, begin, end, "after the scan")
        check_scan(ctx, pc.make_scan_values("u32_wrap", 1000, consts), True, "after the sorts")
        check_sort(ctx, ka, va, begin, end, "the first again")


def test_same_call_twice_same_bytes(ctx, consts):
    n = consts["RS_TILE"] * consts["SCAN_ONE_MAX"] // 256 + 1
    for begin, end in [(0, 64), (0, 13)]:
        keys, vals = pc.make_keys("three", n, begin, end), pc.make_vals(n)
        a = ctx.debug_radix_sort(keys, vals, begin, end)
        b = ctx.debug_radix_sort(keys, vals, begin, end)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for pattern in ("u32_wrap", "u64_wrap"):
        values = pc.make_scan_values(pattern, consts["BLOCK"] * consts["SCAN_TILE"] + 1, consts)
        for in_place in (False, True):
            assert ctx.debug_scan(values, in_place).tobytes() == ctx.debug_scan(values, in_place).tobytes()


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_context_working(consts):
    c = capi.Context(CONTIGS)
    try:
        L, h = c.L, c.h
        k, v = pc.make_keys("uniform", 100, 0, 64), pc.make_vals(100)
        ko, vo = np.zeros(100, np.uint64), np.zeros(100, np.uint32)
        s32, so = np.ones(100, np.uint32), np.zeros(101, np.uint64)
        K, V, KO, VO, S, SO = (a.ctypes.data for a in (k, v, ko, vo, s32, so))
        for args in ((None, V, 100, 0, 64, KO, VO), (K, None, 100, 0, 64, KO, VO), (K, V, 100, 0, 64, None, VO), (K, V, 100, 0, 64, KO, None),
                     (K, V, 100, -1, 64, KO, VO), (K, V, 100, 0, 65, KO, VO), (K, V, 100, -8, 0, KO, VO)):
            assert L.bk_debug_radix_sort(h, *args) == abi.BK_ERR_ARG, args
        assert L.bk_debug_radix_sort(h, K, V, 0xFFFFFFF1, 0, 64, KO, VO) == abi.BK_ERR_LIMIT
        assert L.bk_debug_radix_sort(h, K, V, 1 << 40, 0, 8, KO, VO) == abi.BK_ERR_LIMIT
        assert b"2^32" in L.bk_last_error(h)
        for args in ((4, None, 100, 0, SO), (4, S, 100, 0, None), (8, None, 100, 1, SO), (3, S, 100, 0, SO), (0, S, 100, 0, SO), (16, S, 100, 1, SO)):
            assert L.bk_debug_scan(h, *args) == abi.BK_ERR_ARG, args
        assert L.bk_debug_prims_info(None) == abi.BK_ERR_ARG
        assert ko.tobytes() == bytes(800) and vo.tobytes() == bytes(400) and so.tobytes() == bytes(808)  # nothing was written
        # no items: nothing to point at, and nothing is an error
        assert L.bk_debug_radix_sort(h, None, None, 0, 0, 64, None, None) == abi.BK_OK
        assert c.debug_scan(np.zeros(0, np.uint32)).tolist() == [0] and c.debug_scan(np.zeros(0, np.uint64), in_place=True).tolist() == [0]
        # the context still works
        check_sort(c, k, v, 0, 64, "after the errors")
        check_scan(c, s32, False, "after the errors")
        with pytest.raises(capi.BreakIDError) as e:
            c.debug_radix_sort(k, v, 0, 65)
        assert e.value.code == abi.BK_ERR_ARG
    finally:
        c.close()

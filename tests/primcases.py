"""The two device-wide primitives of csrc/prims.h - exclusive_scan<u32|u64> and the stable LSD radix_sort_pairs - as plain numpy
definitions, with the sizes, bit ranges, key patterns and scan values at which they are pinned (tests/test_cpu_prims.py checks the
definitions themselves, tests/test_gpu_prims.py the kernels against them, byte for byte).  No GPU import here.

Every size follows from the four tile constants of the build (capi.prims_info(): BLOCK, SCAN_TILE, SCAN_ONE_MAX, RS_TILE), so a
change of a tile width moves the boundaries with it:
  scan  one workgroup up to SCAN_ONE_MAX elements, three launches above; the single block that scans the tile sums takes a second
        trip beyond BLOCK * SCAN_TILE elements
  sort  tiles of RS_TILE keys, RS_TILE / (BLOCK / 64) per wave; its histogram has 256 counters per tile and is scanned in place by
        the same code, so the sort changes scan form above RS_TILE * SCAN_ONE_MAX / 256 keys and reaches the second trip above
        RS_TILE * BLOCK * SCAN_TILE / 256 keys."""
import numpy as np

TODAY = {"BLOCK": 256, "SCAN_TILE": 2048, "SCAN_ONE_MAX": 32768, "RS_TILE": 2048}
U64 = (1 << 64) - 1


# ---- the definitions ----------------------------------------------------------------------------------------------------------------
def scan_reference(values):
    """out[0] = 0, out[i] = values[0] + .. + values[i-1] modulo 2^32 (uint32) or 2^64 (uint64), out[n] = the total"""
    values = np.asarray(values)
    assert values.dtype in (np.uint32, np.uint64)
    out = np.zeros(len(values) + 1, np.uint64)
    np.cumsum(values, dtype=np.uint64, out=out[1:])  # uint64 addition wraps at 2^64; n * 2^32 stays below it
    return out.astype(values.dtype)  # (uint64 -> uint32 keeps the low 32 bits)


def range_digits(keys, begin, end):
    """bits [begin, end) of every key, as a number"""
    keys = np.asarray(keys, np.uint64)
    if end <= begin:
        return np.zeros(len(keys), np.uint64)
    mask = np.uint64((1 << (end - begin)) - 1)  # a Python int first: 1 << 64 does not fit a uint64
    return (keys >> np.uint64(begin)) & mask


def sort_reference(keys, vals, begin, end):
    """(keys, vals) in the stable order of bits [begin, end) alone; end <= begin leaves them as they are"""
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.uint32)
    perm = np.argsort(range_digits(keys, begin, end), kind="stable")
    return keys[perm], vals[perm]


def first_difference(got, exp):
    """index of the first entry that differs (or of the first missing one), None when equal"""
    if len(got) != len(exp):
        return min(len(got), len(exp))
    d = np.flatnonzero(got != exp)
    return int(d[0]) if len(d) else None


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
def around(sizes):
    return sorted({m for n in sizes for m in (n - 1, n, n + 1) if m >= 0})


def scan_sizes(c=TODAY):
    block, tile, one = c["BLOCK"], c["SCAN_TILE"], c["SCAN_ONE_MAX"]
    return around([0, 1, 64, block, tile, one, 2 * tile + one, block * tile]) + [block * tile * 6 // 5 + 77]


def scan_tile_boundary(n, c=TODAY):
    """the last position of [0, n) at which one tile (or, in a short array, one block) ends and the next begins"""
    for step in (c["SCAN_TILE"], c["BLOCK"], 64, 2):
        if n > step:
            return (n - 1) // step * step
    return 0


def sort_sizes(c=TODAY):
    block, rs, one = c["BLOCK"], c["RS_TILE"], c["SCAN_ONE_MAX"]
    return around([0, 1, 64, rs // (block // 64), rs, 2 * rs, rs * one // 256])


def sort_big_size(c=TODAY):
    return c["RS_TILE"] * c["BLOCK"] * c["SCAN_TILE"] // 256 + 12345


def sort_range_sizes(c=TODAY):
    """where every bit range and key pattern is run: a partial second tile, and the first size whose histogram takes three launches"""
    return [c["RS_TILE"] + 1, c["RS_TILE"] * c["SCAN_ONE_MAX"] // 256 + 1]


# ---- bit ranges ---------------------------------------------------------------------------------------------------------------------
BIT_RANGES = [(0, 64), (32, 64), (0, 32), (0, 8), (0, 1), (0, 13), (0, 37), (8, 24), (5, 21), (56, 64), (60, 64), (7, 7), (9, 3)]
IDENTITY_RANGES = [(b, e) for b, e in BIT_RANGES if e <= b]
# ranges whose last 8-bit digit would reach beyond end_bit into bits that exist: there a key can differ above the range
UNALIGNED_RANGES = [(b, e) for b, e in BIT_RANGES if e > b and (e - b) % 8 and e < 64]
SIZE_RANGES = [(0, 64), (0, 13)]


# ---- keys and values ----------------------------------------------------------------------------------------------------------------
KEY_PATTERNS = ["uniform", "equal", "digits0", "digits255", "one_digit", "sorted", "reversed", "three", "bit63", "dirty"]


def _rng(*seed):
    return np.random.default_rng([20241019] + [int(s) for s in seed])


def _u64(rng, n):
    return rng.integers(0, U64, n, dtype=np.uint64, endpoint=True)


def make_keys(pattern, n, begin, end, seed=0):
    """n uint64 keys.  Every pattern but "dirty" (and bit 63 of "bit63") is zero above end_bit, so that it asks nothing of how the
    sort treats bits outside its range; below begin_bit the bits are random throughout.  An identity range is filled as (0, 64)."""
    if end <= begin:
        begin, end = 0, 64
    rng = _rng(KEY_PATTERNS.index(pattern), n, begin, end, seed)
    inside = ((1 << (end - begin)) - 1) << begin
    below = (1 << begin) - 1
    clean = np.uint64(inside | below)
    r = _u64(rng, n) & clean
    c = _u64(rng, 4) & clean
    if pattern == "uniform":
        k = r
    elif pattern == "equal":
        k = np.full(n, c[0], np.uint64)
    elif pattern == "digits0":
        k = r & np.uint64(below)
    elif pattern == "digits255":
        k = r | np.uint64(inside)
    elif pattern == "one_digit":
        field = np.uint64((0xFF << (begin + (end - begin - 1) // 8 // 2 * 8)) & inside)
        k = (c[0] & ~field) | (r & field)
    elif pattern in ("sorted", "reversed"):
        k = r[np.argsort(range_digits(r, begin, end), kind="stable")]
        if pattern == "reversed":
            k = k[::-1].copy()
    elif pattern == "three":
        k = c[:3][rng.integers(0, 3, n)]
    elif pattern == "bit63":
        k = r | np.uint64(1 << 63)
    elif pattern == "dirty":
        # a few values inside the range, so that many keys tie there; everything outside it random
        k = (c[rng.integers(0, 4, n)] & np.uint64(inside)) | (_u64(rng, n) & np.uint64(U64 ^ inside))
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(k, np.uint64)


def make_vals(n, seed=0):
    """random, not iota: a sort that numbers its output instead of carrying the values cannot pass"""
    return _rng(77, n, seed).integers(0, 1 << 32, n, dtype=np.uint32)


def dirty_pairs(keys, begin, end):
    """how many neighbours in the reference's output tie inside [begin, end) and differ above end_bit: the keys whose order only a
    sort that looks beyond end_bit would change"""
    ks, _ = sort_reference(keys, np.zeros(len(keys), np.uint32), begin, end)
    d = range_digits(ks, begin, end)
    above = ks >> np.uint64(end)
    return int(np.count_nonzero((d[1:] == d[:-1]) & (above[1:] != above[:-1])))


SCAN_PATTERNS = ["u32_ones", "u32_wrap", "u32_first", "u32_last", "u32_tile", "u64_wide", "u64_wrap"]


def make_scan_values(pattern, n, c=TODAY, seed=0):
    rng = _rng(1000 + SCAN_PATTERNS.index(pattern), n, seed)
    if pattern == "u32_ones":
        return np.ones(n, np.uint32)
    if pattern == "u32_wrap":  # mean 2^31: the total passes 2^32 about n / 2 times
        return rng.integers(0, 1 << 32, n, dtype=np.uint32)
    if pattern in ("u32_first", "u32_last", "u32_tile"):
        v = np.zeros(n, np.uint32)
        if n:
            v[{"u32_first": 0, "u32_last": n - 1, "u32_tile": scan_tile_boundary(n, c)}[pattern]] = 1
        return v
    if pattern == "u64_wide":  # below 2^40: totals far beyond 32 bits, never near 2^64
        return rng.integers(0, 1 << 40, n, dtype=np.uint64)
    if pattern == "u64_wrap":  # full width: the total passes 2^64 about n / 2 times
        return _u64(rng, n)
    raise KeyError(pattern)

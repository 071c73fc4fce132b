"""Shared cases of the site-complexity tests (test_cpu_complexity, test_gpu_complexity): the numpy definition of bk_site_complexity
(include/breakid_hip.h), vectorised over the sites; a deliberately naive brute force for one site; the twin files' fields; and
references built directly as nib-code arrays (homologycases.make_refseq) with planted tandem tracts, soft-masked intervals, contig
ends, segment gaps and N."""
import numpy as np

from breakid_amd import abi
from tests import homologycases as hc

NAMES = ["Lc_N", "Lc_GC", "Lc_Dust", "Lc_Tri", "Lc_Mask", "Lc_MaskRun", "Lc_BpUnit", "Lc_BpLen", "Lc_BpPos", "Lc_MaxUnit", "Lc_MaxLen", "Lc_MaxPos"]
COLUMNS = [name + str(side) for side in (1, 2) for name in NAMES]
W_OF_NIB = np.asarray([3, 1, 0, 2], np.int64)  # nib T C A G = 0 1 2 3 -> A C G T = 0 1 2 3


def as_sites(rows):
    """abi.REF_SITE from [(tid, pos)]"""
    out = np.zeros(len(rows), abi.REF_SITE)
    for k, r in enumerate(rows):
        out[k] = tuple(r)
    return out


def ref_nibbles(ref, tid, pos1):
    """(covered, the raw nibble) at the 1-based positions, on arrays that broadcast; the nibble is 0 where no segment holds the position"""
    tid, p0 = np.broadcast_arrays(np.asarray(tid, np.int64), np.asarray(pos1, np.int64) - 1)
    nib = np.zeros(p0.shape, np.int64)
    n = len(ref["tid"])
    if n == 0:
        return np.zeros(p0.shape, bool), nib
    st, ln, off = ref["start"].astype(np.int64), ref["len"].astype(np.int64), ref["off"].astype(np.int64)
    stid = ref["tid"].astype(np.int64)
    ok = (tid >= 0) & (p0 >= 0)
    g = np.searchsorted((stid << 33) | st, (np.where(ok, tid, 0) << 33) | np.where(ok, p0, 0), "right") - 1
    gi = np.clip(g, 0, n - 1)
    i = p0 - st[gi]
    hit = ok & (g >= 0) & (stid[gi] == tid) & (i < ln[gi])
    if len(ref["bases"]) == 0:
        return hit & False, nib
    byte = np.asarray(ref["bases"], np.int64)[np.where(hit, off[gi] + i // 2, 0)]
    nib[hit] = np.where(i & 1, byte & 15, byte >> 4)[hit]
    return hit, nib


def window_columns(ref, sites, flank):
    """(covered, valid, masked, w) of the contract, each [n, L]; w is 0 where the column is not valid"""
    R = int(flank)
    i = np.arange(2 * R + 1, dtype=np.int64)[None, :]
    covered, nib = ref_nibbles(ref, sites["tid"].astype(np.int64)[:, None], sites["pos"].astype(np.int64)[:, None] - R + i)
    valid = covered & ((nib & 4) == 0)
    masked = covered & ((nib & 8) != 0)
    return covered, valid, masked, np.where(valid, W_OF_NIB[nib & 3], 0)


def _tract_key(length, period, start):
    """the contract's order (-length, period, start) as one integer to maximise; every field is below 1024"""
    return (length * 1024 + (1023 - period)) * 1024 + (1023 - start)


def expected_cplx(ref, sites, flank, max_period):
    """the abi.SITE_CPLX rows of bk_site_complexity"""
    sites = np.ascontiguousarray(sites, abi.REF_SITE)
    n, R = len(sites), int(flank)
    L = 2 * R + 1
    out = np.zeros(n, abi.SITE_CPLX)
    if n == 0:
        return out
    covered, valid, masked, w = window_columns(ref, sites, flank)
    out["covered"], out["valid"], out["masked"] = covered.sum(1), valid.sum(1), masked.sum(1)
    out["gc"] = (valid & ((w == 1) | (w == 2))).sum(1)
    # mask_run: the columns from R up to the first unmasked one, and those below R down to the first unmasked one
    up = np.cumprod(masked[:, R:], axis=1).sum(1)
    down = np.cumprod(masked[:, :R][:, ::-1], axis=1).sum(1)
    out["mask_run"] = np.where(masked[:, R], up + down, 0)
    # trinucleotides
    if L >= 3:
        ok = valid[:, :-2] & valid[:, 1:-1] & valid[:, 2:]
        t = 16 * w[:, :-2] + 4 * w[:, 1:-1] + w[:, 2:]
        c = np.zeros((n, 64), np.int64)
        np.add.at(c, (np.nonzero(ok)[0], t[ok]), 1)
        out["tri_total"], out["tri_pairs"], out["tri_distinct"] = c.sum(1), (c * (c - 1) // 2).sum(1), (c > 0).sum(1)
    # tandem tracts: the runs of m_p as (site, start, end) from the steps of its padded difference
    best = np.zeros(n, np.int64)
    best_bp = np.zeros(n, np.int64)
    for p in range(1, min(int(max_period), L - 1) + 1):
        m = np.zeros((n, L - p + 2), np.int8)
        m[:, 1:-1] = valid[:, :-p] & valid[:, p:] & (w[:, :-p] == w[:, p:])
        step = np.diff(m, axis=1)
        site, start = np.nonzero(step == 1)
        _, end = np.nonzero(step == -1)  # (row-major order: the k-th end belongs to the k-th start)
        run = end - start
        keep = run >= p
        site, start, length = site[keep], start[keep], run[keep] + p
        key = _tract_key(length, p, start)
        np.maximum.at(best, site, key)
        touch = (start <= R + 1) & (start + length - 1 >= R - 1)
        np.maximum.at(best_bp, site[touch], key[touch])
    for name, key in (("bp", best_bp), ("max", best)):
        found = key > 0
        out[name + "_len"] = np.where(found, key >> 20, 0)
        out[name + "_period"] = np.where(found, 1023 - ((key >> 10) & 1023), 0)
        out[name + "_start"] = np.where(found, 1023 - (key & 1023), 0)
    return out


def brute_force(ref, site, flank, max_period):
    """one row, column by column and tract by tract, with no array arithmetic: for small windows"""
    tid, pos = int(site[0]), int(site[1])
    R = int(flank)
    L = 2 * R + 1
    nibs = []  # None where no segment holds the position
    for i in range(L):
        p0 = pos - R + i - 1
        found = None
        for g in range(len(ref["tid"])):
            s, ln = int(ref["start"][g]), int(ref["len"][g])
            if tid >= 0 and int(ref["tid"][g]) == tid and p0 >= 0 and s <= p0 < s + ln:
                byte = int(ref["bases"][int(ref["off"][g]) + (p0 - s) // 2])
                found = (byte & 15) if (p0 - s) & 1 else (byte >> 4)
        nibs.append(found)
    base = [None if x is None or x & 4 else "ACGT"[[3, 1, 0, 2][x & 3]] for x in nibs]
    row = np.zeros(1, abi.SITE_CPLX)[0]
    row["covered"] = sum(x is not None for x in nibs)
    row["valid"] = sum(b is not None for b in base)
    row["gc"] = sum(b in ("C", "G") for b in base)
    is_masked = [x is not None and bool(x & 8) for x in nibs]
    row["masked"] = sum(is_masked)
    if is_masked[R]:
        a = b = R
        while a > 0 and is_masked[a - 1]:
            a -= 1
        while b < L - 1 and is_masked[b + 1]:
            b += 1
        row["mask_run"] = b - a + 1
    counts = {}
    for i in range(L - 2):
        if None not in base[i:i + 3]:
            t = "".join(base[i:i + 3])
            counts[t] = counts.get(t, 0) + 1
    row["tri_total"] = sum(counts.values())
    row["tri_pairs"] = sum(c * (c - 1) // 2 for c in counts.values())
    row["tri_distinct"] = len(counts)
    tracts = []  # (-length, period, start)
    for p in range(1, max_period + 1):
        if p >= L:
            continue
        m = [base[i] is not None and base[i] == base[i + p] for i in range(L - p)]
        for i0 in range(len(m)):
            for n in range(p, len(m) - i0 + 1):
                if all(m[i0:i0 + n]) and (i0 == 0 or not m[i0 - 1]) and (i0 + n == len(m) or not m[i0 + n]):
                    tracts.append((-(n + p), p, i0))
    tracts.sort()
    if tracts:
        row["max_len"], row["max_period"], row["max_start"] = -tracts[0][0], tracts[0][1], tracts[0][2]
    at_bp = [t for t in tracts if any(R - 1 <= c <= R + 1 for c in range(t[2], t[2] - t[0]))]
    if at_bp:
        row["bp_len"], row["bp_period"], row["bp_start"] = -at_bp[0][0], at_bp[0][1], at_bp[0][2]
    return row


def ref_text(ref, tid, first, n):
    """n reference bases from the 1-based position `first`, upper case, N where the table has none"""
    covered, nib = ref_nibbles(ref, tid, first + np.arange(n))
    return "".join("TCAGNNNN"[int(x) & 7] if c else "N" for c, x in zip(covered, nib))


def twin_fields(ref, site, flank, row):
    """the twelve twin-file fields of one side; row None: the side was not submitted"""
    if row is None:
        return ["."] * 12
    v = {f: int(row[f]) for f in abi.SITE_CPLX.names if f != "reserved"}
    out = [str(v["valid"]), "%.3f" % (v["gc"] / v["valid"]) if v["valid"] else ".", "%.2f" % (v["tri_pairs"] / (v["tri_total"] - 1)) if v["tri_total"] >= 2 else ".",
           str(v["tri_distinct"]), "%.3f" % (v["masked"] / v["covered"]) if v["covered"] else ".", str(v["mask_run"])]
    first = int(site["pos"]) - int(flank)
    for name in ("bp", "max"):
        if v[name + "_len"]:
            at = first + v[name + "_start"]
            out += [ref_text(ref, int(site["tid"]), at, v[name + "_period"]), str(v[name + "_len"]), str(at)]
        else:
            out += [".", "0", "."]
    return out


def info_tail(fields):
    """what a breakend's INFO ends with, from the twelve fields of its side"""
    s = ""
    for key, at in (("LCDUST", 2), ("LCGC", 1), ("LCMASK", 4)):
        if fields[at] != ".":
            s += ";%s=%s" % (key, fields[at])
    if fields[6] != ".":
        s += ";LCSTR=%sx%s" % (fields[6], fields[7])
    return s


# ---- references as nib-code arrays ----------------------------------------------------------------------------------------------------
def text_ref(texts, masked=()):
    """a bk_refseq table of whole contigs from texts over ACGTN (lower case: soft-masked), tid = the place in the list"""
    segs = []
    for t, text in enumerate(texts):
        nib = hc.NIB_OF[np.asarray(["ACGTN".index(c) for c in text.upper()], np.int64)]
        nib = nib | (np.asarray([c.islower() for c in text]) * 8).astype(np.uint8)
        segs.append((t, 0, nib))
    return hc.make_refseq(segs)


def primitive_unit(rng, p):
    """p random bases (indices into "ACGT") that are no repeat of a shorter unit"""
    while True:
        u = rng.integers(0, 4, p)
        if not any(p % q == 0 and (u == np.tile(u[:q], p // q)).all() for q in range(1, p)):
            return u


_CASES = {}


def random_case(flank, n_sites, seed=None):
    """(ref, sites, plan) at one flank, computed once: every site has a random contig of 2 L + 40 bases of its own.  Every second site
    gets a planted tract (period 1 to 6, 24 to 60 columns wherever L >= 24, else what fits): of four in a row two over column R, one
    that ends in the window's last column and one that straddles a 64-column boundary of the window.  Of ten sites one has a window
    over a contig end, one a contig in two segments with a seven-base gap, one an N inside its tract; every third has a soft-masked
    interval around the breakpoint that crosses a word boundary of the window (every sixth: one that runs out of the window at both
    ends); the sites without a planted tract have stray N (in all four codes) and stray soft-masked bases.
    plan: arrays per site: planted, period, start, length (window columns), covers (column R), clean (the whole tract lies in the
    contig, off the gap and without N), last, straddles, contig_end, gap, has_n, masked_cross."""
    key = (flank, n_sites)
    if key in _CASES:
        return _CASES[key]
    R = int(flank)
    L = 2 * R + 1
    rng = np.random.default_rng(7000 + R if seed is None else seed)
    size = 2 * L + 40
    cut = size // 2
    plan = {f: np.zeros(n_sites, bool) for f in ("planted", "covers", "clean", "last", "straddles", "contig_end", "gap", "has_n", "masked_cross")}
    plan.update({f: np.zeros(n_sites, np.int64) for f in ("period", "start", "length")})
    segs, rows = [], []
    for k in range(n_sites):
        nib = hc.NIB_OF[rng.integers(0, 4, size)].copy()
        pos = int(rng.integers(R + 10, size - R - 10))  # 1-based centre, the window inside
        if k % 10 == 8:
            pos = int(rng.choice([rng.integers(1, R + 1), size - rng.integers(0, R)]))
            plan["contig_end"][k] = True
        first0 = pos - 1 - R  # the contig's 0-based index of column 0
        plan["gap"][k] = k % 10 == 4
        if k % 2 == 0:
            p = 1 + (k // 2) % 6 if L >= 24 else 1 + (k // 2) % max(1, min(6, L // 2))
            n = int(rng.integers(24, min(L, 60) + 1)) if L >= 24 else int(rng.integers(2 * p, L + 1))
            mode = (k // 2) % 4
            if mode <= 1:
                i0 = int(rng.integers(max(0, R - n + 1), min(R, L - n) + 1))
            elif mode == 2:
                i0 = L - n
            elif L > 64:
                b = 64 * int(rng.integers(1, (L - 1) // 64 + 1))
                i0 = int(np.clip(rng.integers(b - n + 1, b), 0, L - n))
            else:
                i0 = int(rng.integers(0, L - n + 1))
            unit = primitive_unit(rng, p)
            cols = np.arange(i0, i0 + n)
            at = first0 + cols
            inside = (at >= 0) & (at < size)
            nib[at[inside]] = hc.NIB_OF[unit[(cols % p)[inside]]]
            has_n = k % 10 == 2 and n >= 3
            if has_n:
                x = first0 + i0 + n // 2
                if 0 <= x < size:
                    nib[x] = 4 + int(rng.integers(0, 4))
                else:
                    has_n = False
            over_gap = bool(plan["gap"][k]) and bool(((at >= cut) & (at < cut + 7)).any())
            plan["planted"][k], plan["period"][k], plan["start"][k], plan["length"][k] = True, p, i0, n
            plan["covers"][k] = i0 <= R < i0 + n
            plan["last"][k] = i0 + n == L
            plan["straddles"][k] = i0 // 64 != (i0 + n - 1) // 64
            plan["has_n"][k] = has_n
            plan["clean"][k] = bool(inside.all()) and not has_n and not over_gap
        else:
            stray = rng.random(size) < 0.01
            nib[stray] = rng.integers(4, 8, int(stray.sum()))
            nib[rng.random(size) < 0.05] |= 8
        if k % 3 == 0:
            if k % 6 == 0:
                a, b = -3, L + 2
            elif L > 64:
                bnd = 64 * max(1, min((L - 1) // 64, int(round(R / 64.0))))
                a, b = min(R, bnd - 1) - int(rng.integers(0, 6)), max(R, bnd) + int(rng.integers(0, 6))
            else:
                a, b = R - int(rng.integers(0, min(R, 5) + 1)), R + int(rng.integers(0, min(R, 5) + 1))
            lo, hi = max(0, first0 + a), min(size - 1, first0 + b)
            if lo <= hi:
                nib[lo:hi + 1] |= 8
            plan["masked_cross"][k] = a // 64 != b // 64 or L <= 64
        if plan["gap"][k]:  # two segments with a gap between them, the second on an odd start
            segs += [(k, 0, nib[:cut]), (k, cut + 7, nib[cut + 7:])]
        else:
            segs.append((k, 0, nib))
        rows.append((k, pos))
    _CASES[key] = (hc.make_refseq(segs), as_sites(rows), plan)
    return _CASES[key]


def assert_plan(plan, L):
    """the shares random_case promises, on the reference side"""
    n = len(plan["planted"])
    planted = plan["planted"]
    assert planted.sum() * 5 >= 2 * n
    assert (plan["length"][planted] >= min(24, 2)).all() and (L < 24 or (plan["length"][planted] >= 24).all())
    assert ((plan["period"][planted] >= 1) & (plan["period"][planted] <= 6)).all()
    assert plan["covers"].sum() * 2 >= planted.sum()
    assert plan["last"].any() and (L <= 64 or plan["straddles"].any())
    if n >= 40:
        for f in ("contig_end", "gap"):
            assert plan[f].sum() * 10 >= n - 9, f
        assert L < 24 or plan["has_n"].sum() * 10 >= n - 9  # (a tract of two columns has no inside)
        assert plan["masked_cross"].sum() * 3 >= n - 2
        assert plan["clean"].sum() * 5 >= n  # (half are planted; a tenth each may lose theirs to an N, a contig end or the gap)

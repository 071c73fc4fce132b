"""Shared cases of the soft-clip tests (test_gpu_clip, test_cpu_clip): the numpy definition of bk_clip_support
(include/breakid_hip.h) over a record table, the rescue rule in Python, and the seeded and designed datasets."""
import numpy as np

from breakid_amd import abi, synth
from tests.callcases import CONTIGS, NAMES, designed_split

NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
LEFT, RIGHT = 0, 1
CLIP_TILE = 1024  # breakid_amd/csrc/clip.h: positions per tile of the kernel's window walk
OP_S, OP_H = 4, 5


def clip_events(cols, mapq_min, min_clip):
    """(tid, p, dir) of every clip event of the table, straight from the CIGAR words: for every record the first and the last
    op that is not H, found among all of its ops; the reference length summed over all of them"""
    n = len(cols["tid"])
    off = cols["cigar_off"].astype(np.int64)
    cig = cols["cigar"][:off[-1]].astype(np.int64)
    op, ln = cig & 15, cig >> 4
    aux_off = cols["aux_off"].astype(np.int64)
    flag = cols["flag"].astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    consumed = np.concatenate([[0], np.cumsum(np.where(np.isin(op, [0, 2, 3, 7, 8]), ln, 0))])
    reflen = consumed[off[1:]] - consumed[off[:-1]]
    elig = (cols["tid"] >= 0) & ((flag & NEVER) == 0) & (cols["mapq"].astype(np.int64) >= mapq_min) & (aux_off[1:] == aux_off[:-1]) & (reflen > 0)
    not_h = np.nonzero(op != OP_H)[0]
    c0, c1 = off[:-1], off[1:]
    if len(not_h) == 0:
        z = np.zeros(0, np.int64)
        return z.astype(np.int32), z, z
    a = np.searchsorted(not_h, c0, "left")          # first op at or behind c0 that is not H
    z = np.searchsorted(not_h, c1, "left") - 1      # last op before c1 that is not H
    first = not_h[np.minimum(a, len(not_h) - 1)]
    last = not_h[np.maximum(z, 0)]
    has = (a < len(not_h)) & (first < c1) & (z >= 0) & (last >= c0)
    first, last = np.where(has, first, 0), np.where(has, last, 0)
    if len(cig) == 0:
        lead = trail = np.zeros(n, bool)
    else:
        lead = elig & has & (op[first] == OP_S) & (ln[first] >= min_clip)
        trail = elig & has & (op[last] == OP_S) & (ln[last] >= min_clip)
    tid = np.concatenate([cols["tid"][lead], cols["tid"][trail]]).astype(np.int32)
    p = np.concatenate([pos[lead] + 1, (pos + reflen)[trail]])
    d = np.concatenate([np.full(int(lead.sum()), RIGHT, np.int64), np.full(int(trail.sum()), LEFT, np.int64)])
    return tid, p, d


def expected_clip_support(cl, cols, mapq_min, min_clip, w):
    W = int(w)  # (int) w, truncation toward zero like the C conversion
    out = np.zeros(len(cl), abi.CLIP_SUPPORT)
    tid, p, d = clip_events(cols, mapq_min, min_clip)
    by = {}
    for key in set(zip(tid.tolist(), d.tolist())):
        by[key] = np.sort(p[(tid == key[0]) & (d == key[1])])
    for i, c in enumerate(cl):
        voted = bool(c["flags"] & 2)
        for s in (0, 1):
            T = int(c["p%d_tid" % (s + 1)])
            if T < 0:
                continue
            lo = max(1, int(c["p%d_min" % (s + 1)]) - W)
            hi = int(c["p%d_max" % (s + 1)]) + W
            e = int(c["p%d_exact" % (s + 1)])
            for dr in (LEFT, RIGHT):
                ps = by.get((T, dr))
                if ps is None:
                    continue
                inw = ps[np.searchsorted(ps, lo, "left"):np.searchsorted(ps, hi, "right")]
                out["events"][i, s, dr] = len(inw)
                if len(inw):
                    vals, counts = np.unique(inw, return_counts=True)
                    k = int(np.argmax(counts))  # the first of the largest: vals ascend, so the smallest p
                    out["peak_n"][i, s, dr] = counts[k]
                    out["peak_pos"][i, s, dr] = vals[k]
                if voted:
                    out["at"][i, s, dr] = int(np.searchsorted(ps, e + 2, "right") - np.searchsorted(ps, e - 2, "left"))
    return out


def junction_sides(j):
    """bk_junction_sides in Python: (d1, d2)"""
    for v in (j["splits"], j["pairs"]):
        if np.any(v):
            k = int(np.argmax(v))
            return k >> 1, k & 1
    return 0, 1


def expected_rescue(c, j, s, min_support):
    if c["flags"] & 2 or c["p1_tid"] < 0 or c["p2_tid"] < 0:
        return None
    d1, d2 = junction_sides(j)
    if int(s["peak_n"][0][d1]) < min_support or int(s["peak_n"][1][d2]) < min_support:
        return None
    return int(s["peak_pos"][0][d1]), int(s["peak_pos"][1][d2]), int(s["peak_n"][0][d1]), int(s["peak_n"][1][d2])


# ---- a seeded sample: clipped background --------------------------------------------------------------------------------------
def _clip(rng, pair, j, lo=5, hi=40):
    """a soft clip of lo..hi bases on a random end of read j of a pair of 100M reads; the aligned bases stay where they are"""
    k = int(rng.integers(lo, hi + 1))
    r = pair[j]
    if rng.integers(0, 2):
        r.cigar = "%dS%dM" % (k, 100 - k)
        r.pos += k
        pair[1 - j].mpos = r.pos
    else:
        r.cigar = "%dM%dS" % (100 - k, k)


# (ta, pa, tb, pb, split reads)
CLIPPED_LOCI = [(0, 300_000, 1, 700_000, 6), (2, 400_000, 2, 1_200_000, 6), (1, 1_500_000, 3, 250_000, 0), (0, 1_700_000, 2, 900_000, 0), (3, 1_200_000, 0, 1_000_000, 6)]


def clipped_tumor(seed=29, n_background=12000, n_local=300):
    """12 000 background pairs and, around every locus, local pairs; a seeded tenth of the background reads and three tenths of the
    local ones carry a clip of 5-40 bases on a random end.  Loci with and without split reads: voted and unvoted rows."""
    rng = np.random.default_rng(seed)
    ds = synth.Dataset(list(CONTIGS))
    k = 0
    for i in range(n_background):
        pr = synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40, prefix="cb")
        for j in (0, 1):
            if rng.random() < 0.1:
                _clip(rng, pr, j)
        ds.recs += pr
    for li, (ta, pa, tb, pb, n_split) in enumerate(CLIPPED_LOCI):
        for j in range(14):
            ds.recs += synth._discordant_pair("cD%d_%d" % (li, j), ta, pa + int(rng.integers(-300, 301)), tb, pb + int(rng.integers(-300, 301)), 100, False, True)
        for j in range(n_split):
            ds.recs += synth._split_pair("cS%d_%d" % (li, j), NAMES, ta, pa + 30, tb, pb + 30, 60, 40)
        for t, p in ((ta, pa), (tb, pb)):
            for j in range(n_local):
                pr = synth._proper_pair(rng, k, t, p - 2000, p + 2000, 100, 350, 40, prefix="cl")
                k += 1
                for jj in (0, 1):
                    if rng.random() < 0.3:
                        _clip(rng, pr, jj)
                ds.recs += pr
    ds.sort()
    return ds


# ---- designed truth -----------------------------------------------------------------------------------------------------------
# (name, ta, bpa, da, tb, bpb, db): the first four sit where callcases.designed_refgene puts a gene on either side
CLIP_LOCI = [("a", 0, 300_000, "L", 1, 700_000, "R"), ("b", 0, 600_000, "L", 2, 500_000, "L"), ("f", 1, 300_000, "R", 3, 900_000, "R"),
             ("d", 2, 900_000, "R", 3, 400_000, "L"), ("c", 0, 1_000_000, "L", 0, 1_400_000, "R"), ("e", 1, 1_000_000, "L", 1, 1_400_000, "L")]
# clipped reads without an SA tag per side: (on side A, on side B, in the direction of the pairs)
CLIP_READS = {"a": (5, 5, True), "b": (6, 6, True), "c": (0, 0, True), "d": (6, 0, True), "e": (6, 6, False), "f": (2, 2, True)}
CLIP_SPLITS = {"a": 8}


def clipped_read(q, t, bp, d, m=60, s=40):
    """a read without an SA tag whose aligned bases end at 1-based bp (d = 'L': mM sS) or start at it ('R': sS mM), and its plain mate"""
    if d == "L":
        pos, cigar = bp - m, "%dM%dS" % (m, s)
    else:
        pos, cigar = bp - 1, "%dS%dM" % (s, m)
    return [synth.Rec(q, 0x1 | 0x2 | 0x40 | 0x20, t, pos, 60, cigar, t, pos + 200, 300), synth.Rec(q, 0x1 | 0x2 | 0x80 | 0x10, t, pos + 200, 60, "100M", t, pos, -300)]


def clip_tumor(n_proper=12000):
    """Background; per locus 14 discordant pairs whose strands say on which side of each breakpoint the retained sequence lies, the
    split reads of CLIP_SPLITS and the clipped reads of CLIP_READS."""
    rng = np.random.default_rng(41)
    ds = synth.Dataset(list(CONTIGS))
    for i in range(n_proper):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, len(CONTIGS))), 1000, 1_999_000, 100, 350, 40)
    other = {"L": "R", "R": "L"}
    for name, ta, bpa, da, tb, bpb, db in CLIP_LOCI:
        for j in range(14):
            oa = -int(rng.integers(100, 400)) if da == "L" else int(rng.integers(0, 300))
            ob = -int(rng.integers(100, 400)) if db == "L" else int(rng.integers(0, 300))
            ds.recs += synth._discordant_pair("%sD_%d" % (name, j), ta, bpa + oa, tb, bpb + ob, 100, rev_a=(da == "R"), rev_b=(db == "R"))
        for j in range(CLIP_SPLITS.get(name, 0)):
            ds.recs += designed_split("%sS_%d" % (name, j), ta, bpa, da, tb, bpb, db)
        na, nb, along = CLIP_READS[name]
        for j in range(na):
            ds.recs += clipped_read("%sCa_%d" % (name, j), ta, bpa, da if along else other[da])
        for j in range(nb):
            ds.recs += clipped_read("%sCb_%d" % (name, j), tb, bpb, db if along else other[db])
    ds.sort()
    return ds


def locus_of(c, loci=CLIP_LOCI, tol=2000):
    """(locus, True when side 1 of the row is side A of the locus), or (None, None)"""
    for L in loci:
        _, ta, bpa, _, tb, bpb, _ = L
        if (c["p1_tid"], c["p2_tid"]) == (ta, tb) and abs(int(c["p1_mean"]) - bpa) < tol and abs(int(c["p2_mean"]) - bpb) < tol:
            return L, True
        if (c["p1_tid"], c["p2_tid"]) == (tb, ta) and abs(int(c["p1_mean"]) - bpb) < tol and abs(int(c["p2_mean"]) - bpa) < tol:
            return L, False
    return None, None

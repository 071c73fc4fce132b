"""Shared cases of the unique-support tests (test_gpu_dedup, test_cpu_dedup): the numpy definition of bk_unique_support
(include/breakid_hip.h) on top of that of bk_evidence, and the designed datasets: known duplicates, fragments whose keys differ in
one field alone, and one call deeper than any tile of the implementation."""
import numpy as np

from breakid_amd import abi, synth
from tests import callcases as cc
from tests.test_gpu_evidence import expected_evidence

UNIQUE_TILE = 64    # breakid_amd/csrc/unique.h: sorted rows a wavefront looks at per step
RADIX_TILE = 2048   # breakid_amd/csrc/prims.h, RS_TILE: keys per workgroup of a radix pass
PAIR_FIELDS = ("p1_pos", "p2_pos", "p1_rev", "p2_rev")
SPLIT_FIELDS = ("A1_start", "A1_end", "A2_start", "A2_end", "mtid", "mpos")


# ---- the definition, in numpy -----------------------------------------------------------------------------------------------
def fragment_keys(cl, clustered, splits, cols):
    """(rows, call_off, keys): bk_evidence's rows by its own definition and the fragment key of each as a tuple of Python ints.
    The stage rows behind the evidence rows are found again by the rule of expected_evidence and checked against its rows."""
    rows, off = expected_evidence(cl, clustered, splits, cols["qhash"], cols.get("qcheck"), cols["mapq"])
    member = (clustered["group"].astype(np.int64) << 32) | (clustered["cluster"].astype(np.int64) & 0xFFFFFFFF)
    ok_sp = (splits["flags"] & 2) == 0
    pb, sb = splits["prim_bp"].astype(np.int64), splits["sec_bp"].astype(np.int64)
    keys = []
    for i, c in enumerate(cl):
        r0 = len(keys)
        p = clustered[np.flatnonzero(member == ((int(c["group"]) << 32) | (int(c["id"]) & 0xFFFFFFFF)))]
        assert np.array_equal(p["rec"], rows["rec"][r0:r0 + len(p)]) and np.all(rows["kind"][r0:r0 + len(p)] == abi.EV_PAIR)
        keys += [(int(a), int(b), int(x != 0), int(y != 0)) for a, b, x, y in zip(p["p1_pos"], p["p2_pos"], p["p1_rev"], p["p2_rev"])]
        if c["flags"] & 2:
            e1, e2 = int(c["p1_exact"]), int(c["p2_exact"])
            t1, t2 = int(c["p1_tid"]), int(c["p2_tid"])
            own = ((splits["tid"] == t1) | (splits["tid"] == t2)) & ok_sp
            f1 = own & (splits["prim_chr"] == t1) & (splits["sec_chr"] == t2) & (np.abs(pb - e1) <= 2) & (np.abs(sb - e2) <= 2)
            f2 = own & ~f1 & (splits["prim_chr"] == t2) & (splits["sec_chr"] == t1) & (np.abs(pb - e2) <= 2) & (np.abs(sb - e1) <= 2)
            t = np.flatnonzero(f1 | f2)
            r1 = len(keys)
            assert np.array_equal(splits["rec"][t], rows["rec"][r1:r1 + len(t)]) and np.array_equal(f2[t], rows["flag2"][r1:r1 + len(t)] != 0)
            for j in t:
                s = splits[j]
                a = (int(s["prim_start"]), int(s["prim_end"]))
                b = (int(s["sec_start"]), int(s["sec_end"]))
                rec = int(s["rec"])
                keys.append((b + a if f2[j] else a + b) + (int(cols["mtid"][rec]), int(cols["mpos"][rec])))
        assert len(keys) == int(off[i + 1])
    return rows, off, keys


def expected_unique_support(cl, clustered, splits, cols):
    """(rows, first); cols: the columns of the context's table"""
    ev, off, keys = fragment_keys(cl, clustered, splits, cols)
    out = np.zeros(len(cl), abi.UNIQUE_SUPPORT)
    first = np.zeros(len(ev), np.uint64)
    for c in range(len(cl)):
        seen, size = {}, {}
        for r in range(int(off[c]), int(off[c + 1])):
            k = (int(ev["kind"][r]),) + keys[r]
            f = seen.setdefault(k, r)
            first[r] = f
            size[f] = size.get(f, 0) + 1
        for kind, u, t in ((abi.EV_PAIR, "uniq_pairs", "top_pairs"), (abi.EV_SPLIT, "uniq_splits", "top_splits")):
            sizes = [n for f, n in size.items() if ev["kind"][f] == kind]
            out[c][u], out[c][t] = len(sizes), max(sizes, default=0)
    return out, first


def fields_differing_alone(cl, clustered, splits, cols):
    """names of the key fields in which two fragments of one call and kind differ while every other field is equal"""
    ev, off, keys = fragment_keys(cl, clustered, splits, cols)
    found = set()
    for c in range(len(cl)):
        for kind, names in ((abi.EV_PAIR, PAIR_FIELDS), (abi.EV_SPLIT, SPLIT_FIELDS)):
            ks = sorted({keys[r] for r in range(int(off[c]), int(off[c + 1])) if ev["kind"][r] == kind})
            for i, a in enumerate(ks):
                for b in ks[i + 1:]:
                    d = [n for n, x, y in zip(names, a, b) if x != y]
                    if len(d) == 1:
                        found.add(d[0])
    return found


def check_invariants(ev, off, rows, first):
    """class sizes sum to the row counts, first[first[r]] == first[r] <= r, a call with pair rows has a pair fragment"""
    f = first.astype(np.int64)
    assert len(f) == len(ev) == int(off[-1]) and len(rows) == len(off) - 1
    assert np.all(f <= np.arange(len(f))) and np.array_equal(f[f], f)
    assert np.array_equal(ev["call"][f], ev["call"]) and np.array_equal(ev["kind"][f], ev["kind"])
    heads = f == np.arange(len(f))
    size = np.bincount(f, minlength=len(f))
    for c in range(len(rows)):
        a, b = int(off[c]), int(off[c + 1])
        for kind, u, t in ((abi.EV_PAIR, "uniq_pairs", "top_pairs"), (abi.EV_SPLIT, "uniq_splits", "top_splits")):
            m = ev["kind"][a:b] == kind
            h = heads[a:b] & m
            assert int(rows[c][u]) == int(h.sum()) and int(size[a:b][h].sum()) == int(m.sum())
            assert int(rows[c][t]) == (int(size[a:b][h].max()) if h.any() else 0)
        assert rows[c]["uniq_pairs"] >= 1  # (a cluster has member pairs)


# ---- designed datasets --------------------------------------------------------------------------------------------------------
SPLIT_COPIES = ((50, 1), (55, 1), (60, 3), (65, 1), (70, 2))  # (m1, copies): 8 reads, 16 tuples, 5 fragments, the largest of 6 tuples
PAIR_COPIES = (1, 1, 4, 1, 1, 2, 1, 1, 1, 1)                  # ten pairs at staggered offsets: 14 read pairs


def pair_offsets(j, da, db):
    oa = -(120 + 23 * j) if da == "L" else 15 + 23 * j
    ob = -(110 + 17 * j) if db == "L" else 25 + 17 * j
    return oa, ob


def background(ds, n, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, len(ds.contigs))), 1000, 1_999_000, 100, 350, 40)


def add_locus(ds, locus, split_copies=SPLIT_COPIES, pair_copies=PAIR_COPIES):
    name, ta, bpa, da, tb, bpb, db = locus
    for j, copies in enumerate(pair_copies):
        oa, ob = pair_offsets(j, da, db)
        for k in range(copies):  # the same alignments under another read name: a PCR duplicate nobody marked
            ds.recs += synth._discordant_pair("%sD_%d_%d" % (name, j, k), ta, bpa + oa, tb, bpb + ob, 100, rev_a=(da == "R"), rev_b=(db == "R"))
    for m1, copies in split_copies:
        for k in range(copies):
            ds.recs += cc.designed_split("%sS_%d_%d" % (name, m1, k), ta, bpa, da, tb, bpb, db, m1, 100 - m1)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        ds = make()
        ds.sort()
        _CACHE[key] = (ds, ds.to_soa())
    return _CACHE[key]


def dedup_tumor():
    """the eight designed loci of callcases, every one with the same known duplicates"""
    def make():
        ds = synth.Dataset(list(cc.CONTIGS))
        background(ds, 12000, 5)
        for locus in cc.LOCI:
            add_locus(ds, locus)
        return ds
    return _cached("dedup", make)


NEAR = cc.LOCI[0]
NEAR_REQUIRED = {"p2_pos", "mpos", "A2_end"}


def near_key_tumor():
    """One call whose fragments come in pairs that differ in one key field alone: pairs whose second read starts 3 bp further on
    (p2_pos) or whose first does (p1_pos); a split read with the same two alignments and another mate (mpos); one with the same
    own alignment and a partner that is 5 bases longer at its far end (A2_end: the side assignment of the call makes the partner
    side 2 here).  Each of them is there twice, so the near neighbours must stay apart while the true copies merge."""
    def make():
        name, ta, bpa, da, tb, bpb, db = NEAR
        assert (da, db) == ("L", "R")
        ds = synth.Dataset(list(cc.CONTIGS))
        background(ds, 12000, 9)
        add_locus(ds, NEAR, split_copies=((50, 1), (70, 1)), pair_copies=(1,) * 8)
        oa, ob = pair_offsets(3, da, db)
        for k in range(2):
            ds.recs += synth._discordant_pair("NKD_p2_%d" % k, ta, bpa + oa, tb, bpb + ob + 3, 100, rev_a=False, rev_b=True)
            ds.recs += synth._discordant_pair("NKD_p1_%d" % k, ta, bpa + oa + 3, tb, bpb + ob, 100, rev_a=False, rev_b=True)
            ds.recs += cc.designed_split("NKS_base_%d" % k, ta, bpa, da, tb, bpb, db, 60, 40)
            moved = cc.designed_split("NKS_mate_%d" % k, ta, bpa, da, tb, bpb, db, 60, 40)
            moved[0].mpos += 7
            moved[1].mpos += 7
            moved[2].pos += 7
            ds.recs += moved
            ds.recs += cc.designed_split("NKS_far_%d" % k, ta, bpa, da, tb, bpb, db, 60, 45)
        return ds
    return _cached("near", make)


DEEP = ("DEEP", 0, 800_000, "L", 2, 1_100_000, "R")
DEEP_COPIES = RADIX_TILE + 2 * UNIQUE_TILE + 37  # of one pair; of one split read half of it (a read gives two tuples) and a few more
DEEP_DISTINCT = 41


def deep_tumor():
    """One locus (for -fast) with more rows of each kind than a radix tile and than many steps of the run walk hold: one pair
    and one split read copied until their fragment spans those borders, DEEP_DISTINCT other pairs and split reads around them."""
    def make():
        name, ta, bpa, da, tb, bpb, db = DEEP
        ds = synth.Dataset(list(cc.CONTIGS))
        background(ds, 12000, 13)
        add_locus(ds, DEEP, split_copies=tuple((m1, DEEP_COPIES // 2 + 40 if m1 == 57 else 1) for m1 in range(30, 30 + DEEP_DISTINCT)),
                  pair_copies=tuple(DEEP_COPIES if j == 4 else 1 for j in range(12)))
        return ds
    return _cached("deep", make)


def deep_rows_expected(rows):
    """the deep call's own condition: both kinds straddle the tiles, and one fragment of each does"""
    c = rows[np.argmax(rows["top_pairs"])]
    assert c["top_pairs"] > RADIX_TILE + UNIQUE_TILE and c["uniq_pairs"] >= 4, c
    assert c["top_splits"] > RADIX_TILE + UNIQUE_TILE and c["uniq_splits"] >= DEEP_DISTINCT - 2, c

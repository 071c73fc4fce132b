"""Split junctions (`bk_split_junctions`, `-junctions`): two independent statements of the definition in include/breakid_hip.h, both
starting from the BK_STAGE_SPLITS table plus the flag and mapq columns of the records; the case builders; how the command line
prints a row.  `expected` is brute force: Python per tuple, all-pairs near, union-find.  `expected_sweep` is numpy: a lexsort, run
boundaries, a window sweep with a flood fill."""
import numpy as np

from breakid_amd import abi, synth

MAX_TOL = 100
FIELDS = ("tid1", "pos1", "tid2", "pos2", "n_reads", "n_tuples", "n_exact", "lo1", "hi1", "lo2", "hi2", "n_own", "mapq_sum", "call", "right1", "right2", "call_crossed", "reserved",
          "top_reads")


# ---- statement 1: brute force ----------------------------------------------------------------------------------------------------------
def tuple_ends(s):
    """(own end, other end) of one SPLIT row, each (contig, pos, right)"""
    own, oth = ("sec", "prim") if int(s["flags"]) & 1 else ("prim", "sec")
    return ((int(s["tid"]), int(s[own + "_bp"]), int(s[own + "_bp"] == s[own + "_start"])),
            (int(s[oth + "_chr"]), int(s[oth + "_bp"]), int(s[oth + "_bp"] == s[oth + "_start"])))


def why_dropped(s, flag, mapq, tlen, mapq_min):
    """None for an eligible tuple, else the name of the first rule that drops it"""
    a, b = tuple_ends(s)
    nt = len(tlen)
    if int(s["flags"]) & 2:
        return "poison"
    if a[0] < 0 or a[0] >= nt:
        return "own_contig"
    if not 0 <= b[0] < nt:
        return "other_contig"
    if not 1 <= a[1] <= int(tlen[a[0]]) or not 1 <= b[1] <= int(tlen[b[0]]):
        return "position"
    r = int(s["rec"])
    if int(flag[r]) & 0x4:
        return "unmapped"
    if int(flag[r]) & 0x200:
        return "qcfail"
    if int(mapq[r]) < mapq_min:
        return "mapq"
    if a == b:
        return "identical"
    return None


def canonical(s):
    """(end 1, end 2, own_end)"""
    a, b = tuple_ends(s)
    return (a, b, 0) if a < b else (b, a, 1)


def order_key(k):
    """the order of the exact junctions: (tid1, tid2, right1, right2, pos1, pos2); k = (tid1, pos1, right1, tid2, pos2, right2)"""
    return (k[0], k[3], k[2], k[5], k[1], k[4])


def is_near(a, b, tol):
    return (a[0], a[3], a[2], a[5]) == (b[0], b[3], b[2], b[5]) and abs(a[1] - b[1]) <= tol and abs(a[4] - b[4]) <= tol


def voted_rows(clusters):
    return [] if clusters is None else [(i, int(c["p1_tid"]), int(c["p1_exact"]), int(c["p2_tid"]), int(c["p2_exact"])) for i, c in enumerate(clusters) if int(c["flags"]) & 2]


def matches(k, row):
    """(straight, crossed) of exact junction k against a voted row"""
    _, t1, e1, t2, e2 = row
    return (k[0] == t1 and abs(k[1] - e1) <= 2 and k[3] == t2 and abs(k[4] - e2) <= 2,
            k[0] == t2 and abs(k[1] - e2) <= 2 and k[3] == t1 and abs(k[4] - e1) <= 2)


def exact_table(splits, flag, mapq, tlen, mapq_min):
    """{exact junction: [(qhash, own_end, mapq)]}"""
    table = {}
    for s in splits:
        if why_dropped(s, flag, mapq, tlen, mapq_min) is None:
            e1, e2, own_end = canonical(s)
            table.setdefault(e1 + e2, []).append((int(s["qhash"]), own_end, int(mapq[int(s["rec"])])))
    return table


def expected(splits, flag, mapq, tlen, mapq_min, tol, min_reads, clusters=None, info=None):
    table = exact_table(splits, flag, mapq, tlen, mapq_min)
    keys = sorted(table, key=order_key)
    x = len(keys)
    parent = list(range(x))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    if x:
        arr = np.asarray(keys, np.int64)
        for i in range(x):
            m = ((arr[i + 1:, [0, 3, 2, 5]] == arr[i, [0, 3, 2, 5]]).all(axis=1) & (np.abs(arr[i + 1:, 1] - arr[i, 1]) <= tol) & (np.abs(arr[i + 1:, 4] - arr[i, 4]) <= tol))
            for j in np.flatnonzero(m) + i + 1:
                assert is_near(keys[i], keys[j], tol)
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    calls = {}
    for j in range(x):
        calls.setdefault(find(j), []).append(j)
    voted = voted_rows(clusters)
    rows = np.zeros(len(calls), abi.SPLIT_JUNCTION)
    for r, root in zip(rows, sorted(calls)):
        members = calls[root]
        assert members[0] == root
        reads = lambda j: len({q for q, _, _ in table[keys[j]]})  # noqa: E731
        rep = min(members, key=lambda j: (-reads(j), j))
        tup = [t for j in members for t in table[keys[j]]]
        k = keys[rep]
        r["tid1"], r["pos1"], r["right1"], r["tid2"], r["pos2"], r["right2"] = k
        r["n_reads"] = len({q for q, _, _ in tup})
        r["n_tuples"] = len(tup)
        r["n_exact"] = len(members)
        r["lo1"], r["hi1"] = min(keys[j][1] for j in members), max(keys[j][1] for j in members)
        r["lo2"], r["hi2"] = min(keys[j][4] for j in members), max(keys[j][4] for j in members)
        for e in (0, 1):
            r["n_own"][e] = sum(1 for _, o, _ in tup if o == e)
            r["mapq_sum"][e] = sum(mq for _, o, mq in tup if o == e)
        r["top_reads"] = reads(rep)
        r["call"] = -1
        for row in voted:
            hits = [matches(keys[j], row) for j in members]
            if any(s or c for s, c in hits):
                r["call"] = row[0]
                r["call_crossed"] = 0 if any(s for s, _ in hits) else 1
                break
    if info is not None:
        info.update(eligible=sum(len(v) for v in table.values()), exact=x, calls=len(rows), keys=keys, members=[calls[c] for c in sorted(calls)])
    return rows[rows["n_reads"] >= min_reads].copy()


# ---- statement 2: a sorted sweep -------------------------------------------------------------------------------------------------------
def expected_sweep(splits, flag, mapq, tlen, mapq_min, tol, min_reads, clusters=None):
    s = splits
    nt = len(tlen)
    tl = np.asarray(tlen, np.int64)
    sec = (s["flags"] & 1) != 0
    pick = lambda a, b: np.where(sec, s[a], s[b]).astype(np.int64)  # noqa: E731
    own_t = s["tid"].astype(np.int64)
    own_p, own_s = pick("sec_bp", "prim_bp"), pick("sec_start", "prim_start")
    oth_t, oth_p, oth_s = pick("prim_chr", "sec_chr"), pick("prim_bp", "sec_bp"), pick("prim_start", "sec_start")
    own_r, oth_r = (own_p == own_s).astype(np.int64), (oth_p == oth_s).astype(np.int64)
    rec = s["rec"].astype(np.int64)
    ok = ((s["flags"] & 2) == 0) & (own_t >= 0) & (own_t < nt) & (oth_t >= 0) & (oth_t < nt)
    len_of = lambda t: tl[np.clip(t, 0, max(nt - 1, 0))] if nt else np.zeros(len(t), np.int64)  # noqa: E731
    ok &= (own_p >= 1) & (own_p <= len_of(own_t)) & (oth_p >= 1) & (oth_p <= len_of(oth_t))
    f = np.asarray(flag, np.int64)[rec] if len(s) else np.zeros(0, np.int64)
    mq = np.asarray(mapq, np.int64)[rec] if len(s) else np.zeros(0, np.int64)
    ok &= ((f & 0x204) == 0) & (mq >= mapq_min)
    ok &= ~((own_t == oth_t) & (own_p == oth_p) & (own_r == oth_r))
    own_first = (own_t < oth_t) | ((own_t == oth_t) & ((own_p < oth_p) | ((own_p == oth_p) & (own_r < oth_r))))
    sel = lambda a, b: np.where(own_first, a, b)[ok]  # noqa: E731
    t1, p1, r1, t2, p2, r2 = sel(own_t, oth_t), sel(own_p, oth_p), sel(own_r, oth_r), sel(oth_t, own_t), sel(oth_p, own_p), sel(oth_r, own_r)
    own_end, mq, qh = (~own_first[ok]).astype(np.int64), mq[ok], s["qhash"][ok]
    e = len(t1)
    if e == 0:
        return np.zeros(0, abi.SPLIT_JUNCTION)
    order = np.lexsort((qh, p2, p1, r2, r1, t2, t1))
    t1, p1, r1, t2, p2, r2, own_end, mq, qh = (a[order] for a in (t1, p1, r1, t2, p2, r2, own_end, mq, qh))
    K = np.stack([t1, t2, r1, r2, p1, p2], axis=1)
    head = np.concatenate([[True], (K[1:] != K[:-1]).any(axis=1)])
    start = np.flatnonzero(head)
    end = np.concatenate([start[1:], [e]])
    X = K[start]
    x = len(X)
    qhead = head | np.concatenate([[True], qh[1:] != qh[:-1]])
    xreads = np.add.reduceat(qhead.astype(np.int64), start)
    # components: a flood fill over the windows of the sorted table
    grp = np.concatenate([[0], np.cumsum((X[1:, :4] != X[:-1, :4]).any(axis=1))])
    span = int(X[:, 4].max()) + 2 * MAX_TOL + 2
    lin = grp * span + X[:, 4]  # ascending: the table is sorted by (group, pos1)
    lo, hi = np.searchsorted(lin, lin - tol, "left"), np.searchsorted(lin, lin + tol, "right")
    comp = np.full(x, -1, np.int64)
    for j in range(x):
        if comp[j] >= 0:
            continue
        comp[j] = j
        stack = [j]
        while stack:
            v = stack.pop()
            w = np.arange(lo[v], hi[v])
            w = w[(np.abs(X[w, 5] - X[v, 5]) <= tol) & (comp[w] < 0)]
            comp[w] = j
            stack.extend(int(k) for k in w)
    # claimed rows, every exact junction against every voted row at once
    code = np.full(x, -1, np.int64)
    voted = voted_rows(clusters)
    if voted:
        V = np.asarray(voted, np.int64)
        near = lambda a, b: np.abs(a[:, None] - b[None, :]) <= 2  # noqa: E731
        st = (X[:, 0, None] == V[None, :, 1]) & near(X[:, 4], V[:, 2]) & (X[:, 1, None] == V[None, :, 3]) & near(X[:, 5], V[:, 4])
        cr = (X[:, 0, None] == V[None, :, 3]) & near(X[:, 4], V[:, 4]) & (X[:, 1, None] == V[None, :, 1]) & near(X[:, 5], V[:, 2])
        c = np.where(st, 2 * V[None, :, 0], np.where(cr, 2 * V[None, :, 0] + 1, 1 << 40)).min(axis=1)
        code = np.where(c < (1 << 40), c, -1)
    xid = np.cumsum(head) - 1
    tcomp = comp[xid]
    roots = np.unique(comp)
    rows = np.zeros(len(roots), abi.SPLIT_JUNCTION)
    for r, root in zip(rows, roots):
        mem = np.flatnonzero(comp == root)
        tm = tcomp == root
        rep = mem[np.lexsort((mem, -xreads[mem]))[0]]
        r["tid1"], r["tid2"], r["right1"], r["right2"], r["pos1"], r["pos2"] = X[rep]
        r["n_reads"] = len(np.unique(qh[tm]))
        r["n_tuples"] = int(tm.sum())
        r["n_exact"] = len(mem)
        r["lo1"], r["hi1"], r["lo2"], r["hi2"] = X[mem, 4].min(), X[mem, 4].max(), X[mem, 5].min(), X[mem, 5].max()
        for k in (0, 1):
            r["n_own"][k] = int((tm & (own_end == k)).sum())
            r["mapq_sum"][k] = int(mq[tm & (own_end == k)].sum())
        r["top_reads"] = xreads[rep]
        cm = code[mem][code[mem] >= 0]
        r["call"] = int(cm.min()) >> 1 if len(cm) else -1
        r["call_crossed"] = int(cm.min()) & 1 if len(cm) else 0
    return rows[rows["n_reads"] >= min_reads].copy()


# ---- cases without a GPU: SPLIT rows written by hand -----------------------------------------------------------------------------------
def make_splits(rows):
    """rows: (rec, qhash, own (tid, pos, right), other (chr, pos, right), flags).  flags bit 0 puts the own end into sec_*."""
    out = np.zeros(len(rows), abi.SPLIT)
    for s, (rec, qhash, own, oth, flags) in zip(out, rows):
        a, b = ("sec", "prim") if flags & 1 else ("prim", "sec")
        s["rec"], s["qhash"], s["flags"], s["tid"] = rec, qhash, flags, own[0]
        for side, (t, p, right) in ((a, own), (b, oth)):
            s[side + "_chr"], s[side + "_bp"] = t, p
            s[side + "_start"], s[side + "_end"] = (p, p + 40) if right else (p - 40 if p >= 40 else p + 50, p)
    return out


def random_case(rng, n, tlen, n_rec=50):
    """n tuples on few positions, so that exact junctions repeat, lie near each other and chain; some of every kind of dropped tuple"""
    nt = len(tlen)
    flag = np.where(rng.random(n_rec) < 0.06, 0x200, 0).astype(np.uint16) | np.where(rng.random(n_rec) < 0.04, 0x4, 0).astype(np.uint16)
    mapq = rng.choice([0, 19, 20, 37, 60, 60, 60, 60], n_rec).astype(np.uint8)
    rows = []
    for _ in range(n):
        ta, tb = int(rng.integers(-1 if rng.random() < 0.05 else 0, nt)), int(rng.integers(0, nt + (2 if rng.random() < 0.1 else 0)))
        if rng.random() < 0.03:
            tb = 1 << 29  # a hashed contig name
        base = int(rng.choice([100, 110, 300]))
        pa, pb = base + int(rng.integers(0, 8)), int(rng.choice([100, 300, 420])) + int(rng.integers(0, 8))
        if rng.random() < 0.04:
            pa = int(rng.choice([0, 100000]))
        if rng.random() < 0.04:
            pb = int(rng.choice([0, 100000]))
        own, oth = (ta, pa, int(rng.integers(0, 2))), (tb, pb, int(rng.integers(0, 2)))
        u = rng.random()
        if u < 0.05:
            oth = own
        elif u < 0.12:
            oth = (own[0], own[1], 1 - own[2])  # one position, the other side
        flags = int(rng.integers(0, 2)) | (2 if rng.random() < 0.05 else 0)
        rows.append((int(rng.integers(0, n_rec)), int(rng.integers(1, 12)), own, oth, flags))
    return make_splits(rows), flag, mapq


def random_clusters(rng, n, tlen):
    cl = np.zeros(n, abi.CLUSTER)
    cl["p1_tid"], cl["p2_tid"] = rng.integers(0, len(tlen), n), rng.integers(0, len(tlen), n)
    cl["p1_exact"] = rng.choice([100, 110, 300, 420], n) + rng.integers(0, 8, n)
    cl["p2_exact"] = rng.choice([100, 110, 300, 420], n) + rng.integers(0, 8, n)
    cl["flags"] = np.where(rng.random(n) < 0.7, 3, 1)
    return cl


# ---- cases on records ------------------------------------------------------------------------------------------------------------------
def split_800(q, ta, bpa, tb, bpb, names, flag=0x800, m1=60, m2=40):
    """one read, two alignments that both carry SA: synth._split_pair with the partner as 0x800 (or 0x100 | 0x800)"""
    return synth._split_pair(q, names, ta, bpa, tb, bpb, m1, m2, partner_flag=flag)


def canonical_design(ta, bpa, da, tb, bpb, db):
    """the call of callcases.designed_split(q, ta, bpa, da, tb, bpb, db): its 6-tuple, canonicalised"""
    a, b = (ta, bpa, int(da == "R")), (tb, bpb, int(db == "R"))
    a, b = (a, b) if a < b else (b, a)
    return a + b


def dataset(contigs, recs):
    ds = synth.Dataset(list(contigs))
    ds.recs = list(recs)
    ds.sort()
    return ds


# ---- how the command line prints a row ------------------------------------------------------------------------------------------------
COLUMNS = ["Junction", "Chr1", "Pos1", "Side1", "Chr2", "Pos2", "Side2", "Type", "Size", "Reads", "Tuples", "Exact", "TopReads", "Own1", "Own2", "MeanMQ1", "MeanMQ2", "Span1", "Span2",
           "Depth1", "Depth2", "Gene1", "Gene2"]


def type_size(r):
    """(Type, Size) of a row"""
    if int(r["tid1"]) != int(r["tid2"]):
        return "translocation", "."
    size = str(int(r["pos2"]) - int(r["pos1"]))
    if int(r["pos1"]) < int(r["pos2"]):
        sides = (int(r["right1"]), int(r["right2"]))
        return {(0, 1): "deletion", (1, 0): "duplication"}.get(sides, "inversion"), size
    return ".", size


def row_fields(index, r, names, depth1, depth2, gene1=".", gene2="."):
    typ, size = type_size(r)
    mean = lambda k: "%.1f" % (int(r["mapq_sum"][k]) / int(r["n_own"][k])) if int(r["n_own"][k]) else "."  # noqa: E731
    return ["sj%d" % index, names[int(r["tid1"])], str(int(r["pos1"])), "LR"[int(r["right1"])], names[int(r["tid2"])], str(int(r["pos2"])), "LR"[int(r["right2"])], typ, size,
            str(int(r["n_reads"])), str(int(r["n_tuples"])), str(int(r["n_exact"])), str(int(r["top_reads"])), str(int(r["n_own"][0])), str(int(r["n_own"][1])), mean(0), mean(1),
            "%d-%d" % (int(r["lo1"]), int(r["hi1"])), "%d-%d" % (int(r["lo2"]), int(r["hi2"])), str(depth1), str(depth2), gene1, gene2]


def bedpe_line(index, r, names, sample):
    typ, _ = type_size(r)
    return "\t".join([names[int(r["tid1"])], str(int(r["pos1"]) - 1), str(int(r["pos1"])), names[int(r["tid2"])], str(int(r["pos2"]) - 1), str(int(r["pos2"])), sample,
                      str(int(r["n_reads"])), "+-"[int(r["right1"])], "+-"[int(r["right2"])], "sj%d" % index, typ, "0", str(int(r["n_reads"]))])

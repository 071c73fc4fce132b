"""Soft-clip loci (`bk_clip_loci`, include/breakid_hip.h): two independent statements of the definition over the columns of a record
table - `expected`, a walk of every record with dictionaries, and `expected_sweep`, vectorised sorts and sweeps over all CIGAR
operations at once - which both return the abi.CLIP_LOCUS table and the eight counts; `why_dropped` for one record; and how the command
line prints a row, a BEDPE line and its stdout line."""
import numpy as np

from breakid_amd import abi, synth

MAX_TOL = 100
MAX_PAIR = 100_000
TILE = 256  # records per tile of the record pass (include/breakid_hip.h)
NONE = 0xFFFFFFFF
LEFT, RIGHT = 0, 1
COUNTS = ("records", "eligible", "events", "beyond", "exact", "loci", "mutual", "written")
DROP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
OP_S, OP_H = 4, 5
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X


# ---- the event rule, from the header's text ---------------------------------------------------------------------------------------------
def passes(cols, i, mapq_min):
    """tid, flag, mapq and the empty aux blob; the reference length is looked at by `record_events`"""
    return (int(cols["tid"][i]) >= 0 and not (int(cols["flag"][i]) & DROP_FLAGS) and int(cols["mapq"][i]) >= mapq_min
            and int(cols["aux_off"][i + 1]) == int(cols["aux_off"][i]))


def record_ops(cols, i):
    words = [int(w) for w in cols["cigar"][int(cols["cigar_off"][i]):int(cols["cigar_off"][i + 1])]]
    return [(w & 15, w >> 4) for w in words]


def record_events(cols, i, tlen, min_clip):
    """record i, which `passes`: (reference length, kept [(dir, p, clip length)], beyond, clips of any length)"""
    ops = record_ops(cols, i)
    reflen = sum(n for op, n in ops if op in REF_OPS)
    inner = list(ops)
    while inner and inner[0][0] == OP_H:
        inner.pop(0)
    while inner and inner[-1][0] == OP_H:
        inner.pop()
    found = []
    if inner and inner[0][0] == OP_S:
        found.append((RIGHT, int(cols["pos"][i]) + 1, inner[0][1]))
    if inner and inner[-1][0] == OP_S:
        found.append((LEFT, int(cols["pos"][i]) + reflen, inner[-1][1]))
    tid = int(cols["tid"][i])
    length = tlen[tid] if tid < len(tlen) else 0
    kept, beyond = [], 0
    if reflen > 0:
        for d, p, n in found:
            if n < min_clip:
                continue
            if p > length or p < 1:
                beyond += 1
            else:
                kept.append((d, p, n))
    return reflen, kept, beyond, len(found)


def why_dropped(cols, i, tlen, mapq_min, min_clip):
    """why record i gives no event: 'unmapped' (tid < 0), 'flag', 'mapq', 'aux', 'no_ref' (no reference length), 'no_clip', 'short',
    'beyond'; None when it gives one"""
    if int(cols["tid"][i]) < 0:
        return "unmapped"
    if int(cols["flag"][i]) & DROP_FLAGS:
        return "flag"
    if int(cols["mapq"][i]) < mapq_min:
        return "mapq"
    if int(cols["aux_off"][i + 1]) != int(cols["aux_off"][i]):
        return "aux"
    reflen, kept, beyond, clips = record_events(cols, i, tlen, min_clip)
    if reflen <= 0:
        return "no_ref"
    if kept:
        return None
    return "beyond" if beyond else "short" if clips else "no_clip"


def runs(values, tol):
    """the sorted distinct values cut where two neighbours differ by more than tol"""
    out = []
    for v in sorted(set(values)):
        if out and v - out[-1][-1] <= tol:
            out[-1].append(v)
        else:
            out.append([v])
    return out


def voted_breakpoints(cl):
    """(row, tid, pos) of every side of every voted row"""
    out = []
    if cl is None:
        return out
    for r, c in enumerate(cl):
        if not int(c["flags"]) & 2:
            continue
        if int(c["p1_tid"]) >= 0:
            out.append((r, int(c["p1_tid"]), int(c["p1_exact"])))
        if int(c["p2_tid"]) >= 0 and int(c["p2_exact"]) >= 0:
            out.append((r, int(c["p2_tid"]), int(c["p2_exact"])))
    return out


# ---- the first statement ------------------------------------------------------------------------------------------------------------------
def expected(cols, tlen, mapq_min, min_clip, tol, pair_dist, min_reads, cl=None, info=None):
    """one record after the other, dictionaries; the partner by looking at every pair of loci"""
    n = len(cols["tid"])
    exact, n_elig, n_events, n_beyond = {}, 0, 0, 0
    for i in range(n):
        if not passes(cols, i, mapq_min):
            continue
        reflen, kept, beyond, _ = record_events(cols, i, tlen, min_clip)
        if reflen <= 0:
            continue
        n_elig += 1
        n_beyond += beyond
        n_events += beyond + len(kept)
        f = int(cols["flag"][i])
        for d, p, clip in kept:
            exact.setdefault((d, int(cols["tid"][i]), p), []).append((int(cols["qhash"][i]), f, int(cols["mapq"][i]), clip))
    loci = []
    for d, tid in sorted({k[:2] for k in exact}):
        for ps in runs([k[2] for k in exact if k[:2] == (d, tid)], tol):
            members = [(d, tid, p) for p in ps]
            reads = {k: len({e[0] for e in exact[k]}) for k in members}
            rep = min(members, key=lambda k: (-reads[k], k[2]))
            ev = [e for k in members for e in exact[k]]
            loci.append(dict(dir=d, tid=tid, pos=rep[2], n_reads=len({e[0] for e in ev}), n_rows=len(ev), n_exact=len(members), top_reads=reads[rep], lo_pos=ps[0],
                             hi_pos=ps[-1], n_rev=sum((e[1] >> 4) & 1 for e in ev), max_clip=max(e[3] for e in ev), clip_sum=sum(e[3] for e in ev),
                             mapq_sum=sum(e[2] for e in ev), n_orphan=sum(1 for e in ev if e[1] & 1 and e[1] & 8),
                             n_improper=sum(1 for e in ev if e[1] & 1 and not e[1] & 8 and not e[1] & 2)))
    # facing, over all loci
    for a in loci:
        best = None
        for j, b in enumerate(loci):
            if b["tid"] != a["tid"] or b["dir"] == a["dir"]:
                continue
            p, q = (a["pos"], b["pos"]) if a["dir"] == LEFT else (b["pos"], a["pos"])
            if abs(q - p - 1) > pair_dist:
                continue
            key = (-b["n_reads"], abs(q - p - 1), b["pos"])
            if best is None or key < best[0]:
                best = (key, j, q - p)
        a["partner"], a["off"] = (best[1], best[2]) if best else (None, 0)
    bps = voted_breakpoints(cl)
    kept_index, k = {}, 0
    for j, a in enumerate(loci):
        if a["n_reads"] >= min_reads:
            kept_index[j] = k
            k += 1
    table = np.zeros(len(kept_index), abi.CLIP_LOCUS)
    n_mutual = 0
    for j, a in enumerate(loci):
        m = a["partner"]
        mutual = m is not None and loci[m]["partner"] == j
        n_mutual += mutual
        if j not in kept_index:
            continue
        r = table[kept_index[j]]
        for f in ("tid", "pos", "dir", "n_reads", "n_rows", "n_exact", "top_reads", "lo_pos", "hi_pos", "n_rev", "max_clip", "clip_sum", "mapq_sum", "n_orphan", "n_improper"):
            r[f] = a[f]
        r["n_fwd"] = a["n_rows"] - a["n_rev"]
        r["mate"] = NONE
        if m is not None:
            r["flags"] = 1 | (2 if mutual else 0)
            r["mate"] = kept_index.get(m, NONE)
            r["mate_pos"], r["mate_reads"], r["mate_off"] = loci[m]["pos"], loci[m]["n_reads"], a["off"]
        claims = [row for row, tid, pos in bps if tid == a["tid"] and a["lo_pos"] - 2 <= pos <= a["hi_pos"] + 2]
        r["claim"] = min(claims) if claims else NONE
    counts = dict(zip(COUNTS, (n, n_elig, n_events, n_beyond, len(exact), len(loci), n_mutual, len(table))))
    if info is not None:
        info.update(counts)
        info["exact_keys"] = sorted(exact)
    return table, counts


# ---- the second statement -----------------------------------------------------------------------------------------------------------------
def run_ids(heads):
    return np.cumsum(heads) - 1


def expected_sweep(cols, tlen, mapq_min, min_clip, tol, pair_dist, min_reads, cl=None):
    """every CIGAR operation of the table at once, sorts and sweeps; the partner by a search in the other direction's positions"""
    n = len(cols["tid"])
    tid, pos, flag, mapq = cols["tid"].astype(np.int64), cols["pos"].astype(np.int64), cols["flag"].astype(np.int64), cols["mapq"].astype(np.int64)
    off, aux_off = cols["cigar_off"].astype(np.int64), cols["aux_off"].astype(np.int64)
    cig = cols["cigar"][:off[-1] if n else 0].astype(np.int64)
    op, ln = cig & 15, cig >> 4
    consumed = np.concatenate([[0], np.cumsum(np.where(np.isin(op, REF_OPS), ln, 0))])
    reflen = consumed[off[1:]] - consumed[off[:-1]] if n else np.zeros(0, np.int64)
    elig = (tid >= 0) & ((flag & DROP_FLAGS) == 0) & (mapq >= mapq_min) & (aux_off[1:] == aux_off[:-1]) & (reflen > 0)
    counts = [n, int(elig.sum()), 0, 0, 0, 0, 0, 0]
    empty = np.zeros(0, abi.CLIP_LOCUS)
    not_h = np.flatnonzero(op != OP_H)
    if len(not_h) == 0:
        return empty, dict(zip(COUNTS, counts))
    c0, c1 = off[:-1], off[1:]
    a = np.searchsorted(not_h, c0, "left")       # the first operation at or behind c0 that is not H
    z = np.searchsorted(not_h, c1, "left") - 1   # the last one in front of c1
    first, last = not_h[np.minimum(a, len(not_h) - 1)], not_h[np.maximum(z, 0)]
    has = (a < len(not_h)) & (first < c1) & (z >= 0) & (last >= c0)
    first, last = np.where(has, first, 0), np.where(has, last, 0)
    lead = elig & has & (op[first] == OP_S) & (ln[first] >= min_clip)
    trail = elig & has & (op[last] == OP_S) & (ln[last] >= min_clip)
    rec = np.concatenate([np.flatnonzero(lead), np.flatnonzero(trail)])
    d = np.concatenate([np.full(int(lead.sum()), RIGHT, np.int64), np.full(int(trail.sum()), LEFT, np.int64)])
    p = np.concatenate([pos[lead] + 1, (pos + reflen)[trail]])
    clip = np.concatenate([ln[first[lead]], ln[last[trail]]])
    lens = np.asarray(list(tlen) + [0], np.int64)
    t = tid[rec]
    beyond = (p > lens[np.minimum(t, len(tlen))]) | (p < 1)
    counts[2], counts[3] = len(rec), int(beyond.sum())
    keep = ~beyond
    if not keep.any():
        return empty, dict(zip(COUNTS, counts))
    rec, d, p, clip, t = rec[keep], d[keep], p[keep], clip[keep], t[keep]
    q, f, mq = cols["qhash"][rec], flag[rec], mapq[rec]
    o = np.lexsort((p, t, d))
    d, p, clip, t, q, f, mq = d[o], p[o], clip[o], t[o], q[o], f[o], mq[o]
    new_group = np.concatenate([[True], (d[1:] != d[:-1]) | (t[1:] != t[:-1])])
    locus = run_ids(new_group | np.concatenate([[True], p[1:] - p[:-1] > tol]))
    exact = run_ids(new_group | np.concatenate([[True], p[1:] != p[:-1]]))
    n_loci, n_exact = int(locus[-1]) + 1, int(exact[-1]) + 1
    counts[4], counts[5] = n_exact, n_loci
    xq = np.unique(np.stack([exact.astype(np.uint64), q.astype(np.uint64)], axis=1), axis=0)
    x_reads = np.bincount(xq[:, 0].astype(np.int64), minlength=n_exact)
    lq = np.unique(np.stack([locus.astype(np.uint64), q.astype(np.uint64)], axis=1), axis=0)
    l_reads = np.bincount(lq[:, 0].astype(np.int64), minlength=n_loci)
    x_first = np.flatnonzero(np.concatenate([[True], exact[1:] != exact[:-1]]))
    x_locus, x_pos = locus[x_first], p[x_first]
    best = np.lexsort((x_pos, -x_reads, x_locus))
    rep = best[np.concatenate([[True], x_locus[best][1:] != x_locus[best][:-1]])]  # the first exact site of every locus in that order
    l_first = np.flatnonzero(np.concatenate([[True], locus[1:] != locus[:-1]]))
    table = np.zeros(n_loci, abi.CLIP_LOCUS)
    table["tid"], table["dir"] = t[l_first], d[l_first]
    table["pos"], table["top_reads"] = x_pos[rep], x_reads[rep]
    table["n_reads"], table["n_rows"], table["n_exact"] = l_reads, np.bincount(locus, minlength=n_loci), np.bincount(x_locus, minlength=n_loci)
    table["lo_pos"], table["hi_pos"] = np.minimum.reduceat(p, l_first), np.maximum.reduceat(p, l_first)
    table["n_rev"] = np.add.reduceat((f >> 4) & 1, l_first)
    table["n_fwd"] = table["n_rows"] - table["n_rev"]
    table["max_clip"], table["clip_sum"], table["mapq_sum"] = np.maximum.reduceat(clip, l_first), np.add.reduceat(clip, l_first), np.add.reduceat(mq, l_first)
    table["n_orphan"] = np.add.reduceat(((f & 1) != 0) & ((f & 8) != 0), l_first)
    table["n_improper"] = np.add.reduceat(((f & 1) != 0) & ((f & 8) == 0) & ((f & 2) == 0), l_first)
    # facing: the loci are in the order (dir, tid, pos); a search bounds the other direction's window, an ordering picks the partner
    L_dir, L_tid, L_pos, L_reads = table["dir"].astype(np.int64), table["tid"].astype(np.int64), table["pos"].astype(np.int64), table["n_reads"].astype(np.int64)
    width = int(max(lens.max(), L_pos.max())) + 2
    key = (L_dir * (len(tlen) + 1) + L_tid) * width + L_pos
    centre = np.where(L_dir == LEFT, L_pos + 1, L_pos - 1)
    other = ((1 - L_dir) * (len(tlen) + 1) + L_tid) * width
    lo = np.searchsorted(key, other + np.maximum(centre - pair_dist, 0), "left")
    hi = np.searchsorted(key, other + np.minimum(centre + pair_dist, width - 1), "right")
    partner = np.full(n_loci, -1, np.int64)
    for j in np.flatnonzero(hi > lo):
        cand = np.arange(lo[j], hi[j])
        partner[j] = cand[np.lexsort((L_pos[cand], np.abs(L_pos[cand] - centre[j]), -L_reads[cand]))[0]]
    has_p = partner >= 0
    ps = np.where(has_p, partner, 0)
    mutual = has_p & (partner[ps] == np.arange(n_loci))
    counts[6] = int(mutual.sum())
    kept = table["n_reads"] >= min_reads
    new_index = np.cumsum(kept) - 1
    table["flags"] = has_p.astype(np.int64) | (mutual.astype(np.int64) << 1)
    table["mate"] = np.where(has_p & kept[ps], new_index[ps], NONE)
    table["mate_pos"] = np.where(has_p, L_pos[ps], 0)
    table["mate_reads"] = np.where(has_p, L_reads[ps], 0)
    table["mate_off"] = np.where(has_p, np.where(L_dir == LEFT, L_pos[ps] - L_pos, L_pos - L_pos[ps]), 0)
    # the claim: the voted breakpoints sorted by (tid, pos, row); the smallest row inside every span
    table["claim"] = NONE
    if cl is not None and len(cl):
        voted = (cl["flags"] & 2) != 0
        b_row = np.concatenate([np.flatnonzero(voted & (cl["p1_tid"] >= 0)), np.flatnonzero(voted & (cl["p2_tid"] >= 0) & (cl["p2_exact"] >= 0))])
        n1 = int((voted & (cl["p1_tid"] >= 0)).sum())
        b_tid = np.concatenate([cl["p1_tid"][b_row[:n1]], cl["p2_tid"][b_row[n1:]]]).astype(np.int64)
        b_pos = np.concatenate([cl["p1_exact"][b_row[:n1]].astype(np.int64), cl["p2_exact"][b_row[n1:]].astype(np.int64)])
        o = np.lexsort((b_pos, b_tid))
        b_key, b_row = (b_tid * (1 << 33) + b_pos)[o], b_row[o]
        lo = np.searchsorted(b_key, L_tid * (1 << 33) + np.maximum(table["lo_pos"].astype(np.int64) - 2, 0), "left")
        hi = np.searchsorted(b_key, L_tid * (1 << 33) + table["hi_pos"].astype(np.int64) + 2, "right")
        for j in np.flatnonzero(hi > lo):
            table["claim"][j] = b_row[lo[j]:hi[j]].min()
    out = table[kept]
    counts[7] = len(out)
    return out, dict(zip(COUNTS, counts))


def both(cols, tlen, mapq_min=20, min_clip=10, tol=2, pair_dist=50, min_reads=1, cl=None, info=None):
    """the table and the counts, after the two statements agreed byte for byte"""
    a, ca = expected(cols, tlen, mapq_min, min_clip, tol, pair_dist, min_reads, cl, info)
    b, cb = expected_sweep(cols, tlen, mapq_min, min_clip, tol, pair_dist, min_reads, cl)
    assert a.tobytes() == b.tobytes() and ca == cb, (a, b, ca, cb)
    return a, ca


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
PROPER = 0x1 | 0x2


def read(name, tid, pos, cigar, flag=PROPER, mapq=60, sa=None):
    """one alignment (pos 0-based); its mate is not in the table"""
    return synth.Rec(name, flag, tid, pos, mapq, cigar, -1, -1, 0, sa=sa) if sa else synth.Rec(name, flag, tid, pos, mapq, cigar, -1, -1, 0)


def left_clip(name, tid, p, m=60, s=40, **kw):
    """a read whose aligned bases end at 1-based p and whose s clipped bases follow: the event (tid, p, LEFT)"""
    return read(name, tid, p - m, "%dM%dS" % (m, s), **kw)


def right_clip(name, tid, p, m=60, s=40, **kw):
    """a read whose s clipped bases lie in front of aligned bases that begin at 1-based p: the event (tid, p, RIGHT)"""
    return read(name, tid, p - 1, "%dS%dM" % (s, m), **kw)


def dataset(contigs, recs):
    ds = synth.Dataset(list(contigs))
    ds.recs = list(recs)
    ds.sort()
    return ds


SA = "c0,77,+,40S60M,60,0;"


def hand_example():
    """the example of include/breakid_hip.h: (contigs, records)"""
    recs = [read(q, 0, 899, "100M50S") for q in "abc"] + [read("d", 0, 900, "101M49S", flag=PROPER | 0x10, mapq=40)]
    recs += [read(q, 0, 989, "50S100M") for q in "ef"] + [read("g", 0, 989, "9S100M"), read("h", 0, 989, "50S100M", sa=SA)]
    recs += [read("i", 0, 5000, "5H30S100M", flag=0x1 | 0x8), read("j", 0, 899, "100M50S", mapq=10)]
    return [("c0", 1_000_000)], recs


CIGARS = ["100M", "30S70M", "70M30S", "20S60M20S", "5H30S65M", "70M30S5H", "5H12S60M12S5H", "9S91M", "91M9S", "10S90M", "30S5I65M", "30S", "5H30S", "30S40I", "*",
          "40M20D40M15S", "15S40M20N40M", "3H9S50M30S"]


def random_cols(rng, n, tlen):
    """a small table: few positions and few read names, clips around min_clip 10, hard clips in front of soft clips, both clips on one
    record, records without a reference length, every flag that drops a record, SA tags, positions at a contig's end"""
    recs = []
    for i in range(n):
        tid = int(rng.integers(-1, len(tlen))) if rng.random() < 0.1 else int(rng.integers(0, len(tlen)))
        cigar = CIGARS[int(rng.integers(0, len(CIGARS)))]
        flag = int(rng.choice([0, 0x10, PROPER | 0x40, PROPER | 0x80 | 0x10, 0x1 | 0x8 | 0x40, 0x1 | 0x40 | 0x10])) | (int(rng.choice([0x4, 0x100, 0x200, 0x400, 0x800])) if rng.random() < 0.08 else 0)
        pos = max(0, tlen[max(tid, 0)] - int(rng.integers(0, 110))) if rng.random() < 0.1 else 200 + int(rng.integers(0, 30)) * int(rng.choice([1, 3, 20]))
        sa = SA if rng.random() < 0.08 else None
        recs.append(read("r%d" % int(rng.integers(0, max(2, n // 2))), tid, pos, cigar, flag=flag, mapq=int(rng.choice([0, 19, 20, 60])), sa=sa))
    return dataset([("c%d" % k, l) for k, l in enumerate(tlen)], recs).to_soa()


# ---- how the command line prints a row ------------------------------------------------------------------------------------------------
COLUMNS = ["Locus", "Chr", "Pos", "Side", "Reads", "Rows", "Exact", "TopReads", "Fwd", "Rev", "MeanMQ", "Span", "MaxClip", "MeanClip", "Orphans", "Improper", "Mate", "MatePos",
           "MateReads", "MateOff", "Mutual", "Depth", "Gene"]


def written(rows):
    """which returned rows the command line writes: the unclaimed ones"""
    return [i for i, r in enumerate(rows) if int(r["claim"]) == NONE]


def row_fields(index, r, rows, names, depth, gene="intergenic"):
    facing = bool(int(r["flags"]) & 1)
    mate = int(r["mate"])
    shown = facing and mate != NONE and int(rows[mate]["claim"]) == NONE
    return ["cl%d" % index, names[int(r["tid"])], str(int(r["pos"])), "R" if int(r["dir"]) == RIGHT else "L", str(int(r["n_reads"])), str(int(r["n_rows"])), str(int(r["n_exact"])),
            str(int(r["top_reads"])), str(int(r["n_fwd"])), str(int(r["n_rev"])), "%.1f" % (int(r["mapq_sum"]) / int(r["n_rows"])), "%d-%d" % (int(r["lo_pos"]), int(r["hi_pos"])),
            str(int(r["max_clip"])), "%.1f" % (int(r["clip_sum"]) / int(r["n_rows"])), str(int(r["n_orphan"])), str(int(r["n_improper"])), "cl%d" % mate if shown else ".",
            str(int(r["mate_pos"])) if facing else ".", str(int(r["mate_reads"])) if facing else ".", str(int(r["mate_off"])) if facing else ".", "1" if int(r["flags"]) & 2 else "0",
            str(depth), gene]


def bedpe_pairs(rows):
    """(left row, right row) of every mutual pair whose two rows are both written, in the order of its LEFT row"""
    out = []
    for i in written(rows):
        r = rows[i]
        if int(r["dir"]) == LEFT and int(r["flags"]) & 2 and int(r["mate"]) != NONE and int(rows[int(r["mate"])]["claim"]) == NONE:
            out.append((i, int(r["mate"])))
    return out


def bedpe_line(i, j, rows, names, sample):
    a, b = rows[i], rows[j]
    chrom, p, q, reads = names[int(a["tid"])], int(a["pos"]), int(b["pos"]), int(a["n_reads"]) + int(b["n_reads"])
    return "\t".join([chrom, str(p - 1), str(p), chrom, str(q - 1), str(q), sample, str(reads), "+", "-", "cl%d" % i, "insertion_site", "0", str(reads)])


def stdout_line(counts, rows):
    return "cliploci: %d records eligible, %d events, %d beyond a contig's end, %d exact, %d loci, %d with a mutual partner, %d claimed by a voted call, %d written" % (
        counts["eligible"], counts["events"], counts["beyond"], counts["exact"], counts["loci"], counts["mutual"], len(rows) - len(written(rows)), len(written(rows)))

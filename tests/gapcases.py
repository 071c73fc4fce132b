"""CIGAR gaps (`bk_cigar_gaps`, include/breakid_hip.h): two independent statements of the definition over the columns of a record
table - `expected`, a walk of every record with dictionaries, and `expected_sweep`, vectorised sorts and sweeps over all CIGAR
operations at once - which both return the abi.CIGAR_GAP table and the eight counts; `why_dropped` for one record; and how the command
line prints a row, a BEDPE line and its stdout line."""
import numpy as np

from breakid_amd import abi, synth

MAX_TOL = 100
MAX_LEN = 1_000_000
TILE = 256  # records per tile of the record pass (include/breakid_hip.h)
FIELDS = ("tid", "start", "len", "kind", "n_reads", "n_rows", "n_exact", "top_reads", "lo_start", "hi_start", "lo_len", "hi_len", "n_fwd", "n_rev", "mapq_sum")
COUNTS = ("records", "eligible", "events", "beyond", "exact", "loci", "calls", "written")
DROP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
OPS = "MIDNSHP=X"
MATCH, REF_ONLY = (0, 7, 8), (2, 3)  # M = X; D N


def eligible(cols, i, mapq_min):
    return int(cols["tid"][i]) >= 0 and not (int(cols["flag"][i]) & DROP_FLAGS) and int(cols["mapq"][i]) >= mapq_min


def walk(cols, i, tlen, min_len, anchor):
    """the events of record i, eligible or not: (kept [(kind, start, len)], beyond, gaps long enough, gaps long enough and anchored)"""
    words = [int(w) for w in cols["cigar"][int(cols["cigar_off"][i]):int(cols["cigar_off"][i + 1])]]
    ops = [(w & 15, w >> 4) for w in words]
    tid = int(cols["tid"][i])
    length = tlen[tid] if 0 <= tid < len(tlen) else 0
    kept, beyond, long_enough, anchored = [], 0, 0, 0
    p = int(cols["pos"][i])
    for k, (op, n) in enumerate(ops):
        if op in (1, 2) and n >= min_len:
            long_enough += 1
            front = sum(m for o, m in ops[:k] if o in MATCH)
            behind = sum(m for o, m in ops[k + 1:] if o in MATCH)
            if front >= anchor and behind >= anchor:
                anchored += 1
                right = p + n + 1 if op == 2 else p + 1
                if right > length or p < 0:
                    beyond += 1
                else:
                    kept.append((0 if op == 2 else 1, p, n))
        if op in MATCH or op in REF_ONLY:
            p += n
    return kept, beyond, long_enough, anchored


def why_dropped(cols, i, tlen, mapq_min, min_len, anchor):
    """why record i gives no event: 'unmapped' (tid < 0), 'flag', 'mapq', 'no_cigar', 'short' (no D or I of min_len), 'anchor',
    'beyond'; None when it gives one"""
    if int(cols["tid"][i]) < 0:
        return "unmapped"
    if int(cols["flag"][i]) & DROP_FLAGS:
        return "flag"
    if int(cols["mapq"][i]) < mapq_min:
        return "mapq"
    if int(cols["cigar_off"][i + 1]) == int(cols["cigar_off"][i]):
        return "no_cigar"
    kept, beyond, long_enough, anchored = walk(cols, i, tlen, min_len, anchor)
    if kept:
        return None
    return "beyond" if beyond else "anchor" if long_enough else "short"


def runs(values, tol):
    """the sorted distinct values cut where two neighbours differ by more than tol"""
    out = []
    for v in sorted(set(values)):
        if out and v - out[-1][-1] <= tol:
            out[-1].append(v)
        else:
            out.append([v])
    return out


def expected(cols, tlen, mapq_min, min_len, anchor, tol, min_reads, info=None):
    """the first statement: one record after the other, dictionaries"""
    n = len(cols["tid"])
    exact, n_elig, n_events, n_beyond = {}, 0, 0, 0
    for i in range(n):
        if not eligible(cols, i, mapq_min):
            continue
        n_elig += 1
        kept, beyond, _, _ = walk(cols, i, tlen, min_len, anchor)
        n_beyond += beyond
        for kind, start, ln in kept:
            n_events += 1
            exact.setdefault((kind, int(cols["tid"][i]), start, ln), []).append((int(cols["qhash"][i]), (int(cols["flag"][i]) >> 4) & 1, int(cols["mapq"][i])))
    rows, n_loci = [], 0
    for kind, tid in sorted({k[:2] for k in exact}):
        mine = [k for k in exact if k[:2] == (kind, tid)]
        for locus in runs([k[2] for k in mine], tol):
            n_loci += 1
            inside = [k for k in mine if k[2] in locus]
            for lens in runs([k[3] for k in inside], tol):
                members = sorted(k for k in inside if k[3] in lens)
                reads = {k: len({q for q, _, _ in exact[k]}) for k in members}
                rep = min(members, key=lambda k: (-reads[k], k[2], k[3]))
                ev = [e for k in members for e in exact[k]]
                r = np.zeros((), abi.CIGAR_GAP)
                r["tid"], r["start"], r["len"], r["kind"] = tid, rep[2], rep[3], kind
                r["n_reads"], r["n_rows"], r["n_exact"], r["top_reads"] = len({q for q, _, _ in ev}), len(ev), len(members), reads[rep]
                r["lo_start"], r["hi_start"] = min(k[2] for k in members), max(k[2] for k in members)
                r["lo_len"], r["hi_len"] = min(k[3] for k in members), max(k[3] for k in members)
                r["n_rev"] = sum(rev for _, rev, _ in ev)
                r["n_fwd"] = len(ev) - int(r["n_rev"])
                r["mapq_sum"] = sum(mq for _, _, mq in ev)
                rows.append(r)
    table = np.array(rows, abi.CIGAR_GAP) if rows else np.zeros(0, abi.CIGAR_GAP)
    out = table[table["n_reads"] >= min_reads]
    counts = dict(zip(COUNTS, (n, n_elig, n_events, n_beyond, len(exact), n_loci, len(table), len(out))))
    if info is not None:
        info.update(counts)
        info["exact_keys"] = sorted(exact)
    return out, counts


def run_ids(heads):
    return np.cumsum(heads) - 1


def expected_sweep(cols, tlen, mapq_min, min_len, anchor, tol, min_reads):
    """the second statement: every CIGAR operation of the table at once, sorts and sweeps"""
    n = len(cols["tid"])
    tid, pos, flag, mapq = cols["tid"].astype(np.int64), cols["pos"].astype(np.int64), cols["flag"].astype(np.int64), cols["mapq"].astype(np.int64)
    off = cols["cigar_off"].astype(np.int64)
    cig = cols["cigar"][:off[-1] if n else 0].astype(np.int64)
    op, ln = cig & 15, cig >> 4
    rec = np.repeat(np.arange(n), np.diff(off)) if n else np.zeros(0, np.int64)
    matched = np.where(np.isin(op, MATCH), ln, 0)
    moved = np.where(np.isin(op, MATCH + REF_ONLY), ln, 0)
    cm, cr = np.concatenate([[0], np.cumsum(matched)]), np.concatenate([[0], np.cumsum(moved)])
    first = off[rec]
    front = cm[:-1] - cm[first]
    behind = (cm[off[1:]] - cm[off[:-1]])[rec] - front - matched
    start = pos[rec] + cr[:-1] - cr[first]
    ok = (tid >= 0) & ((flag & DROP_FLAGS) == 0) & (mapq >= mapq_min)
    event = ok[rec] & np.isin(op, (1, 2)) & (ln >= min_len) & (front >= anchor) & (behind >= anchor)
    lens = np.asarray(list(tlen) + [0], np.int64)
    length = lens[np.where((tid >= 0) & (tid < len(tlen)), tid, len(tlen))][rec]
    right = np.where(op == 2, start + ln + 1, start + 1)
    beyond = event & ((right > length) | (start < 0))
    keep = event & ~beyond
    counts = [n, int(ok.sum()), int(keep.sum()), int(beyond.sum()), 0, 0, 0, 0]
    if not keep.any():
        return np.zeros(0, abi.CIGAR_GAP), dict(zip(COUNTS, counts))
    kind, t, s, l, r = (op[keep] == 1).astype(np.int64), tid[rec[keep]], start[keep], ln[keep], rec[keep]
    q, rev, mq = cols["qhash"][r], (flag[r] >> 4) & 1, mapq[r]
    o = np.lexsort((l, s, t, kind))
    kind, t, s, l, q, rev, mq = kind[o], t[o], s[o], l[o], q[o], rev[o], mq[o]
    new_group = np.concatenate([[True], (kind[1:] != kind[:-1]) | (t[1:] != t[:-1])])
    locus = run_ids(new_group | np.concatenate([[True], s[1:] - s[:-1] > tol]))
    o = np.lexsort((s, l, locus))
    kind, t, s, l, q, rev, mq, locus = kind[o], t[o], s[o], l[o], q[o], rev[o], mq[o], locus[o]
    call = run_ids(np.concatenate([[True], (locus[1:] != locus[:-1]) | (l[1:] - l[:-1] > tol)]))
    exact = run_ids(np.concatenate([[True], (call[1:] != call[:-1]) | (l[1:] != l[:-1]) | (s[1:] != s[:-1])]))
    n_calls, n_exact = int(call[-1]) + 1, int(exact[-1]) + 1
    counts[4:7] = [n_exact, int(locus.max()) + 1, n_calls]
    # distinct reads of every exact event and of every call
    xq = np.unique(np.stack([exact.astype(np.uint64), q.astype(np.uint64)], axis=1), axis=0)
    x_reads = np.bincount(xq[:, 0].astype(np.int64), minlength=n_exact)
    cq = np.unique(np.stack([call.astype(np.uint64), q.astype(np.uint64)], axis=1), axis=0)
    c_reads = np.bincount(cq[:, 0].astype(np.int64), minlength=n_calls)
    x_first = np.flatnonzero(np.concatenate([[True], exact[1:] != exact[:-1]]))
    x_call, x_start, x_len = call[x_first], s[x_first], l[x_first]
    best = np.lexsort((x_len, x_start, -x_reads, x_call))
    rep = best[np.concatenate([[True], x_call[best][1:] != x_call[best][:-1]])]  # the first exact event of every call in that order
    c_first = np.flatnonzero(np.concatenate([[True], call[1:] != call[:-1]]))
    table = np.zeros(n_calls, abi.CIGAR_GAP)
    table["tid"], table["kind"] = t[c_first], kind[c_first]
    table["start"], table["len"], table["top_reads"] = x_start[rep], x_len[rep], x_reads[rep]
    table["n_reads"], table["n_rows"], table["n_exact"] = c_reads, np.bincount(call, minlength=n_calls), np.bincount(x_call, minlength=n_calls)
    table["lo_start"], table["hi_start"] = np.minimum.reduceat(s, c_first), np.maximum.reduceat(s, c_first)
    table["lo_len"], table["hi_len"] = np.minimum.reduceat(l, c_first), np.maximum.reduceat(l, c_first)
    table["n_rev"] = np.add.reduceat(rev, c_first)
    table["n_fwd"] = table["n_rows"] - table["n_rev"]
    table["mapq_sum"] = np.add.reduceat(mq, c_first)
    out = table[table["n_reads"] >= min_reads]
    counts[7] = len(out)
    return out, dict(zip(COUNTS, counts))


def both(cols, tlen, mapq_min=20, min_len=20, anchor=10, tol=2, min_reads=1, info=None):
    """the table and the counts, after the two statements agreed byte for byte"""
    a, ca = expected(cols, tlen, mapq_min, min_len, anchor, tol, min_reads, info)
    b, cb = expected_sweep(cols, tlen, mapq_min, min_len, anchor, tol, min_reads)
    assert a.tobytes() == b.tobytes() and ca == cb, (a, b, ca, cb)
    return a, ca


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def read(name, tid, pos, cigar, flag=0, mapq=60):
    """one alignment without a mate (pos 0-based)"""
    return synth.Rec(name, flag, tid, pos, mapq, cigar, -1, -1, 0)


def dataset(contigs, recs):
    ds = synth.Dataset(list(contigs))
    ds.recs = list(recs)
    ds.sort()
    return ds


def random_cols(rng, n, tlen):
    """a small table whose CIGARs hold every operation, gaps around min_len 20, anchors around 10, few positions and few read names"""
    recs = []
    for i in range(n):
        tid = int(rng.integers(-1, len(tlen))) if rng.random() < 0.1 else int(rng.integers(0, len(tlen)))
        ops = []
        for _ in range(int(rng.integers(0, 7))):
            o = OPS[int(rng.integers(0, 9))] if rng.random() < 0.4 else "MDI"[int(rng.integers(0, 3))]
            ln = int(rng.choice([1, 5, 9, 10, 11, 19, 20, 21, 22, 24, 45])) if o in "MDI=X" else int(rng.integers(1, 30))
            ops.append("%d%s" % (ln, o))
        flag = int(rng.choice([0, 0x10, 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x10])) | (int(rng.choice([0x4, 0x100, 0x200, 0x400, 0x800])) if rng.random() < 0.08 else 0)
        pos = max(0, tlen[max(tid, 0)] - int(rng.integers(0, 60))) if rng.random() < 0.1 else int(rng.integers(0, 12)) * 3
        recs.append(synth.Rec("r%d" % int(rng.integers(0, max(2, n // 2))), flag, tid, pos, int(rng.choice([0, 19, 20, 60])), "".join(ops), -1, -1, 0))
    return dataset([("c%d" % k, l) for k, l in enumerate(tlen)], recs).to_soa()


# ---- how the command line prints a row ------------------------------------------------------------------------------------------------
COLUMNS = ["Gap", "Chr", "Start", "End", "Type", "Len", "Reads", "Rows", "Exact", "TopReads", "Fwd", "Rev", "MeanMQ", "StartSpan", "LenSpan", "Depth1", "Depth2", "Gene1", "Gene2"]


def gap_end(r):
    return int(r["start"]) + (int(r["len"]) + 1 if int(r["kind"]) == abi.GAP_DEL else 1)


def gap_type(r):
    return "deletion" if int(r["kind"]) == abi.GAP_DEL else "insertion"


def row_fields(index, r, names, depth1, depth2, gene1="intergenic", gene2="intergenic"):
    return ["gp%d" % index, names[int(r["tid"])], str(int(r["start"])), str(gap_end(r)), gap_type(r), str(int(r["len"])), str(int(r["n_reads"])), str(int(r["n_rows"])),
            str(int(r["n_exact"])), str(int(r["top_reads"])), str(int(r["n_fwd"])), str(int(r["n_rev"])), "%.1f" % (int(r["mapq_sum"]) / int(r["n_rows"])),
            "%d-%d" % (int(r["lo_start"]), int(r["hi_start"])), "%d-%d" % (int(r["lo_len"]), int(r["hi_len"])), str(depth1), str(depth2), gene1, gene2]


def bedpe_line(index, r, names, sample):
    chrom, end = names[int(r["tid"])], gap_end(r)
    return "\t".join([chrom, str(int(r["start"]) - 1), str(int(r["start"])), chrom, str(end - 1), str(end), sample, str(int(r["n_reads"])), "+", "-", "gp%d" % index, gap_type(r), "0",
                      str(int(r["n_reads"]))])


def stdout_line(counts):
    return "gaps: %d records eligible, %d events, %d beyond a contig's end, %d exact, %d calls, %d written" % (
        counts["eligible"], counts["events"], counts["beyond"], counts["exact"], counts["calls"], counts["written"])

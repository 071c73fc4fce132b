"""The fusion-frame definition of include/breakid_hip.h in plain Python, twice: `expected` loops over all transcripts per side and all
pairs and takes every number from the coordinates of the coding parts; `per_base` marks every base of a small contig as coding /
retained per transcript and counts.  Also: seeded small models, the nested locus of the GPU tests, and the text of the twin columns
and INFO fields the command line writes."""
import numpy as np

from breakid_amd import abi

NONE, ANTISENSE, TRUNCATING, PROMOTER, OUTFRAME, INFRAME = range(6)
HEAD, TAIL = 1, 2
NONCODING, UTR5, CDS, INTRON, UTR3 = 1, 2, 3, 4, 5


def as_sites(rows):
    """(tid1, pos1, right1, tid2, pos2, right2) rows as abi.FRAME_SITE"""
    s = np.zeros(len(rows), abi.FRAME_SITE)
    for k, (t1, p1, r1, t2, p2, r2) in enumerate(rows):
        s[k]["tid1"], s[k]["pos1"], s[k]["right1"], s[k]["tid2"], s[k]["pos2"], s[k]["right2"] = t1, p1, r1, t2, p2, r2
    return s


def parts_of(cols, i):
    o0, o1 = int(cols["ex_off"][i]), int(cols["ex_off"][i + 1])
    return [(int(cols["ex_start"][g]), int(cols["ex_end"][g])) for g in range(o0, o1)]


def overlapping(cols, tid, P):
    if tid < 0:
        return []
    return [i for i in range(len(cols["tid"])) if int(cols["tid"][i]) == tid and int(cols["tx_start"][i]) < P <= int(cols["tx_end"][i])]


def side_info(cols, i, P, right):
    """(L, cod, role, exon, loc) of transcript i on the side (P, right), from the coordinates of its parts"""
    parts = parts_of(cols, i)
    minus = int(cols["strand"][i]) == 1
    L = sum(e - s for s, e in parts)
    b = P - 1
    if not right:
        r = sum(max(0, min(e, b + 1) - s) for s, e in parts)
        has = [s <= b for s, e in parts]
    else:
        r = sum(max(0, e - max(s, b)) for s, e in parts)
        has = [e - 1 >= b for s, e in parts]
    head = (not minus) == (not right)
    if minus:
        has = has[::-1]
    numbers = [n + 1 for n, h in enumerate(has) if h]
    exon = 0 if not numbers else (numbers[-1] if head else numbers[0])
    if not parts:
        loc = NONCODING
    elif any(s <= b < e for s, e in parts):
        loc = CDS
    elif parts[0][0] <= b < parts[-1][1]:
        loc = INTRON
    else:
        in_front = (b < parts[0][0]) != minus  # in front of the CDS in transcription order
        loc = UTR5 if in_front else UTR3
    return L, (r if head else L - r), (HEAD if head else TAIL), min(exon, 65535), loc


def per_base(cols, i, P, right, length):
    """the same five numbers from one entry per base of a contig of `length` bases"""
    parts = parts_of(cols, i)
    minus = int(cols["strand"][i]) == 1
    coding = np.zeros(length, bool)
    number = np.zeros(length, np.int64)
    for g, (s, e) in enumerate(parts):
        coding[s:e] = True
        number[s:e] = len(parts) - g if minus else g + 1
    at = np.arange(length)
    retained = at >= P - 1 if right else at <= P - 1
    # transcription steps +1 on '+' and -1 on '-'; the junction lies to the right (+1) of what a LEFT side retains: a head runs towards it
    # (the retained bases then hold the transcript's 5' end; at P == tx_end, or b == tx_start, they hold both ends)
    head = (-1 if minus else 1) == (-1 if right else 1)
    assert retained[int(cols["tx_end"][i]) - 1 if minus else int(cols["tx_start"][i])] or not head or not (int(cols["tx_start"][i]) < P <= int(cols["tx_end"][i]))
    L = int(coding.sum())
    r = int((coding & retained).sum())
    kept = number[coding & retained]
    exon = 0 if not len(kept) else int(kept.max() if head else kept.min())
    b = P - 1
    if L == 0:
        loc = NONCODING
    elif coding[b]:
        loc = CDS
    else:
        where = np.flatnonzero(coding)
        if where[0] < b < where[-1]:
            loc = INTRON
        else:
            upstream = b < where[0]
            loc = (UTR3 if upstream else UTR5) if minus else (UTR5 if upstream else UTR3)
    return L, (r if head else L - r), (HEAD if head else TAIL), exon, loc


def pair_class(a, b):
    """a, b: (L, cod, role, ...) of the transcripts on side 1 and side 2"""
    if a[2] == b[2]:
        return ANTISENSE
    (Lh, h), (Lt, t) = ((a[0], a[1]), (b[0], b[1])) if a[2] == HEAD else ((b[0], b[1]), (a[0], a[1]))
    if 0 < h < Lh and 0 < t < Lt:
        return INFRAME if h % 3 == t % 3 else OUTFRAME
    if h == 0 and t == 0 and Lh > 0 and Lt > 0:
        return PROMOTER
    return TRUNCATING


def expected(cols, sites, info=side_info):
    """abi.FRAME_CALL rows by the definition; `info(cols, i, P, right)` gives a transcript's numbers on a side"""
    out = np.zeros(len(sites), abi.FRAME_CALL)
    for k, s in enumerate(sites):
        side = [(int(s["tid1"]), int(s["pos1"]), int(s["right1"])), (int(s["tid2"]), int(s["pos2"]), int(s["right2"]))]
        over = [overlapping(cols, t, P) for t, P, _ in side]
        infos = [{i: info(cols, i, side[x][1], side[x][2]) for i in over[x]} for x in range(2)]
        o = out[k]
        o["tx"] = -1
        o["n_tx"] = [len(over[0]), len(over[1])]
        chosen = [None, None]
        if over[0] and over[1]:
            best = None
            n_in = n_ok = 0
            for ia in over[0]:
                for ib in over[1]:
                    a, b = infos[0][ia], infos[1][ib]
                    c = pair_class(a, b)
                    n_in += c == INFRAME
                    n_ok += c >= TRUNCATING
                    key = (c, a[0] + b[0], -ia, -ib)
                    if best is None or key > best:
                        best = key
            o["cls"] = best[0]
            chosen = [-best[2], -best[3]]
            o["n_inframe"], o["n_compatible"] = min(n_in, 0xFFFFFFFF), min(n_ok, 0xFFFFFFFF)
        else:
            for x in range(2):
                if over[x]:
                    chosen[x] = max(over[x], key=lambda i: (infos[x][i][0], -i))
        for x in range(2):
            if chosen[x] is None:
                continue
            L, cod, role, exon, loc = infos[x][chosen[x]]
            o["tx"][x], o["cod"][x], o["role"][x], o["exon"][x], o["loc"][x] = chosen[x], cod, role, exon, loc
        if o["cls"] > ANTISENSE:
            o["order"] = 1 if o["role"][0] == HEAD else 2
    return out


# ---- models ------------------------------------------------------------------------------------------------------------------------------
def make_cols(rows):
    """(tid, tx_start, tx_end, strand, parts) rows, already in model order, as the dict of bk_txmodel columns"""
    off, starts, ends = [0], [], []
    for r in rows:
        starts += [p[0] for p in r[4]]
        ends += [p[1] for p in r[4]]
        off.append(len(starts))
    return {"tid": np.asarray([r[0] for r in rows], np.int32), "tx_start": np.asarray([r[1] for r in rows], np.uint32), "tx_end": np.asarray([r[2] for r in rows], np.uint32),
            "strand": np.asarray([r[3] for r in rows], np.uint8), "ex_off": np.asarray(off if rows else [], np.uint32), "ex_start": np.asarray(starts, np.uint32),
            "ex_end": np.asarray(ends, np.uint32)}


def random_transcript(rng, tid, length, max_parts=4):
    a = int(rng.integers(0, length - 20))
    z = int(rng.integers(a + 10, min(length, a + 120) + 1))
    n = int(rng.integers(0, max_parts + 1))
    lo, hi = a + int(rng.integers(0, 4)), z - int(rng.integers(0, 4))  # with and without UTRs
    n = min(n, (hi - lo) // 2)
    cuts = np.sort(rng.choice(np.arange(lo, hi + 1), 2 * n, replace=False)) if n else []
    parts = [(int(cuts[2 * g]), int(cuts[2 * g + 1])) for g in range(n)]
    return (tid, a, z, int(rng.integers(0, 2)), parts)


def random_case(rng, length=160):
    """a model of 0 .. 7 transcripts on contigs 0 and 2 of three (contig 1 has none) and one site; breakpoints on and beside the edges
    of transcripts and parts as often as anywhere"""
    rows = sorted([random_transcript(rng, int(rng.choice([0, 0, 2])), length) for _ in range(int(rng.integers(0, 8)))], key=lambda r: (r[0], r[1]))
    cols = make_cols(rows)
    side = []
    for _ in range(2):
        tid, P = int(rng.choice([0, 0, 0, 2, 1, -1])), int(rng.integers(1, length + 1))
        mine = [r for r in rows if r[0] == tid]
        if mine and rng.random() < 0.8:
            r = mine[int(rng.integers(0, len(mine)))]
            edges = [r[1], r[2]] + [v for p in r[4] for v in p]
            if rng.random() < 0.5:
                P = max(1, min(length, edges[int(rng.integers(0, len(edges)))] + int(rng.integers(0, 2))))
            else:
                P = int(rng.integers(r[1] + 1, r[2] + 1))
        side += [tid, P, int(rng.integers(0, 2))]
    if rows and rng.random() < 0.3:  # both sides in one transcript: an intragenic event
        r = rows[int(rng.integers(0, len(rows)))]
        side[0], side[3] = r[0], r[0]
        side[1], side[4] = sorted(int(v) for v in rng.integers(r[1] + 1, r[2] + 1, 2))
        side[2], side[5] = 0, 1
    return cols, as_sites([tuple(side)])


def nested_locus(n_over, tid=0, base=1_000_000, seed=0):
    """Rows of one nested locus and the site position P inside it: one 2 Mb transcript, 300 short ones inside it that end in front of P
    (the walk backwards passes them), n_over - 1 further transcripts that reach across P, and a few that start behind P.  n_over == 0
    leaves the long one out, so that nothing overlaps P."""
    rng = np.random.default_rng(1000 + seed + n_over)
    P = base + 1_500_000
    rows = []
    if n_over:
        rows.append((tid, base, base + 2_000_000, 0, [(base + 1000, base + 1600), (P - 50, P + 50), (base + 1_900_000, base + 1_900_301)]))
    for k in range(300):
        a = base + 10_000 + 4_000 * k
        rows.append((tid, a, a + 3_000, k & 1, [(a + 100, a + 400), (a + 1000, a + 1000 + 100 + k % 7)]))
    for k in range(max(0, n_over - 1)):
        a = P - 1 - int(rng.integers(0, 200_000))
        z = P + int(rng.integers(0, 50_000))
        n = int(rng.integers(0, 5))
        cuts = np.sort(rng.choice(np.arange(a, z + 1), 2 * n, replace=False)) if z - a >= 2 * n else []
        parts = [(int(cuts[2 * g]), int(cuts[2 * g + 1])) for g in range(len(cuts) // 2)]
        rows.append((tid, a, z, int(rng.integers(0, 2)), parts))
    for k in range(5):
        rows.append((tid, P + 10 * k, P + 10 * k + 5000, k & 1, [(P + 10 * k + 7, P + 10 * k + 300)]))
    return rows, P


# ---- the command line's text ---------------------------------------------------------------------------------------------------------
FRAME_COLUMNS = ["Fr_Class", "Fr_Order", "Fr_Gene1", "Fr_Tx1", "Fr_Loc1", "Fr_Exon1", "Fr_Cod1", "Fr_Phase1", "Fr_Gene2", "Fr_Tx2", "Fr_Loc2", "Fr_Exon2", "Fr_Cod2", "Fr_Phase2",
                 "Fr_Pairs", "Fr_Compatible", "Fr_InFrame"]


def call_fields(call, names, genes):
    """the 17 twin columns of one abi.FRAME_CALL row; names / genes by model index"""
    cls = int(call["cls"])
    f = [abi.FRAME_CLASSES[cls], {0: ".", 1: "5-3", 2: "3-5"}[int(call["order"])]]
    for x in range(2):
        i = int(call["tx"][x])
        if i < 0:
            f += ["."] * 6
            continue
        phase = str(int(call["cod"][x]) % 3) if cls in (INFRAME, OUTFRAME) else "."
        f += [genes[i], names[i], abi.FRAME_LOCS[int(call["loc"][x])], str(int(call["exon"][x])), str(int(call["cod"][x])), phase]
    return f + [str(int(call["n_tx"][0]) * int(call["n_tx"][1])), str(int(call["n_compatible"])), str(int(call["n_inframe"]))]


def info_fields(call, genes):
    """what both breakends of the call end their INFO with"""
    cls, order = int(call["cls"]), int(call["order"])
    s = ""
    if cls != NONE:
        s += ";FRCLASS=" + abi.FRAME_CLASSES[cls]
    if order:
        five, three = (0, 1) if order == 1 else (1, 0)
        s += ";FR5P=%s;FR3P=%s" % (genes[int(call["tx"][five])], genes[int(call["tx"][three])])
    return s

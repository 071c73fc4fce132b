"""Fragment sizes (`bk_fragment_sizes`, `-fragsize`): the definition of include/breakid_hip.h stated twice in numpy, a counter of the
branches a case reaches, seeded small cases without a pipeline, the header's hand example and the command line's formatting of a row.

Both statements take the pair rows as bk_evidence lists them (`ev`, `off`: abi.EVIDENCE rows and the n_clusters + 1 offsets; rows of
another kind are ignored), the record columns (`cols`: tid, pos, flag, qhash, cigar_off, cigar) and the sites (abi.FRAG_SITE)."""
import math

import numpy as np

from breakid_amd import abi

LANE_WALK = 8          # FRAG_LANE_WALK of breakid_amd/csrc/fragsize.h: records of one position a lane walks on its own
SAMPLE_STRIDE = 1024   # 1 << REC_SAMPLE_SHIFT of breakid_amd/csrc/bp.h: the stride of the sampled search keys
I32_MAX = 2**31 - 1
U32 = 0xFFFFFFFF
FRAG_NAMES = ["Fg_N", "Fg_Off", "Fg_Mean", "Fg_Dev", "Fg_Min", "Fg_Max", "Fg_Short", "Fg_Long", "Fg_Z"]
CIGAR_OPS = "MIDNSHP=X"


def cigar_words(text):
    """BAM CIGAR words (len << 4 | op) of a text like 50M10D50M"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | CIGAR_OPS.index(ch))
            num = ""
    return out


def rec_endpos(cols):
    """bam_endpos of every record (bam_endpos_hts of bk_common.h): pos + the reference length of M, D, N, =, X; pos + 1 without a CIGAR
    or with flag 0x4"""
    cig = np.asarray(cols["cigar"]).astype(np.int64)
    off = np.asarray(cols["cigar_off"]).astype(np.int64)
    cons = np.isin(cig & 15, [0, 2, 3, 7, 8])
    csum = np.concatenate([[0], np.cumsum(np.where(cons, cig >> 4, 0))])
    pos = np.asarray(cols["pos"]).astype(np.int64)
    has = (off[1:] > off[:-1]) & ((np.asarray(cols["flag"]) & 4) == 0)
    return np.where(has, pos + csum[off[1:]] - csum[off[:-1]], pos + 1)


def clamp(L):
    return max(-I32_MAX, min(I32_MAX, L))


def row_of(lengths, n_off, n_lost, lo, hi):
    """one abi.FRAG_SIZES row from the lengths of the used rows (Python ints)"""
    r = np.zeros(1, abi.FRAG_SIZES)[0]
    n = len(lengths)
    r["n_used"], r["n_off"], r["n_lost"] = n, n_off, n_lost
    if n:
        s = sum(lengths)
        centre = (2 * s + n) // (2 * n)  # (Python's // floors towards minus infinity)
        r["n_short"] = sum(L < lo for L in lengths)
        r["n_long"] = sum(L > hi for L in lengths)
        r["min"], r["max"], r["sum"] = min(lengths), max(lengths), s
        r["abs_dev"] = sum(abs(L - centre) for L in lengths)
    return r


# ---- statement 1: row by row, the record found by a linear scan ----------------------------------------------------------------------
def row_length(row, site, cols, endpos):
    """('off' | 'lost' | 'used', L, (a_1, a_2)) of one pair row"""
    sides = []
    for s in (1, 2):
        F, right = int(row["flag%d" % s]), int(site["right%d" % s])
        if ((F & 0x10) != 0) != (right != 0):
            return "off", 0, None
    for s in (1, 2):
        T, P, F, right = int(row["tid%d" % s]), int(row["pos%d" % s]), int(row["flag%d" % s]), int(site["right%d" % s])
        hit = np.flatnonzero((cols["tid"] == T) & (cols["pos"].astype(np.int64) == P - 1) & (cols["flag"] == F) & (cols["qhash"] == row["qhash"]))
        if not len(hit):
            return "lost", 0, None
        R = int(hit[0])
        sides.append(int(endpos[R]) - int(site["pos%d" % s]) + 1 if right else int(site["pos%d" % s]) - P + 1)
    return "used", clamp(sides[0] + sides[1]), tuple(sides)


def expected(ev, off, cols, sites, lo, hi, detail=None):
    """the brute-force statement; detail (a list) receives (call, kind, L, (a_1, a_2)) per pair row of a site that is not skipped"""
    endpos = rec_endpos(cols)
    out = np.zeros(len(sites), abi.FRAG_SIZES)
    for c, site in enumerate(sites):
        if site["skip"]:
            continue
        lengths, n_off, n_lost = [], 0, 0
        for r in range(int(off[c]), int(off[c + 1])):
            if ev[r]["kind"] != abi.EV_PAIR:
                continue
            kind, L, a = row_length(ev[r], site, cols, endpos)
            if detail is not None:
                detail.append((c, kind, L, a))
            if kind == "off":
                n_off += 1
            elif kind == "lost":
                n_lost += 1
            else:
                lengths.append(L)
        out[c] = row_of(lengths, n_off, n_lost, lo, hi)
    return out


# ---- statement 2: vectorised, over the records sorted by (tid, pos, flag, qhash, index) ---------------------------------------------------
def first_records(cols, T, P0, F, H):
    """per query (T, P0, F, H) the smallest record index with these four values, len(table) without one.  The table is put in the order of
    lexsort (tid, pos, flag, qhash, index): equal keys are neighbours, the smallest index first; a query is searched in that order"""
    n = len(cols["tid"])
    tid, pos = np.asarray(cols["tid"]).astype(np.int64), np.asarray(cols["pos"]).astype(np.int64)
    flag, qh = np.asarray(cols["flag"]).astype(np.int64), np.asarray(cols["qhash"]).astype(np.uint64)
    order = np.lexsort((np.arange(n), qh, flag, pos, tid))
    # ranks stand for the two wide fields, so that the whole key fits one int64 and searchsorted can take it
    qt = np.asarray(T, np.int64)
    assert (len(tid) == 0 or (tid.min() >= -1 and tid.max() < 2**24)) and (len(qt) == 0 or (qt.min() >= -1 and qt.max() < 2**24))
    loc = np.concatenate([(tid + 1) * 2**32 + (pos + 2**31), (qt + 1) * 2**32 + (np.asarray(P0, np.int64) + 2**31) % 2**32])  # (a P0 outside int32 is no record's: pos_ok)
    pos_ok = (np.asarray(P0, np.int64) >= -2**31) & (np.asarray(P0, np.int64) <= I32_MAX)
    _, loc_rank = np.unique(loc, return_inverse=True)
    _, h_rank = np.unique(np.concatenate([qh, np.asarray(H, np.uint64)]), return_inverse=True)
    n_h = int(h_rank.max()) + 1 if len(h_rank) else 1
    assert (int(loc_rank.max()) + 1 if len(loc_rank) else 1) * 65536 * n_h < 2**62
    key = (loc_rank.astype(np.int64) * 65536 + np.concatenate([flag, np.asarray(F, np.int64)])) * n_h + h_rank
    table, query = key[:n][order], key[n:]
    assert np.all(np.diff(table) >= 0)
    at = np.searchsorted(table, query, side="left")
    found = (at < n) & pos_ok
    found[found] = table[at[found]] == query[found]
    return np.where(found, order[np.minimum(at, max(n - 1, 0))] if n else 0, n)


def expected_sorted(ev, off, cols, sites, lo, hi):
    """the vectorised statement"""
    n_calls = len(sites)
    out = np.zeros(n_calls, abi.FRAG_SIZES)
    call = np.repeat(np.arange(n_calls), np.diff(np.asarray(off).astype(np.int64)))
    keep = (ev["kind"] == abi.EV_PAIR) & (sites["skip"][call] == 0) if len(ev) else np.zeros(0, bool)
    rows, call = ev[keep], call[keep]
    if not len(rows):
        return out
    st = sites[call]
    n = len(cols["tid"])
    endpos = rec_endpos(cols)
    is_off = np.zeros(len(rows), bool)
    lost = np.zeros(len(rows), bool)
    a = []
    for s in ("1", "2"):
        F = rows["flag" + s].astype(np.int64)
        right = st["right" + s] != 0
        is_off |= ((F & 0x10) != 0) != right
        P = rows["pos" + s].astype(np.int64)
        R = first_records(cols, rows["tid" + s], P - 1, F, rows["qhash"])
        lost |= R == n
        E = endpos[np.minimum(R, max(n - 1, 0))] if n else np.zeros(len(rows), np.int64)
        a.append(np.where(right, E - st["pos" + s].astype(np.int64) + 1, st["pos" + s].astype(np.int64) - P + 1))
    lost &= ~is_off
    used = ~is_off & ~lost
    L = np.clip(a[0] + a[1], -I32_MAX, I32_MAX)
    cu, Lu = call[used], L[used]
    n_used = np.bincount(cu, minlength=n_calls).astype(np.int64)
    total = np.zeros(n_calls, np.int64)
    np.add.at(total, cu, Lu)
    centre = np.floor_divide(2 * total + n_used, np.maximum(2 * n_used, 1))
    dev = np.zeros(n_calls, np.int64)
    np.add.at(dev, cu, np.abs(Lu - centre[cu]))
    mn, mx = np.full(n_calls, I32_MAX, np.int64), np.full(n_calls, -I32_MAX - 1, np.int64)
    np.minimum.at(mn, cu, Lu)
    np.maximum.at(mx, cu, Lu)
    out["n_used"] = n_used
    out["n_off"] = np.bincount(call[is_off], minlength=n_calls)
    out["n_lost"] = np.bincount(call[lost], minlength=n_calls)
    out["n_short"] = np.bincount(cu[Lu < lo], minlength=n_calls)
    out["n_long"] = np.bincount(cu[Lu > hi], minlength=n_calls)
    out["min"] = np.where(n_used > 0, mn, 0)
    out["max"] = np.where(n_used > 0, mx, 0)
    out["sum"] = total
    out["abs_dev"] = dev
    return out


# ---- what a case reaches ---------------------------------------------------------------------------------------------------------------------
BRANCHES = ("off_side1", "off_side2", "off_both", "sides_LL", "sides_LR", "sides_RL", "sides_RR", "negative_a", "clamp_high", "clamp_low", "short", "in", "long", "lost",
            "skipped_site", "call_without_used_row", "floor_of_negative_sum")


def branches(ev, off, cols, sites, lo, hi):
    seen = dict.fromkeys(BRANCHES, 0)
    detail = []
    res = expected(ev, off, cols, sites, lo, hi, detail)
    for c, site in enumerate(sites):
        if site["skip"]:
            seen["skipped_site"] += 1
            continue
        r = res[c]
        if not r["n_used"]:
            seen["call_without_used_row"] += 1
        elif int(r["sum"]) < 0 and (2 * int(r["sum"]) + int(r["n_used"])) % (2 * int(r["n_used"])) != 0:
            seen["floor_of_negative_sum"] += 1
        for row in ev[int(off[c]):int(off[c + 1])]:
            if row["kind"] != abi.EV_PAIR:
                continue
            o1 = ((int(row["flag1"]) & 0x10) != 0) != (site["right1"] != 0)
            o2 = ((int(row["flag2"]) & 0x10) != 0) != (site["right2"] != 0)
            if o1 or o2:
                seen["off_both" if o1 and o2 else "off_side1" if o1 else "off_side2"] += 1
    for c, kind, L, a in detail:
        site = sites[c]
        if kind == "lost":
            seen["lost"] += 1
        if kind != "used":
            continue
        seen["sides_" + "LR"[int(site["right1"])] + "LR"[int(site["right2"])]] += 1
        seen["negative_a"] += a[0] < 0 or a[1] < 0
        seen["clamp_high"] += a[0] + a[1] > I32_MAX
        seen["clamp_low"] += a[0] + a[1] < -I32_MAX
        seen["short" if L < lo else "long" if L > hi else "in"] += 1
    return seen


# ---- seeded small cases: a record table, pair rows and sites without a pipeline ----------------------------------------------------------------------
CASE_CIGARS = ["100M", "40S60M", "60M40S", "50M10D50M", "50M1000N50M", "50M5I45M", "30=2X68=", ""]


def build_table(recs):
    """recs: [(tid, pos0, flag, qhash, cigar text)] -> the columns, coordinate sorted (stable), and the new index of every record"""
    order = sorted(range(len(recs)), key=lambda i: ((recs[i][0] if recs[i][0] >= 0 else 1 << 40), recs[i][1]))
    cols = {"tid": np.asarray([recs[i][0] for i in order], np.int32), "pos": np.asarray([recs[i][1] for i in order], np.int32),
            "flag": np.asarray([recs[i][2] for i in order], np.uint16), "qhash": np.asarray([recs[i][3] for i in order], np.uint64)}
    words, offs = [], [0]
    for i in order:
        words += cigar_words(recs[i][4])
        offs.append(len(words))
    cols["cigar"], cols["cigar_off"] = np.asarray(words, np.uint32), np.asarray(offs, np.uint32)
    where = np.empty(len(recs), np.int64)
    where[order] = np.arange(len(recs))
    return cols, where


def as_sites(rows):
    """[(pos1, pos2, right1, right2, skip)] -> abi.FRAG_SITE"""
    out = np.zeros(len(rows), abi.FRAG_SITE)
    for k, (p1, p2, r1, r2, skip) in enumerate(rows):
        out[k]["pos1"], out[k]["pos2"], out[k]["right1"], out[k]["right2"], out[k]["skip"] = p1, p2, r1, r2, skip
    return out


def random_case(rng):
    """(ev, off, cols, sites, lo, hi): 6 to 12 calls of 0 to 14 pair rows each on three contigs.  Sites with every side combination, some
    skipped, some at position 0 or 0xFFFFFFFF; reads whose strand does not fit the site; reads beyond the breakpoint; records that share
    position and hash with another flag, position and flag with another hash, and all four values (the smallest index counts); rows without a
    record; a split row now and then"""
    n_calls = int(rng.integers(6, 13))
    recs, rows, off, site_rows = [], [], [0], []
    next_hash = [int(rng.integers(1, 2**63))]

    def new_hash():
        next_hash[0] += int(rng.integers(1, 1000))
        return next_hash[0]

    for c in range(n_calls):
        t1, t2 = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        r1, r2 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        extreme = rng.random() < 0.2
        p1 = int(rng.choice([0, U32])) if extreme else int(rng.integers(2000, 6000))
        p2 = int(rng.choice([0, U32])) if extreme and rng.random() < 0.7 else int(rng.integers(2000, 6000))
        skip = int(rng.random() < 0.15)
        site_rows.append((p1, p2, r1, r2, skip))
        beyond = rng.random() < 0.25  # every read lies beyond its breakpoint: negative lengths and sums
        m = int(rng.choice([0, 0, 1, 2, 3, 5, 8, 14]))
        for _ in range(m):
            if rng.random() < 0.08:
                row = np.zeros(1, abi.EVIDENCE)[0]
                row["kind"], row["call"] = abi.EV_SPLIT, c
                rows.append(row)
                continue
            h = new_hash()
            row = np.zeros(1, abi.EVIDENCE)[0]
            row["kind"], row["call"], row["qhash"] = abi.EV_PAIR, c, h
            for s, (T, bp, right) in enumerate(((t1, p1, r1), (t2, p2, r2)), 1):
                base = int(rng.integers(2000, 6000)) if bp in (0, U32) else bp
                if right:
                    start = base + int(rng.integers(-150, 200)) - (700 if beyond else 0)
                else:
                    start = base - int(rng.integers(50, 300)) + (700 if beyond else 0)
                rev = bool(right) if rng.random() < 0.85 else not right
                flag = 0x1 | (0x40 if s == 1 else 0x80) | (0x10 if rev else 0)
                cigar = CASE_CIGARS[int(rng.integers(0, len(CASE_CIGARS)))]
                row["tid%d" % s], row["pos%d" % s], row["flag%d" % s] = T, start + 1, flag
                kind = rng.random()
                if kind < 0.06:
                    continue  # no record: the row is lost
                if kind < 0.3:
                    recs.append((T, start, flag ^ 0x20, h, "77M"))          # the same name and position, another flag, in front
                if kind < 0.5:
                    recs.append((T, start, flag, new_hash(), "33M"))         # the same flag, another hash, in front
                recs.append((T, start, flag, h, cigar))
                if 0.4 < kind < 0.6:
                    recs.append((T, start, flag, h, "9M"))                   # all four values again: the smallest index counts
                for _ in range(int(rng.integers(0, 3))):
                    recs.append((T, start + int(rng.integers(-2, 3)), int(rng.integers(0, 2)) * 0x10 | 0x1, new_hash(), "100M"))
            rows.append(row)
        off.append(len(rows))
    cols, _ = build_table(recs if recs else [(0, 0, 0, 1, "1M")])
    ev = np.asarray(rows, abi.EVIDENCE) if rows else np.zeros(0, abi.EVIDENCE)
    lo, hi = [(230, 470), (0, 100), (300, 300), (-50, 5000)][int(rng.integers(0, 4))]
    return ev, np.asarray(off, np.uint64), cols, as_sites(site_rows), lo, hi


# ---- the header's hand example ------------------------------------------------------------------------------------------------------------
HAND_MEAN, HAND_SD = 350.0, 40.0
HAND_SITE = (10000, 50000, 0, 1, 0)
# (start of read 1, 1-based | mate: start 1-based, reverse, CIGAR)
HAND_PAIRS = [(9801, 50101, True, "100M"), (9851, 50051, True, "50M10D50M"), (9901, 49991, True, "40S60M"), (9951, 50201, False, "100M")]


def hand_case():
    recs, rows = [], []
    for k, (s1, s2, rev2, cigar) in enumerate(HAND_PAIRS):
        h = 1000 + k
        f1, f2 = 0x1 | 0x40 | (0x20 if rev2 else 0), 0x1 | 0x80 | (0x10 if rev2 else 0)
        recs += [(0, s1 - 1, f1, h, "100M"), (1, s2 - 1, f2, h, cigar)]
        row = np.zeros(1, abi.EVIDENCE)[0]
        row["kind"], row["qhash"], row["tid1"], row["pos1"], row["flag1"], row["tid2"], row["pos2"], row["flag2"] = abi.EV_PAIR, h, 0, s1, f1, 1, s2, f2
        rows.append(row)
    cols, _ = build_table(recs)
    return np.asarray(rows, abi.EVIDENCE), np.asarray([0, len(rows)], np.uint64), cols, as_sites([HAND_SITE])


# ---- the library's bounds, and how the command line prints a row -------------------------------------------------------------------------------
def bounds(mean, sd):
    """bk_fragment_bounds: (max(0, floor(mean - 3 sd)), ceil(mean + 3 sd)), clamped to int32"""
    three = 3.0 * sd
    a, b = math.floor(mean - three), math.ceil(mean + three)
    return max(0, min(a, I32_MAX)), max(-I32_MAX - 1, min(b, I32_MAX))


def mean_text(r):
    return "%.1f" % (float(int(r["sum"])) / float(int(r["n_used"]))) if r["n_used"] else "."


def z_text(r, mean, sd):
    return "%.2f" % ((float(int(r["sum"])) / float(int(r["n_used"])) - mean) / sd) if r["n_used"] and sd != 0 else "."


def call_fields(r, mean, sd):
    """the nine columns of one call"""
    used = int(r["n_used"])
    return [str(used), str(int(r["n_off"])), mean_text(r), "%.1f" % (float(int(r["abs_dev"])) / float(used)) if used else ".", str(int(r["min"])) if used else ".",
            str(int(r["max"])) if used else ".", str(int(r["n_short"])), str(int(r["n_long"])), z_text(r, mean, sd)]


def info_fields(r, mean, sd):
    """what both breakends of the call end their INFO with"""
    s = ";FGN=%d" % int(r["n_used"])
    if mean_text(r) != ".":
        s += ";FGMEAN=" + mean_text(r)
    if z_text(r, mean, sd) != ".":
        s += ";FGZ=" + z_text(r, mean, sd)
    return s


def touched_rows(n_rows, lookups, walked, used, n_sites):
    """the part of the byte model that is this stage's own (the listing's part is bk_evidence's): 120 bytes per pair row, 80 per looked-up
    record, 18 per walked record, 8 per used side, 80 per site"""
    return n_rows * 120 + lookups * 80 + walked * 18 + 2 * used * 8 + n_sites * 80

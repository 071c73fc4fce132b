"""Known junctions (`bk_known_calls`, `-known`, `-bedpe`): the definition of include/breakid_hip.h in Python, stated twice.  `expected` is a
plain double loop over sites and entries; `expected_sorted` goes through the intervals sorted by (tid, beg) and sets of entries per
breakend.  Also the BEDPE reader and writer of the command line, how it prints a row and an INFO tail, and the byte model.

Definition.  Breakend s of a site is (tid_s, P_s, right_s), P 1-based, x = P - 1.  Interval k of an entry is (tid, [beg, end)), 0-based
and half-open.  dist(x, [b, e)) is 0 when b <= x < e, b - x below the interval and x - (e - 1) at or above end.  A breakend falls into an
interval when the tids are equal and >= 0 and dist <= slop.  Straight: breakend 0 falls into interval 0 and breakend 1 into interval 1;
crossed: 0 into 1 and 1 into 0; a mapping's dist is the sum of its two.  A mapping agrees when both strands are stated and each equals
the side (LEFT = 1 for right 0, RIGHT = 2 for right 1) of the breakend paired with it; it opposes when both are stated and it does not
agree.  An entry is a hit when a mapping holds, once; its mapping is the first by (agrees, smaller dist, straight).  n_hits, n_oriented,
n_opposed, n_names (distinct names among the hits), n_side[s] (entries with an interval that breakend s falls into).  best: the hit with
the largest score (NO_SCORE below every score), then the smaller dist, then the smaller index.

Byte model (bits(x) = x.bit_length()):
  index  per entry 40 + 24 + 48 per radix pass, passes = ceil((32 + bits(max tid + 1)) / 8), 0 without an interval with tid >= 0;
         per such interval 16
  sites  per site 80; per listed hit 12 + 24 per radix pass, passes = ceil(bits(max name) / 8) + ceil(bits(n - 1) / 8)
  known_calls is their sum."""
import math
import re

import numpy as np

from breakid_amd import abi

NO_SCORE = abi.KNOWN_NO_SCORE
NONE, LEFT, RIGHT = abi.STRAND_NONE, abi.STRAND_LEFT, abi.STRAND_RIGHT
KNOWN_COLUMNS = ["Kn_Hits", "Kn_Names", "Kn_Oriented", "Kn_Opposed", "Kn_Best", "Kn_Score", "Kn_BestDist", "Kn_BestMap", "Kn_Side1", "Kn_Side2"]
STRAND_OF = {"+": LEFT, "-": RIGHT}


def as_entries(rows):
    """rows of (tid1, beg1, end1, tid2, beg2, end2, name, score, strand1, strand2)"""
    e = np.zeros(len(rows), abi.KNOWN_ENTRY)
    for k, r in enumerate(rows):
        for f, v in zip(("tid1", "beg1", "end1", "tid2", "beg2", "end2", "name", "score", "strand1", "strand2"), r):
            e[k][f] = v
    return e


def as_sites(rows):
    """rows of (tid1, pos1, right1, tid2, pos2, right2)"""
    s = np.zeros(len(rows), abi.KNOWN_SITE)
    for k, r in enumerate(rows):
        s[k]["tid1"], s[k]["pos1"], s[k]["right1"], s[k]["tid2"], s[k]["pos2"], s[k]["right2"] = r
    return s


def dist(x, b, e):
    return b - x if x < b else x - (e - 1) if x >= e else 0


def breakends(site):
    return [(int(site["tid1"]), int(site["pos1"]) - 1, int(site["right1"]) + 1), (int(site["tid2"]), int(site["pos2"]) - 1, int(site["right2"]) + 1)]


def intervals(entry):
    return [(int(entry["tid1"]), int(entry["beg1"]), int(entry["end1"])), (int(entry["tid2"]), int(entry["beg2"]), int(entry["end2"]))]


def falls(bk, iv, slop):
    """the distance when the breakend falls into the interval, else None"""
    if bk[0] != iv[0] or bk[0] < 0:
        return None
    d = dist(bk[1], iv[1], iv[2])
    return d if d <= slop else None


def hit_of(site, entry, slop):
    """None, or (crossed, agrees, opposes, dist) of the hit's mapping"""
    bk, iv = breakends(site), intervals(entry)
    st1, st2 = int(entry["strand1"]), int(entry["strand2"])
    stated = st1 != NONE and st2 != NONE
    found = None
    for crossed in (0, 1):
        d0, d1 = falls(bk[0], iv[crossed], slop), falls(bk[1], iv[1 - crossed], slop)
        if d0 is None or d1 is None:
            continue
        paired = (bk[1][2], bk[0][2]) if crossed else (bk[0][2], bk[1][2])  # the sides of the breakends paired with strand1, strand2
        agrees = stated and (st1, st2) == paired
        cand = (crossed, agrees, stated and not agrees, d0 + d1)
        if found is None:
            found = cand
        elif (not cand[1], cand[3], cand[0]) < (not found[1], found[3], found[0]):
            found = cand
    return found


def expected(entries, sites, slop):
    """the plain statement: every site against every entry"""
    res = np.zeros(len(sites), abi.KNOWN_CALL)
    for i, site in enumerate(sites):
        r = res[i]
        r["best"], r["best_score"] = -1, NO_SCORE
        names, best = set(), None
        bk = breakends(site)
        for e, entry in enumerate(entries):
            iv = intervals(entry)
            for s in (0, 1):
                if falls(bk[s], iv[0], slop) is not None or falls(bk[s], iv[1], slop) is not None:
                    r["n_side"][s] += 1
            h = hit_of(site, entry, slop)
            if h is None:
                continue
            r["n_hits"] += 1
            r["n_oriented"] += int(h[1])
            r["n_opposed"] += int(h[2])
            names.add(int(entry["name"]))
            score = int(entry["score"])
            if best is None or score > best[0] or (score == best[0] and h[3] < best[1]):  # (e ascends: an equal one stays behind)
                best = (score, h[3], e, h[0], h[1])
        r["n_names"] = len(names)
        if best is not None:
            r["best"], r["best_score"], r["best_dist"], r["best_crossed"], r["best_oriented"] = best[2], best[0], best[1], best[3], int(best[4])
    return res


def expected_sorted(entries, sites, slop):
    """the sorted statement: the intervals with a contig in (tid, beg) order with a running maximum of end; per breakend the intervals
    from the last one that begins at or before x + slop back to where the running maximum no longer reaches x - slop; the entries of
    each breakend as a map entry -> {interval: dist}, and the hits as the entries that both maps hold in a straight or crossed way"""
    iv = []
    for e, entry in enumerate(entries):
        for k, (tid, b, x) in enumerate(intervals(entry)):
            if tid >= 0:
                iv.append((tid, b, 2 * e + k, x))
    iv.sort(key=lambda t: (t[0], t[1], t[2]))
    keys = np.array([(t[0] + 1) << 32 | t[1] for t in iv], np.uint64)
    run_max, prev = [], None
    for t in iv:
        prev = (t[0], t[3]) if prev is None or prev[0] != t[0] else (t[0], max(prev[1], t[3]))
        run_max.append(prev[1])
    res = np.zeros(len(sites), abi.KNOWN_CALL)
    for i, site in enumerate(sites):
        held = []
        for tid, x, _ in breakends(site):
            m = {}
            hi = min(x + slop, 0xFFFFFFFF)
            if tid >= 0 and hi >= 0 and len(iv):
                q = int(np.searchsorted(keys, np.uint64((tid + 1) << 32 | hi), side="right")) - 1
                while q >= 0 and iv[q][0] == tid and run_max[q] - 1 >= x - slop:
                    if iv[q][3] - 1 >= x - slop:
                        m.setdefault(iv[q][2] >> 1, {})[iv[q][2] & 1] = dist(x, iv[q][1], iv[q][3])
                    q -= 1
            held.append(m)
        sides = [b[2] for b in breakends(site)]
        hits = []
        for e in sorted(set(held[0]) & set(held[1])):
            st = (int(entries[e]["strand1"]), int(entries[e]["strand2"]))
            stated = NONE not in st
            maps = []
            if 0 in held[0][e] and 1 in held[1][e]:
                maps.append((not (stated and st == (sides[0], sides[1])), held[0][e][0] + held[1][e][1], 0))
            if 1 in held[0][e] and 0 in held[1][e]:
                maps.append((not (stated and st == (sides[1], sides[0])), held[0][e][1] + held[1][e][0], 1))
            if maps:
                disagrees, d, crossed = min(maps)
                hits.append((-int(entries[e]["score"]), d, e, crossed, not disagrees, stated and disagrees))
        r = res[i]
        r["n_hits"], r["n_oriented"], r["n_opposed"] = len(hits), sum(h[4] for h in hits), sum(h[5] for h in hits)
        r["n_names"] = len({int(entries[h[2]]["name"]) for h in hits})
        r["n_side"] = [len(held[0]), len(held[1])]
        r["best"], r["best_score"] = -1, NO_SCORE
        if hits:
            b = min(hits)
            r["best"], r["best_score"], r["best_dist"], r["best_crossed"], r["best_oriented"] = b[2], -b[0], b[1], b[3], int(b[4])
    return res


def random_case(rng, n_sites, n_entries, slop, n_contigs=3, length=50_000, n_names=6):
    """sites drawn on a few contigs (a third of them with both breakpoints on one contig and close together) and a panel: half of the
    entries drawn freely, the others laid over a site, straight or crossed, with ends up to two slops off, so that every kind of hit,
    tie and miss occurs; scores come from a handful of values and some entries have none"""
    site_rows = []
    for _ in range(n_sites):
        t1 = int(rng.integers(-1, n_contigs)) if rng.random() < 0.05 else int(rng.integers(0, n_contigs))
        p1 = int(rng.integers(1, length))
        if rng.random() < 0.33:
            t2, p2 = t1, max(1, p1 + int(rng.integers(-2 * slop - 2, 2 * slop + 3)))
        else:
            t2, p2 = int(rng.integers(0, n_contigs)), int(rng.integers(1, length))
        site_rows.append((t1, p1, int(rng.integers(0, 2)), t2, p2, int(rng.integers(0, 2))))
    sites = as_sites(site_rows)
    entry_rows = []
    strands = [NONE, LEFT, RIGHT]

    def around(x):
        b = max(0, x + int(rng.integers(-2 * slop - 3, 3)))
        e = max(b + 1, x + 1 + int(rng.integers(-2, 2 * slop + 3)))
        if rng.random() < 0.3:  # beside the breakpoint, at a distance around the slop
            b = x + slop + int(rng.integers(-1, 2)) + 1 if rng.random() < 0.5 else max(0, x - slop - 8 + int(rng.integers(-1, 2)))
            e = b + int(rng.integers(1, 8)) if b > x else max(b + 1, x - slop + int(rng.integers(-1, 2)))
        return b, e

    for _ in range(n_entries):
        score = int(rng.choice([NO_SCORE, 0, 5, 5, 40, -3]))
        name = int(rng.integers(0, n_names))
        s1, s2 = (int(rng.choice(strands)), int(rng.choice(strands))) if rng.random() < 0.4 else (0, 0)
        if rng.random() < 0.5 or not n_sites:
            iv = []
            for _k in range(2):
                b = int(rng.integers(0, length))
                iv.append((int(rng.integers(-1, n_contigs)) if rng.random() < 0.1 else int(rng.integers(0, n_contigs)), b, b + int(rng.integers(1, 4 * slop + 50))))
        else:
            site = sites[int(rng.integers(0, max(1, n_sites // 4)))]  # (the first quarter of the sites: several entries meet at one)
            bk = breakends(site)
            iv = [(bk[k][0],) + around(bk[k][1]) for k in (0, 1)]
            if rng.random() < 0.5:
                s1, s2 = bk[0][2], bk[1][2]
                if rng.random() < 0.3:
                    s1 = 3 - s1
            if rng.random() < 0.4:
                iv, s1, s2 = iv[::-1], s2, s1
            if rng.random() < 0.15:
                iv[1] = (int(rng.integers(0, n_contigs)), 7, 9)  # one partner only
        entry_rows.append(iv[0] + iv[1] + (name, score, s1, s2))
    return as_entries(entry_rows), sites


# ---- the command line's panel file ---------------------------------------------------------------------------------------------------------
class BedpeError(ValueError):
    def __init__(self, line, why):
        ValueError.__init__(self, "line %d: %s" % (line, why))
        self.line, self.why = line, why


_DECIMAL = re.compile(r"^[+-]?((\d+\.?\d*|\.\d+)([eE][+-]?\d+)?|inf(inity)?|nan)$", re.IGNORECASE)
_HEX = re.compile(r"^[+-]?0[xX]([0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)([pP][+-]?\d+)?$")


def score_of(text):
    """the score column: through strtod, truncated towards zero, clamped to int32; what strtod does not take whole, or NaN, is no score"""
    if _HEX.match(text):
        v = float.fromhex(text)
    elif _DECIMAL.match(text):
        v = float(text)
    else:
        return NO_SCORE
    if v != v:
        return NO_SCORE
    return 2147483647 if v >= 2147483647.0 else -2147483648 if v <= -2147483648.0 else int(v)


def read_bedpe(text, contigs):
    """contigs: [(name, length)].  Returns (entries, names by id, lines with a contig the header lacks); BedpeError for a line that ends
    the run"""
    tid_of = {}
    for k, (name, _) in enumerate(contigs):
        tid_of.setdefault(name, k)
    rows, names, ids, unknown = [], [], {}, 0
    for no, line in enumerate(text.split("\n"), 1):
        f = line.split()
        if not f or f[0][0] == "#" or f[0] in ("track", "browser"):
            continue
        if len(f) < 6:
            raise BedpeError(no, "fewer than six fields")
        row, lacking = [], False
        for k in (0, 1):
            try:
                b, e = (int(v) if re.match(r"^[+-]?\d+$", v) else None for v in f[3 * k + 1:3 * k + 3])
            except ValueError:
                b = e = None
            if b is None or e is None or max(abs(b), abs(e)) >= 1 << 63:
                raise BedpeError(no, "not a number")
            tid = -1
            if f[3 * k] not in tid_of:
                lacking = True
            else:
                if b < 0 or e < 0:
                    raise BedpeError(no, "negative coordinate")
                if e <= b:
                    raise BedpeError(no, "end <= start")
                length = contigs[tid_of[f[3 * k]]][1]
                b, e = min(b, length), min(e, length)
                if e > b:
                    tid = tid_of[f[3 * k]]
            row += [tid, b, e] if tid >= 0 else [-1, 0, 0]
        unknown += lacking
        name = f[6] if len(f) > 6 else "."
        if name not in ids:
            ids[name] = len(names)
            names.append(name)
        row += [ids[name], score_of(f[7]) if len(f) > 7 else NO_SCORE]
        row += [STRAND_OF.get(f[k], NONE) if len(f) > k else NONE for k in (8, 9)]
        rows.append(tuple(row))
    return as_entries(rows), names, unknown


def bedpe_line(chr1, p1, chr2, p2, sample, n_drp, n_sr, strand1, strand2, row, fusion_type):
    """one line of -bedpe: each breakpoint as the one-base interval [P - 1, P)"""
    return "\t".join(str(v) for v in (chr1, p1 - 1, p1, chr2, p2 - 1, p2, sample, n_drp + n_sr, strand1, strand2, "bk%d" % row, fusion_type, n_drp, n_sr))


def strand_text(right, source):
    return "." if not source else "-" if right else "+"


def call_fields(r, entries, names):
    """the ten columns that a twin adds for one call"""
    hit = int(r["best"]) >= 0
    return [str(int(r["n_hits"])), str(int(r["n_names"])), str(int(r["n_oriented"])), str(int(r["n_opposed"])),
            names[int(entries[int(r["best"])]["name"])] if hit else ".", str(int(r["best_score"])) if hit and int(r["best_score"]) != NO_SCORE else ".",
            str(int(r["best_dist"])), "." if not hit else "crossed" if r["best_crossed"] else "straight", str(int(r["n_side"][0])), str(int(r["n_side"][1]))]


def info_text(s):
    return re.sub(r"[ \t;=,]", "_", s) if s else "."


def info_fields(r, entries, names):
    """what both breakends of the call end their INFO with"""
    tail = ";KNOWN=%d;KNAMES=%d" % (int(r["n_hits"]), int(r["n_names"]))
    if int(r["best"]) >= 0:
        tail += ";KBEST=" + info_text(names[int(entries[int(r["best"])]["name"])])
    return tail


def touched(entries, sites, hits):
    """the byte model: (index, sites, known_calls)"""
    tids = [t for t in list(entries["tid1"]) + list(entries["tid2"]) if t >= 0]
    passes = math.ceil((32 + (int(max(tids)) + 1).bit_length()) / 8) if tids else 0
    index = len(entries) * (40 + 24 + 48 * passes) + 16 * len(tids)
    max_name = int(entries["name"].max()) if len(entries) else 0
    name_passes = math.ceil(max_name.bit_length() / 8) + math.ceil((max(len(sites), 1) - 1).bit_length() / 8)
    at_sites = len(sites) * 80 + hits * (12 + 24 * name_passes)
    return index, at_sites, index + at_sites

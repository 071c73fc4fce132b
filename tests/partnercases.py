"""Partner loci (`bk_locus_partners`, include/breakid_hip.h) stated twice in Python, for the tests without and with a GPU: a brute-force pass
per site over all ends, and a pass over the sorted index and the sorted runs.  Also the rule of `bk_call_partner_sites`, the byte model
of `bk_timing_touched`, and what the command line prints of a call."""
import numpy as np

from breakid_amd import abi

U32 = 0xFFFFFFFF
PARTNER_NAMES = ["Pt_Ends1", "Pt_Partner1", "Pt_Loci1", "Pt_Top1", "Pt_TopN1", "Pt_Ends2", "Pt_Partner2", "Pt_Loci2", "Pt_Top2", "Pt_TopN2", "Pt_Frac"]


def as_pairs(rows):
    """abi.PAIR rows from (p1_tid, p1_pos, p2_tid, p2_pos): the four fields the definition reads"""
    out = np.zeros(len(rows), abi.PAIR)
    for k, (t1, p1, t2, p2) in enumerate(rows):
        out[k]["p1_tid"], out[k]["p1_pos"], out[k]["p2_tid"], out[k]["p2_pos"] = t1, p1, t2, p2
    return out


def as_sites(rows):
    """abi.PARTNER_SITE rows from (tid, beg, end, mtid, mbeg, mend)"""
    out = np.zeros(len(rows), abi.PARTNER_SITE)
    for k, r in enumerate(rows):
        for f, v in zip(("tid", "beg", "end", "mtid", "mbeg", "mend"), r):
            out[k][f] = v
    return out


def ends_of(pairs):
    """(own tid, own pos, mate tid, mate pos) of the 2 P ends as int64 arrays: end 2 i is side 1 of pair i, end 2 i + 1 side 2"""
    n = len(pairs)
    cols = [np.empty(2 * n, np.int64) for _ in range(4)]
    for c, (a, b) in zip(cols, (("p1_tid", "p2_tid"), ("p1_pos", "p2_pos"), ("p2_tid", "p1_tid"), ("p2_pos", "p1_pos"))):
        c[0::2] = pairs[a]
        c[1::2] = pairs[b]
    return cols


def none_row():
    r = np.zeros(1, abi.LOCUS_PARTNERS)[0]
    r["top_tid"] = -1
    return r


def site_is_empty(s, n_targets):
    return int(s["tid"]) < 0 or int(s["tid"]) >= n_targets or int(s["end"]) < int(s["beg"])


def elsewhere_of(pairs, s, n_targets):
    """the first statement's middle: (ends, to_partner, the mates that go elsewhere as a sorted list of (mtid, mpos))"""
    if site_is_empty(s, n_targets):
        return 0, 0, []
    tid, pos, mtid, mpos = ends_of(pairs)
    own = (tid == int(s["tid"])) & (pos >= int(s["beg"])) & (pos <= int(s["end"]))
    to = own & (mtid == int(s["mtid"])) & (mpos >= int(s["mbeg"])) & (mpos <= int(s["mend"]))
    if int(s["mtid"]) < 0 or int(s["mend"]) < int(s["mbeg"]):
        to[:] = False
    rest = own & ~to
    return int(own.sum()), int(to.sum()), sorted(zip(mtid[rest].tolist(), mpos[rest].tolist()))


def runs_of(mates, max_gap):
    """maximal runs of a sorted list of (mtid, mpos): [(first index, length)]"""
    runs = []
    for k, (t, p) in enumerate(mates):
        if k and mates[k - 1][0] == t and p - mates[k - 1][1] <= max_gap:
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    return runs


def expected(pairs, sites, max_gap, n_targets):
    """the definition, a brute-force pass per site over all ends"""
    out = np.zeros(len(sites), abi.LOCUS_PARTNERS)
    for k, s in enumerate(sites):
        r = none_row()
        ends, to, mates = elsewhere_of(pairs, s, n_targets)
        r["ends"], r["to_partner"] = ends, to
        runs = runs_of(mates, max_gap)
        r["loci"] = len(runs)
        best = None
        for first, length in runs:
            if best is None or length > best[1]:  # strictly greater: a tie goes to the first in sorted order
                best = (first, length)
        if best:
            r["top_n"] = best[1]
            r["top_tid"], r["top_beg"], r["top_end"] = mates[best[0]][0], mates[best[0]][1], mates[best[0] + best[1] - 1][1]
        out[k] = r
    return out


def key_of(tid, pos):
    return ((np.asarray(tid, np.int64) + 1) << 32) | np.asarray(pos, np.int64)


def expected_runs(pairs, sites, max_gap, n_targets, with_rows=False):
    """the same by the way of the kernels: the ends sorted by ((tid + 1) << 32) | pos, two searches per site, the elsewhere mates' keys
    sorted by (site, key), run starts where the contig changes or the gap exceeds max_gap"""
    tid, pos, mtid, mpos = ends_of(pairs)
    own, mate = key_of(tid, pos), key_of(mtid, mpos)
    order = np.argsort(own, kind="stable")
    own, mate = own[order], mate[order]
    out = np.zeros(len(sites), abi.LOCUS_PARTNERS)
    out["top_tid"] = -1
    seg_site, seg_key = [], []
    for k, s in enumerate(sites):
        if site_is_empty(s, n_targets):
            continue
        lo = int(np.searchsorted(own, key_of(int(s["tid"]), int(s["beg"])), "left"))
        hi = int(np.searchsorted(own, key_of(int(s["tid"]), int(s["end"])), "right"))
        m = mate[lo:hi]
        if int(s["mtid"]) >= 0 and int(s["mend"]) >= int(s["mbeg"]):
            to = (m >= key_of(int(s["mtid"]), int(s["mbeg"]))) & (m <= key_of(int(s["mtid"]), int(s["mend"])))
        else:
            to = np.zeros(len(m), bool)
        out[k]["ends"], out[k]["to_partner"] = hi - lo, int(to.sum())
        seg_key.append(m[~to])
        seg_site.append(np.full(int((~to).sum()), k, np.int64))
    n_rows = int(sum(len(x) for x in seg_key))
    if n_rows:
        site, key = np.concatenate(seg_site), np.concatenate(seg_key)
        by_key = np.argsort(key, kind="stable")
        site, key = site[by_key], key[by_key]
        by_site = np.argsort(site, kind="stable")
        site, key = site[by_site], key[by_site]
        start = np.ones(n_rows, bool)
        start[1:] = (site[1:] != site[:-1]) | ((key[1:] >> 32) != (key[:-1] >> 32)) | (key[1:] - key[:-1] > max_gap)
        first = np.flatnonzero(start)
        length = np.diff(np.append(first, n_rows))
        run_site = site[first]
        for k in np.unique(run_site):
            mine = np.flatnonzero(run_site == k)
            top = mine[int(np.argmax(length[mine]))]  # argmax returns the first of equals
            a, b = int(key[first[top]]), int(key[first[top] + length[top] - 1])
            out[k]["loci"], out[k]["top_n"] = len(mine), int(length[top])
            out[k]["top_tid"], out[k]["top_beg"], out[k]["top_end"] = (a >> 32) - 1, a & U32, b & U32
    return (out, n_rows) if with_rows else out


def bits(x):
    return int(x).bit_length()


def row_passes(n_targets, n_sites):
    """the passes of the two sorts of the elsewhere rows (include/breakid_hip.h)"""
    return (32 + bits(n_targets + 1) + 7) // 8 + ((bits(n_sites - 1) if n_sites else 0) + 7) // 8


def touched_index(n_pairs):
    return 56 * n_pairs + 12 * 2 * n_pairs


def touched_sites(n_targets, n_sites, n_rows):
    return 64 * n_sites + 12 * n_rows * row_passes(n_targets, n_sites)


def touched(n_pairs, n_targets, n_sites, n_rows):
    """the byte model of `locus_partners`: the pair rows read, 12 bytes per end of the index, 64 bytes per site, 12 bytes per elsewhere row
    per sort pass"""
    return touched_index(n_pairs) + touched_sites(n_targets, n_sites, n_rows)


def call_sites(cluster, w):
    """bk_call_partner_sites: side s has the window [max(1, ps_min - W), ps_max + W] on ps_tid, W = int(w), and the other side's as its
    partner window"""
    W = int(w)
    win = []
    for s in ("p1", "p2"):
        a, b = max(1, int(cluster[s + "_min"]) - W), min(U32, int(cluster[s + "_max"]) + W)
        a = min(a, U32)
        if b < a:
            a, b = 1, 0
        win.append((int(cluster[s + "_tid"]), a, b))
    return as_sites([win[0] + win[1], win[1] + win[0]])


def top_text(row, names):
    if not int(row["top_n"]):
        return "."
    t = int(row["top_tid"])
    return "%s:%d-%d" % (names[t] if 0 <= t < len(names) else "*", int(row["top_beg"]), int(row["top_end"]))


def call_fields(two, names):
    """the eleven cells of one call from the rows of its two sides"""
    f = []
    for r in two:
        f += [str(int(r["ends"])), str(int(r["to_partner"])), str(int(r["loci"])), top_text(r, names), str(int(r["top_n"]))]
    ends, to = int(two[0]["ends"]) + int(two[1]["ends"]), int(two[0]["to_partner"]) + int(two[1]["to_partner"])
    f.append("%.3f" % (float(to) / float(ends)) if ends else ".")
    return f


def info_fields(row):
    """what a breakend of the call ends its INFO with: the row of its own side"""
    return ";PTN=%d;PTP=%d;PTL=%d" % (int(row["ends"]), int(row["to_partner"]), int(row["loci"]))


HAND_PAIRS = ([(0, 1000 + 10 * k, 1, 5000 + 10 * k) for k in range(5)] + [(0, 1100, 2, 9000), (0, 1110, 2, 9100), (0, 1120, 2, 9500)] +
              [(0, 1200, 0, 80000), (0, 900, 1, 5600)])
HAND_SITE = (0, 800, 1300, 1, 4800, 5300)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------
def random_case(rng, max_gap, n_targets=3, length=50_000, max_pairs=2000):
    """pairs on `n_targets` contigs of `length` bases and sites over them.  Background pairs lie below 0.85 * length; a few hot loci
    send most of their pairs to one partner locus and spray the rest over the other hot loci, unmapped mates (tid -1) and their own
    neighbourhood; above 0.9 * length, where nothing else lies, designed triples of mates stand max_gap and max_gap + 1 apart."""
    quiet = int(length * 0.85)
    rows = []
    n_bg = int(rng.integers(0, max_pairs // 2))
    for _ in range(n_bg):
        t2 = int(rng.integers(-1, n_targets)) if rng.random() < 0.1 else int(rng.integers(0, n_targets))
        rows.append((int(rng.integers(0, n_targets)), int(rng.integers(1, quiet)), t2, int(rng.integers(1, quiet))))
    hot = [(int(rng.integers(0, n_targets)), int(rng.integers(500, quiet - 500))) for _ in range(int(rng.integers(2, 9)))]
    sites = []
    g = min(max_gap, 1000)
    slot = int(length * 0.9)
    for h, (t, p) in enumerate(hot):
        pt, pp = hot[(h + 1) % len(hot)]
        k = int(rng.integers(5, max(6, (max_pairs - n_bg) // len(hot))))
        for _ in range(k):
            own = (t, p + int(rng.integers(-150, 151)))
            u = rng.random()
            if u < 0.6:
                mate = (pt, pp + int(rng.integers(-150, 151)))
            elif u < 0.8:
                ot, op = hot[int(rng.integers(0, len(hot)))]
                mate = (ot, op + int(rng.integers(-60, 61)))
            elif u < 0.9:
                mate = (-1, int(rng.integers(0, 50)))
            else:
                mate = (t, p + int(rng.integers(-3000, 3001)))
            mate = (mate[0], max(1, mate[1]))
            rows.append(own + mate if rng.random() < 0.5 else mate + own)
        if max_gap < U32 and slot + 2 * g + 2 < length:
            qt = int(rng.integers(0, n_targets))
            for q in (slot, slot + g, slot + 2 * g + 1):  # joined at exactly max_gap, split by exactly max_gap + 1
                rows.append((t, p + int(rng.integers(-150, 151)), qt, q))
            slot += 2 * g + 2 + 1500
        a, b = max(1, p - int(rng.integers(0, 400))), p + int(rng.integers(0, 400))
        sites.append((t, a, b, pt, max(1, pp - 200), pp + 200))
        sites.append((t, a, b, -1, 1, U32))                                     # no partner: only elsewhere ends
        sites.append((t, a, b, pt, 1, U32))                                     # the whole partner contig
        sites.append((t, p + 160, p + 150, pt, 1, U32))                         # b < a
        sites.append((t, a, b, pt, pp + 200, pp - 200))                         # mb < ma
        sites.append((pt, max(1, pp - 10), pp + 10, t, 1, U32))                 # a narrow window on the partner: mostly partner ends
    for j in range(3):  # clean junctions between 0.85 and 0.9 * length: every end goes to the partner
        ta, tb = int(rng.integers(0, n_targets)), int(rng.integers(0, n_targets))
        a0, b0 = quiet + 100 + 300 * j, quiet + 1300 + 300 * j
        for _ in range(int(rng.integers(1, 12))):
            rows.append((ta, a0 + int(rng.integers(0, 50)), tb, b0 + int(rng.integers(0, 50))))
        sites.append((ta, a0, a0 + 50, tb, b0, b0 + 50))
        sites.append((tb, b0, b0 + 50, ta, a0, a0 + 50))
    for _ in range(int(rng.integers(5, 40))):
        t, c =int(rng.integers(-1, n_targets + 1)), int(rng.integers(1, length))
        wdt = int(rng.choice([0, 5, 50, 500, 5000]))
        mt, mc = int(rng.integers(-1, n_targets + 1)), int(rng.integers(1, length))
        sites.append((t, max(1, c - wdt), c + wdt, mt, max(1, mc - wdt), mc + wdt))
    sites.append((0, 1, U32, 1, 1, U32))
    order = rng.permutation(len(rows))
    return as_pairs([rows[k] for k in order][:max_pairs]), as_sites(sites)


def branches(pairs, sites, max_gap, n_targets):
    """which branches of the definition the sites reach: counts by name"""
    seen = dict.fromkeys(("no_end", "only_partner", "only_elsewhere", "tie", "top_unmapped_or_own", "split_at_gap_plus_1", "joined_at_gap"), 0)
    for s in sites:
        ends, to, mates = elsewhere_of(pairs, s, n_targets)
        runs = runs_of(mates, max_gap)
        seen["no_end"] += ends == 0
        seen["only_partner"] += ends > 0 and to == ends
        seen["only_elsewhere"] += ends > 0 and to == 0
        if runs:
            longest = max(l for _, l in runs)
            seen["tie"] += sum(l == longest for _, l in runs) > 1
            top = [f for f, l in runs if l == longest][0]
            seen["top_unmapped_or_own"] += mates[top][0] in (-1, int(s["tid"]))
        gaps = [b[1] - a[1] for a, b in zip(mates, mates[1:]) if a[0] == b[0]]
        seen["split_at_gap_plus_1"] += (max_gap + 1) in gaps
        seen["joined_at_gap"] += max_gap in gaps
    return seen

"""Designed candidate tables for the mate join (csrc/join.hip) and a plain Python model of it.  No GPU imports:
tests/test_cpu_join.py checks the model against the oracle on every case and that every case sits on the edge it is named for;
tests/test_gpu_join.py runs the cases.

A table is a list of records under read names; the read-name hashes are then CHOSEN (the way test_gpu_limits overwrites qhash), and
choosing them chooses where every run of equal hashes lands in the join's sorted order: layout() gives that order, so a case can
say "a run of two at sorted positions 255 / 256" and the tests can assert it."""
import numpy as np

from breakid_amd import abi

QUAL = 20
WG = 256           # lanes of a workgroup of k_join_pairs / k_join_fix_runs: one per sorted position
JOIN_FIX_MAX = 64  # csrc/join.hip: the longest mixed run of equal upper hash halves that is put right in place
MASK64 = (1 << 64) - 1
CONTIGS3 = [("chr1", 10_000_000), ("chr2", 10_000_000), ("chr3", 10_000_000)]
# numeric (header) order and string order of "chrA_chrB" differ: chr1 < chr10 < chr11 < chr12 < chr13 < chr2 as strings
CONTIGS13 = [("chr%d" % (k + 1), 2_000_000 + 1000 * k) for k in range(13)]
# prefix sums pass 2^32 at the fourth contig: gpos wraps from chr4 on
CONTIGS_WRAP = [("chr1", 1_500_000_000), ("chr2", 1_500_000_000), ("chr3", 1_200_000_000), ("chr4", 900_000_000), ("chr5", 800_000_000)]


class Case:
    def __init__(self, name, contigs, cols, w, witness=None):
        self.name, self.contigs, self.cols, self.w, self.witness = name, contigs, cols, w, witness or {}


def mix64(k):
    """splitmix64: distinct, well spread hashes for names that no case places"""
    z = (k + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


class Table:
    """records under integer read names; cols() sorts them by coordinate (an unmapped tid of -1 last, as the library compares it)"""

    def __init__(self, contigs):
        self.contigs = contigs
        self.rows = []
        self.hashes = {}
        self.seen = {}

    def add(self, name, tid, pos, mtid=None, mpos=None, flag=None, mapq=60):
        k = self.seen.get(name, 0)
        self.seen[name] = k + 1
        flag = (0x41 if k % 2 == 0 else 0x91) if flag is None else flag
        self.rows.append((name, tid, pos, tid if mtid is None else mtid, pos + 300 if mpos is None else mpos, flag, mapq))

    def set_hash(self, name, h):
        self.hashes[name] = h & MASK64

    def cols(self):
        rows = sorted(enumerate(self.rows), key=lambda e: (e[1][1] & 0xFFFFFFFF, e[1][2], e[0]))
        rows = [r for _, r in rows]
        n = len(rows)
        names = np.array([r[0] for r in rows], np.int64) if n else np.zeros(0, np.int64)
        used = set(self.hashes.values())
        assert len(used) == len(self.hashes)
        qh = np.zeros(n, np.uint64)
        for i, nm in enumerate(names):
            h = self.hashes.get(int(nm))
            if h is None:
                h = mix64(int(nm))
                assert h not in used
            qh[i] = h
        col = lambda j, dt: np.array([r[j] for r in rows], dt) if n else np.zeros(0, dt)
        return {"tid": col(1, np.int32), "pos": col(2, np.int32), "mtid": col(3, np.int32), "mpos": col(4, np.int32), "isize": np.zeros(n, np.int32),
                "flag": col(5, np.uint16), "mapq": col(6, np.uint8), "qhash": qh, "cigar_off": np.arange(n + 1, dtype=np.uint32),
                "cigar": np.full(n, (100 << 4) | 0, np.uint32), "aux_off": np.zeros(n + 1, np.uint32), "aux": np.zeros(0, np.uint8),
                "qcheck": (names + 1).astype(np.uint32)}


# ---- the plain model -----------------------------------------------------------------------------------------------------------------------
def candidate_mask(cols, q=QUAL):
    f = cols["flag"].astype(np.int64)
    return (cols["mapq"].astype(np.int64) >= q) & ((f & 0x400) == 0) & ((f & 0x100) == 0) & ((f & 1) != 0) & ((f & 2) == 0)


def gpos(prefix, nt, tid, pos):
    """combine_genome_chr_pos (util_bam.cc:57-68): uint32 wrap, no offset for tid <= 0, the whole genome for a tid past the list"""
    base = 0 if tid <= 0 else prefix[min(tid, nt)]
    return (base + pos) & 0xFFFFFFFF


def model(contigs, cols, q, w, rec_base=0):
    """(pairs as abi.PAIR in the order of BK_STAGE_SCAN, group offsets): scan_discordant_pairs (BreakID.cc:1424-1512) with a dict as
    the reference's std::map - buffer the first record of a name, pair the second with it, erase"""
    nt = len(contigs)
    prefix = [0]
    for _, l in contigs:
        prefix.append((prefix[-1] + l) & 0xFFFFFFFF)
    rname = lambda t: "*" if t < 0 else contigs[t][0]
    cand = candidate_mask(cols, q)
    buffered, found = {}, []
    for i in np.nonzero(cand)[0]:
        i = int(i)
        h = int(cols["qhash"][i])
        if h not in buffered:
            buffered[h] = i
            continue
        b = buffered.pop(h)
        ct, bt = int(cols["tid"][i]), int(cols["tid"][b])
        dp = abs(int(cols["pos"][i]) - int(cols["pos"][b]))
        if not (rname(bt) != rname(ct) or float(dp) >= float(w)):
            continue
        c1 = gpos(prefix, nt, ct, int(cols["pos"][i]))
        c2 = gpos(prefix, nt, int(cols["mtid"][i]), int(cols["mpos"][i]))
        cur = (int(cols["flag"][i]), ct, (int(cols["pos"][i]) + 1) & 0xFFFFFFFF, int(cols["mapq"][i]))
        buf = (int(cols["flag"][b]), bt, (int(cols["pos"][b]) + 1) & 0xFFFFFFFF, int(cols["mapq"][b]))
        one, two, x, y = (cur, buf, c1, c2) if c1 <= c2 else (buf, cur, c2, c1)
        found.append({"x": x, "y": y, "p1_flag": one[0], "p1_tid": one[1], "p1_pos": one[2], "p1_mapq": one[3], "p2_flag": two[0], "p2_tid": two[1],
                      "p2_pos": two[2], "p2_mapq": two[3], "rec": i + rec_base})
    # sort by (chr-pair key, record); ordinals of the groups in the order of their "chrA_chrB" strings; ids inside the group
    key = lambda p: (p["p1_tid"] + 1) * (nt + 1) + (p["p2_tid"] + 1)
    found.sort(key=lambda p: (key(p), p["rec"]))
    groups = {}
    for p in found:
        groups.setdefault(key(p), []).append(p)
    text = {k: (rname(v[0]["p1_tid"]) + "_" + rname(v[0]["p2_tid"])).encode() for k, v in groups.items()}
    order = sorted(groups, key=lambda k: text[k])
    out = np.zeros(len(found), abi.PAIR)
    off, r = [0], 0
    for ordinal, k in enumerate(order):
        for ident, p in enumerate(groups[k]):
            for f, v in p.items():
                out[f][r] = v
            out["p1_rev"][r] = 1 if p["p1_flag"] & 0x10 else 0
            out["p2_rev"][r] = 1 if p["p2_flag"] & 0x10 else 0
            out["id"][r], out["cluster"][r], out["group"][r] = ident, -1, ordinal
            r += 1
        off.append(r)
    return out, np.array(off, np.uint64)


def layout(cols, q=QUAL):
    """the join's sorted order: [(hash, first sorted position, length)] of every run of equal read-name hashes among the candidates"""
    h = np.sort(cols["qhash"][candidate_mask(cols, q)])
    if not len(h):
        return []
    starts = np.concatenate([[0], np.nonzero(h[1:] != h[:-1])[0] + 1, [len(h)]])
    return [(int(h[a]), int(a), int(b - a)) for a, b in zip(starts[:-1], starts[1:])]


def upper_runs(cols, q=QUAL):
    """[(first sorted position, candidates, names)] of every run of equal UPPER hash halves (what k_join_fix_runs looks at)"""
    out = []
    for h, a, l in layout(cols, q):
        if out and out[-1][3] == h >> 32:
            out[-1][1] += l
            out[-1][2] += 1
        else:
            out.append([a, l, 1, h >> 32])
    return [(a, l, names) for a, l, names, _ in out]


def pairs_per_run(case, q=QUAL):
    """{hash: number of pairs the model forms from that run}"""
    pairs, _ = model(case.contigs, case.cols, q, case.w)
    out = {}
    for r in pairs["rec"]:
        h = int(case.cols["qhash"][int(r)])
        out[h] = out.get(h, 0) + 1
    return out


# ---- case builders ---------------------------------------------------------------------------------------------------------------------------
def runs_table(lengths, seed, contigs=CONTIGS3, close=0.15, hashes="ranked"):
    """one read name per entry of `lengths`, in the join's sorted order when hashes == 'ranked' (name r gets the r-th smallest
    hash; the lower half is scrambled so nothing else follows the rank).  Records arrive in coordinate order, which the seed
    scatters against the hash order.  A share `close` of the records sits 100 bases behind the record of its name in front of
    it: that pair fails the gate |dpos| >= w = 400 when both are on one contig."""
    rng = np.random.default_rng(seed)
    t = Table(contigs)
    slots = rng.permutation(sum(lengths) * 2 + 16)
    s = 0
    for r, L in enumerate(lengths):
        prev = None
        for j in range(L):
            tid, pos = int(rng.integers(0, len(contigs))), 1000 + 700 * int(slots[s])
            s += 1
            if prev is not None and rng.random() < close:
                tid, pos = prev[0], prev[1] + 100
            t.add(r, tid, pos, mtid=int(rng.integers(0, len(contigs))), mpos=int(rng.integers(0, 9_000_000)), mapq=int(rng.integers(QUAL, 61)))
            prev = (tid, pos)
        if hashes == "ranked":
            t.set_hash(r, ((r + 1) << 32) | (mix64(r) & 0xFFFFFFFF))
    return t


def run_length_cases():
    out = []
    for L in (1, 2, 3, 4, 5, 7, 8):
        lengths = [L if k % 3 == 0 else 2 for k in range(150)]
        for tag, hashes in (("ranked", "ranked"), ("spread", None)):
            t = runs_table(lengths, 100 + L, hashes=hashes)
            out.append(Case("runs_of_%d_%s" % (L, tag), t.contigs, t.cols(), 400.0, {"length": L}))
    t = runs_table([(1, 2, 3, 4, 5, 7, 8)[k % 7] for k in range(210)], 99, close=0.3)
    out.append(Case("runs_mixed", t.contigs, t.cols(), 400.0, {"length": 8}))
    return out


def workgroup_cases():
    out = []
    t = runs_table([2] * 127 + [1] + [2] * 40, 201, close=0.0)
    out.append(Case("run_of_2_across_workgroups", t.contigs, t.cols(), 400.0, {"run_at": (WG - 1, 2)}))
    t = runs_table([2] * 127 + [5] + [2] * 40, 202, close=0.0)
    out.append(Case("run_of_5_across_workgroups", t.contigs, t.cols(), 400.0, {"run_at": (WG - 2, 5)}))
    # workgroup 0: every run start yields a pair (128 runs of two - a pair takes two sorted positions, so 128 is the most a
    # workgroup of 256 can hold); workgroup 1: 256 names of one record; workgroup 2: 128 runs of two that all fail the gate
    t = runs_table([2] * 128 + [1] * 256, 203, close=0.0)
    base = len(t.rows)
    for r in range(128):
        t.add(1000 + r, 1, 5_000_000 + 2000 * r)
        t.add(1000 + r, 1, 5_000_000 + 2000 * r + 100)
        t.set_hash(1000 + r, ((1000 + r) << 32) | r)
    assert len(t.rows) == base + 256
    out.append(Case("workgroups_all_none_failing", t.contigs, t.cols(), 400.0, {"full": 0, "single": 1, "failing": 2}))
    t = runs_table([2] * 60 + [9] + [2] * 30 + [12] + [2] * 30, 204, close=0.0)
    out.append(Case("several_pairs_from_one_lane", t.contigs, t.cols(), 400.0, {"length": 12}))
    return out


def shared_upper_table(total, seed, lead=0, one_name=False):
    """`lead` names of one record with small hashes, then `total` candidates whose hashes share one upper half: names of two
    records (and one of a single record when `total` is odd), or - one_name - a single name; then names of two behind them"""
    rng = np.random.default_rng(seed)
    t = Table(CONTIGS3)
    name = 0
    slots = rng.permutation(4 * (lead + total) + 400)
    s = 0

    def put(nm, k):
        nonlocal s
        for _ in range(k):
            t.add(nm, int(rng.integers(0, 3)), 1000 + 700 * int(slots[s]), mtid=int(rng.integers(0, 3)), mpos=int(rng.integers(0, 9_000_000)))
            s += 1

    for _ in range(lead):
        put(name, 1)
        t.set_hash(name, ((name + 1) << 32) | (mix64(name) & 0xFFFFFFFF))
        name += 1
    upper = 0x40000000
    if one_name:
        put(name, total)
        t.set_hash(name, (upper << 32) | 12345)
        name += 1
    else:
        left = total
        while left:
            k = 2 if left >= 2 else 1
            put(name, k)
            t.set_hash(name, (upper << 32) | (mix64(1000 + name) & 0xFFFFFFFF))
            name += 1
            left -= k
    for _ in range(30):
        put(name, 2)
        t.set_hash(name, ((0x50000000 + name) << 32) | (mix64(name) & 0xFFFFFFFF))
        name += 1
    return t


def shared_upper_cases():
    out = []
    for total in (JOIN_FIX_MAX - 1, JOIN_FIX_MAX, JOIN_FIX_MAX + 1):
        t = shared_upper_table(total, 300 + total)
        out.append(Case("mixed_run_of_%d" % total, t.contigs, t.cols(), 400.0, {"upper_run": (0, total, (total + 1) // 2)}))
    t = shared_upper_table(JOIN_FIX_MAX, 310, one_name=True)
    out.append(Case("one_name_run_of_%d" % JOIN_FIX_MAX, t.contigs, t.cols(), 400.0, {"upper_run": (0, JOIN_FIX_MAX, 1)}))
    t = shared_upper_table(12, 311, lead=WG - 6)
    out.append(Case("mixed_run_across_workgroups", t.contigs, t.cols(), 400.0, {"upper_run": (WG - 6, 12, 6)}))
    return out


def gate_case(w):
    """pairs at |dpos| = floor(w) - 1, floor(w), floor(w) + 1 on one contig (both arrival orders of the sides), on two contigs at
    |dpos| = 0, with tid / mtid of -1, with c1 == c2, with gpos wrapped, with mtid past the list"""
    W = int(w)
    nt = len(CONTIGS_WRAP)
    t = Table(CONTIGS_WRAP)
    nm = 0
    for d in (W - 1, W, W + 1):
        for tid in (0, 3):  # chr4: its genome offset has wrapped
            # the mate fields of the record that arrives second decide the sides (c1 <= c2): in front of it, behind it, on it (the
            # tie), unmapped, on a wrapped contig, one and six past the list
            for mt, mp in ((tid, 10), (tid, 2_000_000_000), (tid, None), (-1, -1), (4, 700_000_000), (nt, 77), (nt + 5, 0)):
                base = 100_000 + 10_000 * nm
                t.add(nm, tid, base, mtid=tid, mpos=base + d)
                t.add(nm, tid, base + d, mtid=mt, mpos=base + d if mp is None else mp)
                nm += 1
    for tid_a, tid_b in ((0, 1), (1, 3), (2, 4)):  # different contigs: the distance does not matter
        t.add(nm, tid_a, 500_000, mtid=tid_b, mpos=500_000)
        t.add(nm, tid_b, 500_000, mtid=tid_a, mpos=500_000)
        nm += 1
    # c1 == c2: the mate fields point at the record itself (the tie goes to the record that arrives second as side 1)
    t.add(nm, 2, 800_000, mtid=2, mpos=800_000)
    t.add(nm, 2, 900_000, mtid=2, mpos=900_000)
    nm += 1
    # unmapped ends: tid -1 sorts last; two of them under one name are the same contig "*" and gated by the distance alone
    for d in (W - 1, W, W + 1):
        t.add(nm, -1, 1000 + 10_000 * nm, mtid=-1, mpos=0)
        t.add(nm, -1, 1000 + 10_000 * nm + d, mtid=-1, mpos=0)
        nm += 1
    t.add(nm, 1, 650_000, mtid=-1, mpos=-1)
    t.add(nm, -1, 5, mtid=1, mpos=650_000)
    nm += 1
    t.add(nm, 1, 660_000, mtid=-1, mpos=-1)
    t.add(nm, -1, 900, mtid=0, mpos=5)  # c1 > c2: the unmapped record is side 2
    nm += 1
    return Case("gate_w_%s" % w, t.contigs, t.cols(), float(w), {"w": float(w)})


def group_cases():
    out = []
    t = Table(CONTIGS13)
    nm = 0
    for a in range(13):
        for b in range(a, 13):
            if (a + b) % 2 == 0:
                t.add(nm, a, 10_000 + 1000 * nm, mtid=b, mpos=20_000)
                t.add(nm, b, 900_000 + 1000 * nm, mtid=a, mpos=10_000)
                nm += 1
    t.add(nm, 12, 1_500_000, mtid=-1, mpos=0)  # and "chr13_*"
    t.add(nm, -1, 0, mtid=12, mpos=1_500_000)
    out.append(Case("groups_of_one_pair", t.contigs, t.cols(), 400.0, {"groups": nm + 1, "pairs": nm + 1}))
    t = Table(CONTIGS13)
    for nm in range(300):
        t.add(nm, 9, 10_000 + 1000 * nm, mtid=1, mpos=5)
        t.add(nm, 9, 1_000_000 + 1000 * nm, mtid=1, mpos=5)
    out.append(Case("single_group", t.contigs, t.cols(), 400.0, {"groups": 1, "pairs": 300}))
    t = Table(CONTIGS13)
    for nm in range(300):
        t.add(nm, nm % 13, 10_000 + 1000 * nm)
        if nm % 2:
            t.add(nm, nm % 13, 10_000 + 1000 * nm + 50)
    out.append(Case("no_pair", t.contigs, t.cols(), 400.0, {"groups": 0, "pairs": 0}))
    t = Table(CONTIGS13)
    for nm in range(40):
        t.add(nm, nm % 13, 10_000 + 1000 * nm, flag=0x63)
    out.append(Case("no_candidate", t.contigs, t.cols(), 400.0, {"groups": 0, "pairs": 0}))
    # many groups of very different sizes, names in both orders of the sides
    t = runs_table([2] * 900 + [3] * 50, 401, contigs=CONTIGS13, close=0.1, hashes=None)
    out.append(Case("groups_of_all_sizes", t.contigs, t.cols(), 400.0, {"groups": 30, "pairs": 500}))
    return out


def table_cases():
    return run_length_cases() + workgroup_cases() + shared_upper_cases() + [gate_case(500), gate_case(350.5)] + group_cases()


MAX_RECORDS = 20_000
REC_BASES = (0, 1 << 31, 1 << 40)
REC_BASE_LIMIT = 1 << 60  # 61 record bits and the 8 bits of 14 x 14 chr-pair keys do not fit the 64-bit sort key


def rec_bits_case():
    t = runs_table([2] * 400 + [3] * 40, 501, contigs=CONTIGS13, close=0.1, hashes=None)
    return Case("measured_rec_bits", t.contigs, t.cols(), 400.0)

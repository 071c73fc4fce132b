"""Designed record tables for the stream pass (csrc/stream.hip: k_stream, launch_stream, run_stream) and the plain numpy definition
of what the pass must give: the candidate rows (abi.CAND), the indices of the SA-bearing records, the insert-size sums and max_span.
No GPU imports: tests/test_cpu_stream.py checks the definition against the oracle and that every case sits on the edge it is named
for; tests/test_gpu_stream.py runs the cases.

A table is described record by record (Plan): is_candidate, has_sa, is_proper, isize and the CIGAR words; flag, mapq, tid and pos
may be given outright.  The geometry of the kernel - which block and which iteration a record belongs to under a cap on the grid,
what the two LDS bins hold at every look - is modelled by Geo from the constants of the build (capi.stream_info), so a case says
where it sits and the tests assert that it does."""
import numpy as np

from breakid_amd import abi

TODAY = {"STREAM_V": 4, "ST_CAND_CAP": 640, "ST_SA_CAP": 1024}  # csrc/stream.h, csrc/stream.hip (capi.stream_info of today's build)
QUAL = 20
CONTIGS = [("chr1", 50_000_000), ("chr2", 40_000_000), ("chr3", 30_000_000)]
M100 = (100 << 4) | 0
OWN_SPLIT = [(60 << 4) | 0, (40 << 4) | 4]  # 60M40S: complementary to the SA text below, so the record yields an evidence tuple
SA_TEXT = "chr2,%d,+,60S40M,60,0;"
LONG_CIGAR = [(3000 << 4) | 0, (7 << 4) | 2, (2000 << 4) | 0, (5 << 4) | 4]  # 3000M7D2000M5S: 5007 reference bases
LONG_SPAN = 5007
ELIGIBLE_MASK = 0x4 | 0x100 | 0x200 | 0x400


class Geo:
    """The launch geometry of k_stream: V records per lane and iteration, B = 256 V records per block and iteration, a look at the
    bins after every fourth iteration of a block and after its last."""

    def __init__(self, info=None):
        info = dict(TODAY if info is None else info)
        self.V = info["STREAM_V"]
        self.B = 256 * self.V
        self.CC = info["ST_CAND_CAP"]
        self.SC = info["ST_SA_CAP"]
        self.W = 4 * self.B  # records of a flush window of one block

    def blocks(self, n, cap, resident=0):
        """the grid launch_stream takes for n records (q_begin = 0); cap / resident 0 = unknown or none"""
        b = (n // self.V + 1 + 255) // 256
        if resident:
            b = min(b, resident)
        if cap:
            b = min(b, cap)
        return b

    def iterations(self, n, blocks):
        return -(-(n // self.V) // (blocks * 256))

    def per_iteration(self, mask, blocks):
        """counts[block][iteration] of the set records of `mask` among the full groups of V records (the tail is not staged)"""
        n = len(mask)
        nq = n // self.V
        iters = self.iterations(n, blocks)
        c = np.zeros((blocks, max(iters, 1)), np.int64)
        idx = np.nonzero(np.asarray(mask[:nq * self.V], bool))[0]
        chunk = idx // self.B  # a block's records of one iteration
        np.add.at(c, (chunk % blocks, chunk // blocks), 1)
        return c[:, :iters]

    def bin_events(self, counts, cap):
        """One block's bin over its iterations: [(iteration, held at the look, flushed)] for every look, and the number of
        entries that found the bin full and went straight to global memory."""
        held, spilled, looks = 0, 0, []
        iters = len(counts)
        for it, c in enumerate(counts):
            spilled += max(0, held + int(c) - max(held, cap))
            held += int(c)
            last = it == iters - 1
            if not (last or (it + 1) % 4 == 0):
                continue
            nc = min(held, cap)
            flush = bool(nc) and (nc >= cap // 2 or last)
            looks.append((it, nc, flush))
            if flush:
                held = 0
        return looks, spilled


class Plan:
    def __init__(self, n, name=""):
        self.name = name
        self.n = n
        self.is_candidate = np.zeros(n, bool)
        self.has_sa = np.zeros(n, bool)
        self.is_proper = np.zeros(n, bool)
        self.isize = np.zeros(n, np.int32)
        self.cigar = {}   # record -> list of CIGAR words (default: 100M; 60M40S for a record with SA text)
        self.flag = None  # explicit columns (the flag-gate table, the order-check tables)
        self.mapq = None
        self.tid = None
        self.pos = None


def spread(lo, hi, count):
    """`count` distinct record indices in [lo, hi), evenly spread (all four waves, several lanes of a group of V)"""
    assert 0 <= count <= hi - lo, (lo, hi, count)
    if count == 0:
        return np.zeros(0, np.int64)
    return lo + (np.arange(count, dtype=np.int64) * (hi - lo)) // count


def build(plan):
    """(contigs, cols): the coordinate-sorted SoA table of a plan, every column Context.upload takes"""
    n = plan.n
    i = np.arange(n, dtype=np.int64)
    assert not np.any(plan.is_candidate & plan.is_proper)
    if plan.flag is None:
        flag = np.where(plan.is_proper, np.where(i % 2 == 0, 0x63, 0x93), np.where(i % 2 == 0, 0x41, 0x91)).astype(np.uint16)
        # neither candidate nor proper: below the quality threshold, or (no SA text to gate) not paired at all
        mapq = np.where(plan.is_candidate | plan.is_proper, 60, QUAL - 1).astype(np.uint8)
        unpaired = ~plan.is_candidate & ~plan.is_proper & ~plan.has_sa & (i % 3 == 0)
        flag[unpaired] = 0x10
        mapq[unpaired] = 60
    else:
        flag, mapq = np.asarray(plan.flag, np.uint16), np.asarray(plan.mapq, np.uint8)
    tid = np.zeros(n, np.int32) if plan.tid is None else np.asarray(plan.tid, np.int32)
    pos = (1000 + 3 * i).astype(np.int32) if plan.pos is None else np.asarray(plan.pos, np.int32)
    words, aux = [], bytearray()
    coff, aoff = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    for k in range(n):
        w = plan.cigar.get(k)
        if w is None:
            w = OWN_SPLIT if plan.has_sa[k] else [M100]
        words.extend(w)
        coff[k + 1] = len(words)
        if plan.has_sa[k]:
            aux += (SA_TEXT % (5000 + k)).encode()
        aoff[k + 1] = len(aux)
    pair = i // 2  # neighbours share a read name: with w = 0 the oracle's mate join pairs the candidates two by two
    cols = {"tid": tid, "pos": pos, "mtid": (i % 3).astype(np.int32), "mpos": (7 * i + 3).astype(np.int32), "isize": np.asarray(plan.isize, np.int32),
            "flag": flag, "mapq": mapq, "qhash": ((pair + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)), "cigar_off": coff,
            "cigar": np.asarray(words, np.uint32), "aux_off": aoff, "aux": np.frombuffer(bytes(aux), np.uint8).copy(), "qcheck": (pair + 1).astype(np.uint32)}
    return CONTIGS, cols


# ---- the plain definition ----------------------------------------------------------------------------------------------------------------
def candidate_mask(cols, q=QUAL):
    """BreakID.cc:1419-1420: mapq >= q && !DUP && !SECONDARY && PAIRED && !PROPER_PAIR"""
    f = cols["flag"].astype(np.int64)
    return (cols["mapq"].astype(np.int64) >= q) & ((f & 0x400) == 0) & ((f & 0x100) == 0) & ((f & 1) != 0) & ((f & 2) == 0)


def sa_mask(cols):
    """BreakID.cc:898: SA text present, !DUP, PAIRED"""
    f = cols["flag"].astype(np.int64)
    return (np.diff(cols["aux_off"].astype(np.int64)) > 0) & ((f & 0x400) == 0) & ((f & 1) != 0)


def isize_mask(cols):
    """BreakID.cc:1932: PAIRED && PROPER && !(UNMAP | SECONDARY | QCFAIL | DUP)"""
    f = cols["flag"].astype(np.int64)
    return ((f & 1) != 0) & ((f & 2) != 0) & ((f & ELIGIBLE_MASK) == 0)


def spans(cols):
    """bam_endpos - pos of every record: the reference bases of its CIGAR (M, D, N, =, X), 1 without CIGAR or with UNMAP"""
    n = len(cols["tid"])
    w = cols["cigar"].astype(np.int64)
    use = np.isin(w & 15, (0, 2, 3, 7, 8))
    run = np.concatenate([[0], np.cumsum(np.where(use, w >> 4, 0))])
    off = cols["cigar_off"].astype(np.int64)
    ref = run[off[1:]] - run[off[:-1]]
    plain = ((cols["flag"].astype(np.int64) & 4) != 0) | (off[1:] == off[:-1])
    return np.where(plain, 1, ref)[:n]


class Expected:
    pass


def expected(cols, q=QUAL, rec_base=0):
    e = Expected()
    n = len(cols["tid"])
    c = np.nonzero(candidate_mask(cols, q))[0]
    rows = np.zeros(len(c), abi.CAND)
    rows["qhash"], rows["rec"] = cols["qhash"][c], c.astype(np.uint64) + np.uint64(rec_base)
    for k in ("tid", "pos", "mtid", "mpos", "flag", "mapq"):
        rows[k] = cols[k][c]
    rows["qcheck"] = cols["qcheck"][c] if "qcheck" in cols else 0
    e.cand = rows
    e.sa = np.nonzero(sa_mask(cols))[0]
    v = np.abs(cols["isize"].astype(np.int64))[isize_mask(cols)]
    e.isize_sum, e.isize_n = int(v.sum()), len(v)
    e.vmax = int(v.max()) if len(v) else 0
    sq = int((v * v).sum())
    assert sq < 2 ** 53  # every partial sum is an integer below 2^53: the double sum is exact in any order
    e.sumsq = float(sq)
    e.max_span = max(1, int(spans(cols).max())) if n else 1
    return e


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _fill_isize(p, seed):
    rng = np.random.default_rng(seed)
    p.isize[:] = rng.integers(-20000, 20001, p.n)
    return p


def window_case(geo, kind, first, tag=None, second=3, tail=None):
    """cap 1: `first` entries of `kind` ('cand', 'sa' or 'both') in the first flush window of the one block, `second` in the next
    window (one more iteration, the last), and a tail"""
    tail = geo.V - 1 if tail is None else tail
    p = Plan(geo.W + geo.B + tail, "%s_%s" % (kind, tag or first))
    a = spread(0, geo.W, first)
    b = spread(geo.W, geo.W + geo.B, second) + 1
    for m in ((p.is_candidate, p.has_sa) if kind == "both" else (p.is_candidate,) if kind == "cand" else (p.has_sa,)):
        m[a] = True
        m[b] = True
    p.is_proper[:] = ~p.is_candidate & (np.arange(p.n) % 5 == 0)
    return _fill_isize(p, first)


def cand_edges(geo):
    return [geo.CC // 2 - 1, geo.CC // 2, geo.CC - 1, geo.CC, geo.CC + 1, geo.W]


def sa_edges(geo):
    return [geo.SC // 2 - 1, geo.SC // 2, geo.SC - 1, geo.SC, geo.SC + 1, geo.W]


def both_bins_cases(geo):
    """the look after the fourth iteration finds: only the candidate bin half full, only the SA bin, both"""
    out = []
    for tag, nc, ns in (("cand_only", geo.CC // 2, geo.SC // 2 - 1), ("sa_only", geo.CC // 2 - 1, geo.SC // 2), ("both", geo.CC // 2, geo.SC // 2)):
        p = Plan(geo.W + geo.B + 1, "bins_" + tag)
        p.is_candidate[spread(0, geo.W, nc)] = True
        p.has_sa[spread(0, geo.W, ns) ^ 1] = True
        p.is_candidate[geo.W + 5] = p.has_sa[geo.W + 6] = True
        p.is_proper[:] = ~p.is_candidate & (np.arange(p.n) % 2 == 0)
        out.append((tag, _fill_isize(p, nc + ns)))
    return out


def order_of_flushes_case(geo, first):
    """cap 1: `first` candidates in the first window, EVERY record of the second window (two iterations) a candidate.  When the
    look after the fourth iteration flushes (first >= ST_CAND_CAP / 2) the first rows of the buffer are the first window's;
    when it does not, the second window overflows the bin and its direct appends come first."""
    p = Plan(geo.W + 2 * geo.B, "flush_order_%d" % first)
    p.is_candidate[spread(0, geo.W, first)] = True
    p.is_candidate[geo.W:] = True
    return _fill_isize(p, first)


GEOMETRY_CAPS = (1, 2, 3, 0)
GEOMETRY_K = (1, 4, 5)


def geometry_rests(geo):
    return [0, 1, geo.V - 1, geo.V, geo.B - 1, geo.B + 1]


def random_plan(n, seed, name="", cand=0.3, sa=0.1, proper=0.4):
    rng = np.random.default_rng(seed)
    p = Plan(n, name)
    u = rng.random(n)
    p.is_candidate[:] = u < cand
    p.is_proper[:] = (u >= cand) & (u < cand + proper)
    p.has_sa[:] = rng.random(n) < sa
    p.isize[:] = rng.integers(-20000, 20001, n)
    for k in np.nonzero(rng.random(n) < 0.05)[0]:  # CIGARs of other lengths, so that the offsets move unevenly
        p.cigar[int(k)] = [(30 << 4) | 4, (50 << 4) | 0, (int(rng.integers(1, 400)) << 4) | 3, (20 << 4) | 0][: int(rng.integers(1, 5))]
    return p


def geometry_case(geo, cap, k, rest):
    n = k * geo.B * max(cap, 1) + rest
    return random_plan(n, 1000 * cap + 10 * k + rest, "geometry_cap%d_k%d_r%d" % (cap, k, rest))


def tail_only_sizes(geo):
    return [1, geo.V - 1]


def places(geo, n):
    """record indices where k_stream takes a neighbour's value another way: from the lane beside it, from global memory at the edge
    of a wave, of the table, of an iteration, and in the tail path"""
    nq = n // geo.V
    assert n - nq * geo.V >= 2 and nq * geo.V > geo.B + 64 * geo.V
    return {"inside_a_group": 10 * geo.V + 1, "between_groups_of_a_wave": 11 * geo.V, "last_lane_of_a_wave": 64 * geo.V - 1, "lane_0_of_a_wave": 64 * geo.V,
            "iteration_boundary": geo.B, "first_of_last_group": nq * geo.V - geo.V, "last_of_last_group": nq * geo.V - 1, "first_tail_record": nq * geo.V,
            "last_record": n - 1}


def places_n(geo):
    return geo.B + 70 * geo.V + geo.V - 1  # cap 1: two iterations and a tail of V - 1 records


def neighbour_case(geo, place):
    """the record at `place` alone carries the long CIGAR (max_span), SA text and is a candidate; its neighbours are plain"""
    n = places_n(geo)
    at = places(geo, n)[place]
    p = Plan(n, "neighbour_" + place)
    p.is_candidate[at] = p.has_sa[at] = True
    p.cigar[at] = LONG_CIGAR
    p.has_sa[spread(0, n, 40)] = True
    for k in (at - 1, at + 1):
        if 0 <= k < n:
            p.has_sa[k] = False
    p.is_proper[:] = ~p.is_candidate & (np.arange(n) % 7 == 0)
    return _fill_isize(p, at), at


def unsorted_case(geo, place, by):
    """one inversion between the record at `place` and the one in front of it, by position or by contig"""
    n = places_n(geo)
    at = places(geo, n)[place]
    p = random_plan(n, at, "unsorted_%s_%s" % (place, by))
    i = np.arange(n, dtype=np.int64)
    p.pos, p.tid = 1000 + 3 * i, np.ones(n, np.int64)
    if by == "pos":
        p.pos[at - 1] += 5
    else:
        p.tid[at] = 0
    return p, at


def equal_neighbours_case(geo):
    """the record at every place has the position of the one in front of it: sorted"""
    n = places_n(geo)
    p = random_plan(n, 77, "equal_neighbours")
    i = np.arange(n, dtype=np.int64)
    p.pos, p.tid = 1000 + 3 * i, np.ones(n, np.int64)
    for at in places(geo, n).values():
        p.pos[at] = p.pos[at - 1]
    return p


def inversions(cols):
    t, q = cols["tid"].astype(np.int64) & 0xFFFFFFFF, cols["pos"].astype(np.int64)
    return np.nonzero((t[:-1] > t[1:]) | ((t[:-1] == t[1:]) & (q[:-1] > q[1:])))[0] + 1


def capacity_cases():
    """more candidates / SA-bearing records than the first pass of run_stream gives room for"""
    a = Plan(80_000, "capacity_candidates")
    a.is_candidate[spread(0, 80_000, 70_000)] = True
    a.is_proper[:] = ~a.is_candidate
    b = Plan(40_000, "capacity_sa")
    b.has_sa[spread(0, 40_000, 20_000)] = True
    b.is_candidate[spread(0, 40_000, 900)] = True
    b.is_proper[:] = ~b.is_candidate & (np.arange(40_000) % 2 == 0)
    return [_fill_isize(a, 1), _fill_isize(b, 2)]


def first_capacity(n):
    """(cand_cap, sa_cap) of the first attempt of run_stream on a fresh context (api.hip: stream_prepare)"""
    return max(1 << 16, n // 8 + 1024), max(1 << 14, n // 16 + 1024)


GATE_BITS = (0x1, 0x2, 0x4, 0x100, 0x200, 0x400)  # PAIRED, PROPER, UNMAP, SECONDARY, QCFAIL, DUP


def flag_gate_case(q=QUAL):
    """one record of every combination of the six flag bits the three predicates read, with mapq q - 1 and q; every record carries SA
    text and a non-zero insert size, so only the flags and mapq decide the three memberships"""
    flags, mapq = [], []
    for m in range(64):
        f = sum(b for j, b in enumerate(GATE_BITS) if m >> j & 1)
        for mq in (q - 1, q):
            flags.append(f | 0x40)
            mapq.append(mq)
    n = len(flags)
    p = Plan(n, "flag_gates")
    p.flag, p.mapq = np.array(flags), np.array(mapq)
    p.has_sa[:] = True
    p.isize[:] = 100 + np.arange(n)
    return p


def take(cols, idx):
    """the table of the records `idx` (in that order; offsets rebuilt)"""
    idx = np.asarray(idx, np.int64)
    out = {k: np.ascontiguousarray(v[idx]) for k, v in cols.items() if k not in ("cigar_off", "cigar", "aux_off", "aux")}
    for blob, off in (("cigar", "cigar_off"), ("aux", "aux_off")):
        o = cols[off].astype(np.int64)
        parts = [cols[blob][o[i]:o[i + 1]] for i in idx]
        out[off] = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32)
        out[blob] = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, cols[blob].dtype)
    return out

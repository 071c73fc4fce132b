"""Window coverage (`bk_window_coverage`, `-coverage`): the definition of include/breakid_hip.h in numpy, independent of the prefix sums
the library uses.  `bases` comes from a difference array per contig (one entry per base; for a contig too long for that, one entry per
coordinate at which the depth can change), `reads` from a direct interval test.  `bk_call_windows` and the command line's column
formatting are stated here in Python as well, and the record tables the GPU tests share are built here."""
import numpy as np

from breakid_amd import abi

NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
CONSUMES_REF = (0, 2, 3, 7, 8)  # M D N = X
DENSE_MAX = 8_000_000  # contigs up to this length get a per-base array
COLUMNS = ["Cov_L1", "Cov_R1", "Cov_L2", "Cov_R2", "Cov_Span", "Cov_SpanRatio", "Cov_Contig1", "Cov_Contig2"]
OPS = "MIDNSHP=X"


# ---- record tables ----------------------------------------------------------------------------------------------------------------------
def words(text):
    """'40S60M' -> BAM CIGAR words"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | OPS.index(ch))
            num = ""
    return out


def make_cols(recs):
    """recs: (tid, pos, flag, mapq, cigar text) in any order -> a host table in coordinate order (tid -1 last; stable), with every
    column bk_upload_records takes; no aux bytes, read names by number"""
    order = sorted(range(len(recs)), key=lambda k: ((recs[k][0] if recs[k][0] >= 0 else 1 << 40), recs[k][1]))
    n = len(recs)
    cig, off = [], [0]
    for k in order:
        cig += words(recs[k][4])
        off.append(len(cig))
    col = lambda j, dt: np.asarray([recs[k][j] for k in order], dt).reshape(n)
    return {"tid": col(0, np.int32), "pos": col(1, np.int32), "mtid": np.full(n, -1, np.int32), "mpos": np.full(n, -1, np.int32), "isize": np.zeros(n, np.int32),
            "flag": col(2, np.uint16), "mapq": col(3, np.uint8), "qhash": (np.arange(n, dtype=np.uint64) + 1) * np.uint64(0x9E3779B97F4A7C15),
            "qcheck": np.arange(n, dtype=np.uint32) + 1, "cigar_off": np.asarray(off, np.uint32), "cigar": np.asarray(cig, np.uint32), "aux_off": np.zeros(n + 1, np.uint32),
            "aux": np.zeros(0, np.uint8)}


def random_table(rng, n, contigs, read_len=150, unmapped=0, step=None):
    """n single-word reads spread over the contigs (tid, length), mapq 0..60, about a tenth with one of the five barred flags, a few
    with a clip-only CIGAR or a deletion; `unmapped` records with tid -1 behind them"""
    recs = []
    barred = (0x4, 0x100, 0x200, 0x400, 0x800)
    for k in range(n):
        tid, length = contigs[int(rng.integers(0, len(contigs)))]
        pos = int(rng.integers(0, max(1, length - 2 * read_len))) if step is None else (k * step) % max(1, length - 2 * read_len)
        flag = 0x1 | (barred[int(rng.integers(0, 5))] if rng.random() < 0.1 else 0)
        kind = rng.random()
        third = max(1, read_len // 3)
        cigar = ("%dM" % read_len if kind < 0.8 else "%dS%dM" % (third, read_len - third) if kind < 0.9 else "%dM7D%dM" % (third, read_len - third) if kind < 0.97
                 else "%dS" % read_len)
        recs.append((tid, pos, flag, int(rng.integers(0, 61)), cigar))
    for k in range(unmapped):
        recs.append((-1, -1, 0x4, 0, "%dS" % read_len if k & 1 else ""))
    return make_cols(recs)


def as_windows(rows):
    w = np.zeros(len(rows), abi.COV_WINDOW)
    for k, r in enumerate(rows):
        w[k]["tid"], w[k]["beg"], w[k]["end"] = r[0], r[1], r[2]
    return w


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def eligible_len(cols, mapq_min):
    """per record: the reference length of its CIGAR when it is eligible, 0 otherwise"""
    cig = cols["cigar"].astype(np.int64)
    off = cols["cigar_off"].astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(np.where(np.isin(cig & 15, CONSUMES_REF), cig >> 4, 0))])
    ln = csum[off[1:]] - csum[off[:-1]]
    ok = (cols["tid"] >= 0) & ((cols["flag"].astype(np.int64) & NEVER) == 0) & (cols["mapq"].astype(np.int64) >= mapq_min)
    return np.where(ok, ln, 0)


def expected_cov(cols, n_targets, windows, mapq_min):
    """one abi.WINDOW_COV row per window"""
    windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
    out = np.zeros(len(windows), abi.WINDOW_COV)
    ln = eligible_len(cols, mapq_min)
    tid = cols["tid"].astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    end = pos + ln
    live = [(k, int(w["tid"]), int(w["beg"]), int(w["end"])) for k, w in enumerate(windows) if 0 <= int(w["tid"]) < n_targets and int(w["end"]) > int(w["beg"])]
    for T in sorted({t for _, t, _, _ in live}):
        m = (tid == T) & (ln > 0)
        p, e = pos[m], end[m]
        mine = [(k, a, b) for k, t, a, b in live if t == T]
        top = int(e.max()) if len(e) else 0
        if top <= DENSE_MAX:
            diff = np.zeros(top + 2, np.int64)
            np.add.at(diff, np.clip(p, 0, top + 1), 1)  # (a pos below 0 covers from base 0 on: no window reaches below it)
            np.add.at(diff, e, -1)
            filled = np.concatenate([[0], np.cumsum(np.cumsum(diff)[:-1])])  # filled[x] = covered bases in [0, x)
            at = lambda x: int(filled[min(x, top + 1)])
        else:
            xs = np.unique(np.concatenate([p, e, [0]]))
            d = np.zeros(len(xs), np.int64)
            np.add.at(d, np.searchsorted(xs, p), 1)
            np.add.at(d, np.searchsorted(xs, e), -1)
            depth = np.cumsum(d)  # on [xs[j], xs[j + 1])
            filled = np.concatenate([[0], np.cumsum(depth[:-1] * np.diff(xs))])  # covered bases in [xs[0], xs[j])

            def at(x):
                j = int(np.searchsorted(xs, x, side="right")) - 1
                return 0 if j < 0 else int(filled[j]) + int(depth[j]) * (x - int(xs[j]))
        for k, a, b in mine:
            out[k]["bases"] = at(b) - at(a)
            out[k]["reads"] = int(((p < b) & (e > a)).sum())
    return out


def brute_force(cols, n_targets, windows, mapq_min):
    """the same by a plain double loop over records and windows, nothing shared with expected_cov but the CIGAR operators"""
    out = np.zeros(len(windows), abi.WINDOW_COV)
    n = len(cols["tid"])
    for k, w in enumerate(windows):
        T, a, b = int(w["tid"]), int(w["beg"]), int(w["end"])
        if T < 0 or T >= n_targets or b <= a:
            continue
        bases = reads = 0
        for i in range(n):
            if int(cols["tid"][i]) != T or int(cols["flag"][i]) & NEVER or int(cols["mapq"][i]) < mapq_min:
                continue
            length = 0
            for j in range(int(cols["cigar_off"][i]), int(cols["cigar_off"][i + 1])):
                v = int(cols["cigar"][j])
                if v & 15 in CONSUMES_REF:
                    length += v >> 4
            if length <= 0:
                continue
            p = int(cols["pos"][i])
            ov = min(p + length, b) - max(p, a)
            if ov > 0:
                bases += ov
                reads += 1
        out[k]["bases"], out[k]["reads"] = bases, reads
    return out


# ---- bk_call_windows and the command line's columns ------------------------------------------------------------------------------------
def call_cuts(c, right1, right2):
    return int(c["p1_exact"]) - (1 if right1 else 0), int(c["p2_exact"]) - (1 if right2 else 0)


def call_windows(c, right1, right2, flank, target_len):
    """the five windows of one abi.CLUSTER row: left and right of either cut, then the span between the cuts"""
    assert flank >= 1
    out = np.zeros(5, abi.COV_WINDOW)
    tid = (int(c["p1_tid"]), int(c["p2_tid"]))
    cut = call_cuts(c, right1, right2)

    def put(k, t, a, b):
        out[k]["tid"] = t
        if t < 0:
            return
        a, b = max(a, 0), min(b, int(target_len[t]))
        if b > a:
            out[k]["beg"], out[k]["end"] = a, b
    for s in range(2):
        put(2 * s, tid[s], cut[s] - flank, cut[s])
        put(2 * s + 1, tid[s], cut[s], cut[s] + flank)
    if tid[0] == tid[1] and tid[0] >= 0:
        put(4, tid[0], min(cut), max(cut))
    else:
        put(4, -1, 0, 0)
    return out


def mean_text(w, cov):
    n = int(w["end"]) - int(w["beg"])
    return "." if n <= 0 else "%.2f" % (float(int(cov["bases"])) / float(n))


def ratio_text(windows, cov, cuts):
    """the span's mean over the mean of the two outer flanks: the left window of the lower cut and the right window of the higher one"""
    lo = 0 if cuts[0] <= cuts[1] else 1
    left, right = 2 * lo, 2 * (1 - lo) + 1
    size = lambda k: int(windows[k]["end"]) - int(windows[k]["beg"])
    if size(4) <= 0 or size(left) <= 0 or size(right) <= 0:
        return "."
    mean = lambda k: float(int(cov[k]["bases"])) / float(size(k))
    flanks = mean(left) + mean(right)
    if flanks == 0.0:
        return "."
    return "%.3f" % (mean(4) / (flanks / 2.0))


def call_fields(windows7, cov7, cuts):
    """the eight columns of one call: windows7 = the five of call_windows, then the whole contig of side 1 and of side 2"""
    f = [mean_text(windows7[k], cov7[k]) for k in range(5)]
    f.append(ratio_text(windows7, cov7, cuts))
    return f + [mean_text(windows7[k], cov7[k]) for k in (5, 6)]


def expected_call_fields(c, right1, right2, flank, target_len, cols, mapq_min):
    """(the eight columns, the seven windows) of one call on the record table `cols`"""
    w = np.zeros(7, abi.COV_WINDOW)
    w[:5] = call_windows(c, right1, right2, flank, target_len)
    for s, t in enumerate((int(c["p1_tid"]), int(c["p2_tid"]))):
        w[5 + s]["tid"] = t
        if t >= 0:
            w[5 + s]["end"] = int(target_len[t])
    cov = expected_cov(cols, len(target_len), w, mapq_min)
    return call_fields(w, cov, call_cuts(c, right1, right2)), w

"""Window context (`bk_window_context`, `-context`): the definition of include/breakid_hip.h stated twice, once in vectorised numpy
(boolean masks per class, a masked sum per window) and once as a plain loop over windows and records that shares nothing with it, the
record tables the tests share, and the command line's column formatting.  Nothing here knows of tiles or prefix sums."""
import numpy as np

from breakid_amd import abi
from tests import coveragecases as vc

FIELDS = ["mapq_sum", "reads", "mq0", "lowq", "clipped", "improper", "orphan", "dup", "secsup"]
NAMES = ["Cx_Reads", "Cx_MeanMQ", "Cx_MQ0", "Cx_LowQ", "Cx_Clip", "Cx_Improper", "Cx_Orphan", "Cx_Dup", "Cx_SecSup"]
COLUMNS = [name + str(side) for side in (1, 2) for name in NAMES]
OP_S, OP_H = 4, 5

as_windows = vc.as_windows
make_cols = vc.make_cols


# ---- record tables ----------------------------------------------------------------------------------------------------------------------
FLAGS = [0x0, 0x1 | 0x2, 0x1 | 0x2 | 0x10, 0x1, 0x1 | 0x20, 0x1 | 0x8, 0x1 | 0x8 | 0x2, 0x8, 0x400, 0x1 | 0x400, 0x100, 0x800, 0x800 | 0x400, 0x100 | 0x200, 0x200, 0x200 | 0x400,
         0x4 | 0x1, 0x4 | 0x1 | 0x8, 0x1 | 0x2 | 0x800]
CIGARS = ["{n}M", "{a}S{b}M", "{b}M{a}S", "5H{a}S{b}M", "{b}M{a}S5H", "5H{n}M", "{n}M5H", "{n}S", "", "{a}M{a}S{a}M", "{a}M7D{b}M", "3H", "4H{n}S6H", "{a}S{a}M{a}S"]


def random_table(rng, n, contigs, read_len=100, unmapped=0):
    """n reads spread over the contigs (tid, length): about half are plain proper pairs with mapq 60, the rest draw a flag of FLAGS, a
    CIGAR of CIGARS and a mapq of 0, 1, 19, 20, 21, 60 or 255, so that every class is populated; `unmapped` records with tid -1 behind"""
    a = max(1, read_len // 3)
    texts = [c.format(n=read_len, a=a, b=read_len - a) for c in CIGARS]
    recs = []
    for _ in range(n):
        tid, length = contigs[int(rng.integers(0, len(contigs)))]
        pos = int(rng.integers(0, max(1, length - 2 * read_len)))
        if rng.random() < 0.5:
            recs.append((tid, pos, 0x1 | 0x2, 60, texts[0]))
        else:
            recs.append((tid, pos, FLAGS[int(rng.integers(0, len(FLAGS)))], (0, 1, 19, 20, 21, 60, 255)[int(rng.integers(0, 7))], texts[int(rng.integers(0, len(texts)))]))
    for k in range(unmapped):
        recs.append((-1, -1, 0x4 | 0x1, 0, "%dS" % read_len if k & 1 else ""))
    return make_cols(recs)


# ---- the definition, vectorised ---------------------------------------------------------------------------------------------------------
def record_classes(cols, mapq_min):
    """per record: the nine values it adds to the row of a window it belongs to (an int64 array per field)"""
    flag = cols["flag"].astype(np.int64)
    mapq = cols["mapq"].astype(np.int64)
    off = cols["cigar_off"].astype(np.int64)
    ops = cols["cigar"].astype(np.int64) & 15
    n = len(flag)
    has = lambda bit: (flag & bit) != 0
    mapped = (cols["tid"].astype(np.int64) >= 0) & ~has(0x4)
    base = mapped & ~has(0x100) & ~has(0x200) & ~has(0x400) & ~has(0x800)
    # the first and the last operation once one leading and one trailing H are gone
    lo, hi = off[:-1].copy(), off[1:].copy()
    pad = np.concatenate([ops, [-1]])  # (an index of an empty CIGAR may be len(ops))
    lead_h = (hi > lo) & (pad[np.minimum(lo, len(ops))] == OP_H)
    lo = lo + lead_h
    trail_h = (hi > lo) & (pad[np.maximum(hi - 1, 0)] == OP_H)
    hi = hi - trail_h
    some = hi > lo
    first = np.where(some, pad[np.minimum(lo, len(ops))], -1)
    last = np.where(some, pad[np.maximum(hi - 1, 0)], -1)
    clipped = some & ((first == OP_S) | (last == OP_S))
    assert len(clipped) == n
    return {"reads": base.astype(np.int64), "mapq_sum": np.where(base, mapq, 0), "mq0": (base & (mapq == 0)).astype(np.int64), "lowq": (base & (mapq < mapq_min)).astype(np.int64),
            "clipped": (base & clipped).astype(np.int64), "improper": (base & has(0x1) & ~has(0x8) & ~has(0x2)).astype(np.int64), "orphan": (base & has(0x1) & has(0x8)).astype(np.int64),
            "dup": (mapped & has(0x400) & ~has(0x100) & ~has(0x200) & ~has(0x800)).astype(np.int64), "secsup": (mapped & (has(0x100) | has(0x800))).astype(np.int64)}


def expected_ctx(cols, n_targets, windows, mapq_min):
    """one abi.WINDOW_CTX row per window: the records with tid == T and beg <= pos < end, by masking"""
    windows = np.ascontiguousarray(windows, abi.COV_WINDOW)
    out = np.zeros(len(windows), abi.WINDOW_CTX)
    cls = record_classes(cols, mapq_min)
    tid = cols["tid"].astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    for k, w in enumerate(windows):
        T, a, b = int(w["tid"]), int(w["beg"]), int(w["end"])
        if T < 0 or T >= n_targets or b <= a:
            continue
        m = (tid == T) & (pos >= a) & (pos < b)
        for f in FIELDS:
            out[k][f] = int(cls[f][m].sum())
    return out


def class_totals(cols, mapq_min):
    """the nine sums over every record with tid >= 0"""
    cls = record_classes(cols, mapq_min)
    return {f: int(cls[f][cols["tid"] >= 0].sum()) for f in FIELDS}


# ---- the definition once more, a plain loop ---------------------------------------------------------------------------------------------
def is_clipped(ops):
    """ops: the operation letters of one CIGAR"""
    if ops and ops[0] == "H":
        ops = ops[1:]
    if ops and ops[-1] == "H":
        ops = ops[:-1]
    return bool(ops) and (ops[0] == "S" or ops[-1] == "S")


def expected_ctx_slow(cols, n_targets, windows, mapq_min):
    out = np.zeros(len(windows), abi.WINDOW_CTX)
    for k, w in enumerate(windows):
        T, a, b = int(w["tid"]), int(w["beg"]), int(w["end"])
        if T < 0 or T >= n_targets or b <= a:
            continue
        row = dict.fromkeys(FIELDS, 0)
        for i in range(len(cols["tid"])):
            if int(cols["tid"][i]) != T or not a <= int(cols["pos"][i]) < b:
                continue
            flag, mapq = int(cols["flag"][i]), int(cols["mapq"][i])
            if flag & 0x4:
                continue
            if flag & 0x100 or flag & 0x800:
                row["secsup"] += 1
                continue
            if flag & 0x200:
                continue
            if flag & 0x400:
                row["dup"] += 1
                continue
            ops = "".join(vc.OPS[int(v) & 15] for v in cols["cigar"][int(cols["cigar_off"][i]):int(cols["cigar_off"][i + 1])])
            row["reads"] += 1
            row["mapq_sum"] += mapq
            row["mq0"] += mapq == 0
            row["lowq"] += mapq < mapq_min
            row["clipped"] += is_clipped(ops)
            if flag & 0x1:
                if flag & 0x8:
                    row["orphan"] += 1
                elif not flag & 0x2:
                    row["improper"] += 1
        for f in FIELDS:
            out[k][f] = row[f]
    return out


# ---- the command line's columns ---------------------------------------------------------------------------------------------------------
def add_rows(a, b):
    out = np.zeros(1, abi.WINDOW_CTX)[0]
    for f in FIELDS:
        out[f] = int(a[f]) + int(b[f])
    return out


def side_columns(row):
    """the nine columns of one side from its row; every ratio is a quotient of two doubles"""
    reads = int(row["reads"])
    ratio = lambda f, fmt: "." if reads == 0 else fmt % (float(int(row[f])) / float(reads))
    return [str(reads), ratio("mapq_sum", "%.1f"), ratio("mq0", "%.3f"), ratio("lowq", "%.3f"), ratio("clipped", "%.3f"), ratio("improper", "%.3f"), str(int(row["orphan"])),
            str(int(row["dup"])), str(int(row["secsup"]))]


def expected_columns(row_pair):
    """the eighteen columns of one call from the rows of its two sides"""
    return side_columns(row_pair[0]) + side_columns(row_pair[1])


def expected_call_rows(c, right1, right2, flank, target_len, cols, mapq_min):
    """(the rows of the two sides, the four flank windows) of one call on the record table `cols`: side s is rows 2 s and 2 s + 1 added"""
    w = vc.call_windows(c, right1, right2, flank, target_len)[:4]
    r = expected_ctx(cols, len(target_len), w, mapq_min)
    return (add_rows(r[0], r[1]), add_rows(r[2], r[3])), w

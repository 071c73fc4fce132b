"""Measurement: what `bk_junction_fit` costs at the bench shape.

The bench shape (configs[1], `-fast`; profiles/r14_unique_620M.json) has 126 618 voted calls, so 253 236 sides.  Every side gets a
probe: side 2c and side 2c + 1 are each other's mate, a LEFT side has a query of 40 bases and a RIGHT side one of 60, as the
designed split reads clip them.  The reference is synthetic: random bases on 24 contigs, of which only the windows
[pos - R, pos + R], R = 64 + 32 + 33, around every probe position are packed, merged where they touch (the sites come in pairs 200
bases apart, so two windows merge into one segment), as the command line reads them from the nib files.  A query is the mate
walk itself with a twentieth of its bases substituted; every tenth query starts with five inserted bases and goes on from M[3].
After a warm-up call the fit runs `--reps` times at the command line's defaults (32 / 32 / 32); each repetition gives the
HIP-event time of the call's scope (`junction_fit`: the one kernel; the upload of the table is outside it), the wall time of
the whole call with the upload, and the bytes of the library's model (bk_timing_touched).

    python tools/gpu_homology_bench.py [--calls 126618] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8e12  # bytes per second: the rate DESIGN.md measures every stage against
MAX_LEN, MAX_SHIFT, MAX_INS, MAX_HOM = 64, 32, 32, 32
RADIUS = MAX_LEN + MAX_SHIFT + 33
NIB_OF = (2, 1, 3, 0)  # A C G T -> nib code


def make_table(calls, seed):
    """(ref, probes, query): the packed windows, the 2 x calls probes and their queries"""
    import numpy as np
    from breakid_amd import abi

    rng = np.random.default_rng(seed)
    n = 2 * calls
    k = np.arange(n)
    tid, slot = k % 24, k // 24
    pos = 10_000 + (slot // 2) * 1_200 + (slot & 1) * 200
    length = (int(pos.max()) + RADIUS + 1_000) & ~1  # of every contig (even: two bases to a byte)
    genome = rng.integers(0, 4, (24, length), dtype=np.int8)  # A C G T = 0 .. 3; position p (1-based) is genome[tid, p - 1]
    probes = np.zeros(n, abi.JUNCTION_PROBE)
    probes["tid_own"], probes["pos_own"], probes["dir_own"] = tid, pos, k & 1
    probes["tid_mate"], probes["pos_mate"], probes["dir_mate"] = tid[k ^ 1], pos[k ^ 1], (k ^ 1) & 1
    probes["qlen"] = np.where(k & 1, 60, 40)
    # queries: the mate walk (never complemented here: the two sides of a call have unlike directions)
    with_ins = k % 10 == 0
    i = np.arange(MAX_LEN)[None, :] + np.where(with_ins, 3 - 5, 0)[:, None]
    step = np.where(probes["dir_mate"] == 1, 1, -1)[:, None]
    codes = genome[probes["tid_mate"][:, None], probes["pos_mate"].astype(np.int64)[:, None] + step * i - 1]
    off = rng.random((n, MAX_LEN)) < 0.05
    codes = np.where(off, rng.integers(0, 4, (n, MAX_LEN)), codes)
    inserted = with_ins[:, None] & (np.arange(MAX_LEN)[None, :] < 5)  # ... each unlike the base its diagonal has there
    codes = np.where(inserted, (genome[probes["tid_mate"][:, None], probes["pos_mate"].astype(np.int64)[:, None] + step * i - 1] + rng.integers(1, 4, (n, MAX_LEN))) % 4, codes)
    query = np.frombuffer(b"ACGT", np.uint8)[codes]
    query[np.arange(MAX_LEN)[None, :] >= probes["qlen"][:, None]] = 0
    # the windows, merged per contig (the sites of a contig ascend)
    packed = np.asarray(NIB_OF, np.uint8)[genome]
    packed = (packed[:, 0::2] << 4) | packed[:, 1::2]
    segs, parts = [], []
    for t in range(24):
        p = pos[tid == t]
        a, b = np.maximum(1, p - RADIUS), np.minimum(length, p + RADIUS)
        new = np.concatenate([[True], a[1:] > b[:-1] + 1])
        first, last = a[new], np.maximum.reduceat(b, np.flatnonzero(new))
        start0 = (first - 1) & ~1  # a segment starts on a byte
        for s, e in zip(start0, last):
            segs.append((t, s, e - s))
            parts.append(packed[t, s // 2:(e + 1) // 2])
    ref = {"tid": np.asarray([s[0] for s in segs], np.int32), "start": np.asarray([s[1] for s in segs], np.uint32), "len": np.asarray([s[2] for s in segs], np.uint32),
           "off": np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64), "bases": np.concatenate(parts)}
    return ref, probes, np.ascontiguousarray(query)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=126_618)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    from breakid_amd import capi

    ref, probes, query = make_table(args.calls, args.seed)
    n = len(probes)
    t = capi.Context([("chr%d" % (i + 1), 250_000_000) for i in range(24)], device=0)
    call = lambda: t.junction_fit(ref, probes, query, MAX_SHIFT, MAX_INS, MAX_HOM)  # noqa: E731
    rows = call()  # warm-up: the call's buffers are allocated here
    plain = np.arange(n) % 10 != 0
    # the fit finds what the queries were cut with (a substituted column 0 reads as one inserted base on the same diagonal)
    assert (rows["placed"] == 1).all() and (rows["shift"][plain] == rows["ins"][plain]).mean() > 0.99 and (rows["mism"] * 4 < rows["aligned"]).mean() > 0.99
    assert (rows["ins"][~plain] >= 5).mean() > 0.99 and (rows["shift"][~plain] - rows["ins"][~plain].astype(np.int64) == -2).mean() > 0.99
    ev, wall, by, tb = [], [], 0, 0
    t.timing_enable(True)
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, by, tb = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == "junction_fit"][-1]
        ev.append(ms)
    t.timing_enable(False)
    med = float(np.median(ev))
    q = probes["qlen"].astype(np.int64)
    imax = np.minimum(MAX_INS, q - 1)
    columns = int(((2 * MAX_SHIFT + 1) * ((imax + 1) * q - imax * (imax + 1) // 2)).sum())  # sum over the placements of qlen - ins
    out = {
        "what": "bk_junction_fit of one probe per side of the calls of configs[1] after one -fast step, against a synthetic reference of merged windows",
        "calls": args.calls, "probes": n, "query_lengths": [40, 60], "max_len": MAX_LEN, "max_shift": MAX_SHIFT, "max_ins": MAX_INS, "max_hom": MAX_HOM, "reps": args.reps,
        "segments": int(len(ref["tid"])), "reference_bytes": int(ref["bases"].nbytes), "placements_per_probe": (2 * MAX_SHIFT + 1) * (MAX_INS + 1),
        "placement_columns": columns, "event_ms": [round(x, 4) for x in ev], "event_ms_median": round(med, 4), "event_ms_min": round(min(ev), 4),
        "event_ms_max": round(max(ev), 4), "wall_ms_with_upload": [round(x, 2) for x in wall], "bytes": int(by), "model_bytes": int(tb),
        "model_gbps": round(tb / med / 1e6, 1), "frac_of_hbm_peak": round(tb / (med * 1e-3) / HBM_PEAK, 4), "placement_columns_per_s": round(columns / (med * 1e-3), 0),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

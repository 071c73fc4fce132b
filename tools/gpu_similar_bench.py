"""Measurement: what `bk_locus_similarity` costs at the bench shape.

The bench shape (configs[1], `-fast`; profiles/r14_unique_620M.json) has 126 618 voted calls, and every call gives one pair, as
the command line submits them.  The two positions of a call lie on different contigs.  The reference is synthetic: random bases
on 24 contigs, of which only the windows [pos - R, pos + R] around every position are packed, as the command line reads them from
the nib files.  Every tenth call has an 80-base stretch of its first locus copied into the second with three substitutions, every
twentieth reverse-complemented, so that the search has something to find; the others are background.  After a warm-up call the
search runs `--reps` times at each flank (150, the command line's default, and 255, the largest); each repetition gives the
HIP-event time of the call's scope (`locus_similarity`: the one kernel; the upload of the table is outside it), the wall time of
the whole call with the upload, and the bytes of the library's model (bk_timing_touched).

    python tools/gpu_similar_bench.py [--calls 126618] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLANKS = (150, 255)
NIB_OF = (2, 1, 3, 0)  # A C G T -> nib code
SPACING = 600          # between the positions of one contig: the windows of the largest flank stay apart
COPY = 80


def make_table(calls, flank, seed):
    """(ref, pairs): the packed windows and one pair per call"""
    import numpy as np
    from breakid_amd import abi

    rng = np.random.default_rng(seed)
    c = np.arange(calls)
    tid1, tid2 = c % 12, 12 + c % 12
    pos = 10_000 + (c // 12) * SPACING
    length = (int(pos.max()) + 2_000) & ~1  # of every contig (even: two bases to a byte)
    genome = rng.integers(0, 4, (24, length), dtype=np.int8)  # A C G T = 0 .. 3; position p (1-based) is genome[tid, p - 1]
    for k in np.flatnonzero(c % 10 == 0):
        src = genome[tid1[k], pos[k] - 40 - 1:pos[k] - 40 - 1 + COPY].copy()
        if k % 20 == 0:
            src = (3 - src)[::-1]
        src[[20, 40, 60]] = (src[[20, 40, 60]] + 1) % 4
        genome[tid2[k], pos[k] - 25 - 1:pos[k] - 25 - 1 + COPY] = src
    pairs = np.zeros(calls, abi.LOCUS_PAIR)
    pairs["tid_a"], pairs["pos_a"], pairs["tid_b"], pairs["pos_b"] = tid1, pos, tid2, pos
    packed = np.asarray(NIB_OF, np.uint8)[genome]
    packed = (packed[:, 0::2] << 4) | packed[:, 1::2]
    segs, parts = [], []
    for t in range(24):
        p = np.unique(pos[(tid1 if t < 12 else tid2) == t])
        start0 = (p - flank - 1) & ~1  # a segment starts on a byte
        for s, e in zip(start0, p + flank):
            segs.append((t, s, e - s))
            parts.append(packed[t, s // 2:(e + 1) // 2])
    ref = {"tid": np.asarray([s[0] for s in segs], np.int32), "start": np.asarray([s[1] for s in segs], np.uint32), "len": np.asarray([s[2] for s in segs], np.uint32),
           "off": np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64), "bases": np.concatenate(parts)}
    return ref, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=126_618)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    from breakid_amd import capi

    t = capi.Context([("chr%d" % (i + 1), 250_000_000) for i in range(24)], device=0)
    out = {"what": "bk_locus_similarity of one pair per call of configs[1] after one -fast step, against a synthetic reference of windows",
           "calls": args.calls, "pairs": args.calls, "reps": args.reps, "flanks": {}}
    for flank in FLANKS:
        ref, pairs = make_table(args.calls, flank, args.seed)
        n, L = len(pairs), 2 * flank + 1
        call = lambda: t.locus_similarity(ref, pairs, flank)  # noqa: E731
        rows = call()  # warm-up: the call's buffers are allocated here
        with_copy = np.arange(args.calls) % 10 == 0
        # the search finds what was planted, and nothing like it elsewhere
        assert (rows["found"] == 1).all() and (rows["score"][with_copy] >= COPY - 9).all() and (rows["len"][with_copy] >= COPY).all()
        assert (rows["score"][~with_copy] < 30).all() and (rows["orient"][np.arange(args.calls) % 20 == 0] == 1).all()
        ev, wall, by, tb = [], [], 0, 0
        t.timing_enable(True)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, by, tb = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == "locus_similarity"][-1]
            ev.append(ms)
        t.timing_enable(False)
        med = float(np.median(ev))
        cells = 2 * L * L * n  # every cell of both orientations (the excluded diagonal never applies: the contigs differ)
        out["flanks"][str(flank)] = {
            "window": L, "segments": int(len(ref["tid"])), "reference_bytes": int(ref["bases"].nbytes), "diagonals_per_pair": 2 * (2 * L - 1), "cells": cells,
            "background_score_median": float(np.median(rows["score"][~with_copy])), "background_run_median": float(np.median(rows["run"][~with_copy])),
            "event_ms": [round(x, 4) for x in ev], "event_ms_median": round(med, 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
            "wall_ms_with_upload": [round(x, 2) for x in wall], "bytes": int(by), "model_bytes": int(tb), "cells_per_s": round(cells / (med * 1e-3), 0),
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

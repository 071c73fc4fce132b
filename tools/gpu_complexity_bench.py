"""Measurement: what `bk_site_complexity` costs at the bench shape.

The bench shape (configs[1], `-fast`; profiles/r14_unique_620M.json) has 126 618 voted calls, and every call gives two sites, as
the command line submits them: 253 236 sites.  The reference is synthetic: random bases on 24 contigs, of which only the windows
[pos - R, pos + R] around every site are packed, as the command line reads them from the nib files.  Every tenth site lies in a
planted (CA)20, every seventh in a soft-masked interval of 200 bases, so that the tract walk and the mask walk have something to
find; the others are background.  After a warm-up call the description runs `--reps` times at each flank (32, the command line's
default, and 255, the largest) with the default max_period of 6; each repetition gives the HIP-event time of the call's scope
(`site_complexity`: the one kernel; the upload of the table is outside it), the wall time of the whole call with the upload, and
the bytes of the library's model (bk_timing_touched: n * (72 + L)).

    python tools/gpu_complexity_bench.py [--calls 126618] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLANKS = (32, 255)
MAX_PERIOD = 6
NIB_OF = (2, 1, 3, 0)  # A C G T -> nib code
SPACING = 600          # between the sites of one contig: the windows of the largest flank stay apart
TRACT = 40             # (CA)20
MASKED = 200
HBM_BYTES_PER_S = 8e12  # the datasheet rate the fraction is quoted against


def make_table(n_sites, flank, seed):
    """(ref, sites): the packed windows and the sites"""
    import numpy as np
    from breakid_amd import abi

    rng = np.random.default_rng(seed)
    c = np.arange(n_sites)
    tid = c % 24
    pos = 10_000 + (c // 24) * SPACING
    length = (int(pos.max()) + 2_000) & ~1  # of every contig (even: two bases to a byte)
    nib = np.asarray(NIB_OF, np.uint8)[rng.integers(0, 4, (24, length), dtype=np.int8)]  # position p (1-based) is nib[tid, p - 1]
    ca = np.asarray(NIB_OF, np.uint8)[np.asarray([1, 0] * (TRACT // 2))]
    for k in np.flatnonzero(c % 10 == 0):
        at = pos[k] - 1 - TRACT // 2
        nib[tid[k], at:at + TRACT] = ca
        nib[tid[k], at - 1] = nib[tid[k], at + TRACT] = NIB_OF[2]  # G on either side: the tract is 40 columns and no more
    for k in np.flatnonzero(c % 7 == 0):
        nib[tid[k], pos[k] - 1 - MASKED // 2:pos[k] - 1 + MASKED // 2] |= 8
    sites = np.zeros(n_sites, abi.REF_SITE)
    sites["tid"], sites["pos"] = tid, pos
    packed = (nib[:, 0::2] << 4) | nib[:, 1::2]
    segs, parts = [], []
    for t in range(24):
        p = pos[tid == t]
        start0 = (p - flank - 1) & ~1  # a segment starts on a byte
        for s, e in zip(start0, p + flank):
            segs.append((t, s, e - s))
            parts.append(packed[t, s // 2:(e + 1) // 2])
    ref = {"tid": np.asarray([s[0] for s in segs], np.int32), "start": np.asarray([s[1] for s in segs], np.uint32), "len": np.asarray([s[2] for s in segs], np.uint32),
           "off": np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64), "bases": np.concatenate(parts)}
    return ref, sites


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
    n = 2 * args.calls
    out = {"what": "bk_site_complexity of two sites per call of configs[1] after one -fast step, against a synthetic reference of windows",
           "calls": args.calls, "sites": n, "max_period": MAX_PERIOD, "reps": args.reps, "hbm_bytes_per_s": HBM_BYTES_PER_S, "flanks": {}}
    for flank in FLANKS:
        ref, sites = make_table(n, flank, args.seed)
        L = 2 * flank + 1
        call = lambda: t.site_complexity(ref, sites, flank, MAX_PERIOD)  # noqa: E731
        rows = call()  # warm-up: the call's buffers are allocated here
        planted, masked = np.arange(n) % 10 == 0, np.arange(n) % 7 == 0
        # the description finds what was planted, and nothing like it elsewhere
        assert (rows["covered"] == L).all() and (rows["valid"] == L).all()
        assert (rows["bp_len"][planted] == TRACT).all() and (rows["bp_period"][planted] == 2).all() and (rows["max_len"][~planted] < 30).all()
        assert (rows["mask_run"][masked] == min(L, MASKED)).all() and (rows["mask_run"][~masked] == 0).all()
        ev, wall, by, tb = [], [], 0, 0
        t.timing_enable(True)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, by, tb = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == "site_complexity"][-1]
            ev.append(ms)
        t.timing_enable(False)
        med = float(np.median(ev))
        assert int(tb) == n * (72 + L)
        bg = ~planted
        out["flanks"][str(flank)] = {
            "window": L, "segments": int(len(ref["tid"])), "reference_bytes": int(ref["bases"].nbytes),
            "background_dust_mean": round(float(np.mean(rows["tri_pairs"][bg] / (rows["tri_total"][bg] - 1.0))), 3),
            "background_max_len_mean": round(float(np.mean(rows["max_len"][bg])), 2), "background_max_len_highest": int(rows["max_len"][bg].max()),
            "event_ms": [round(x, 4) for x in ev], "event_ms_median": round(med, 4), "event_ms_min": round(min(ev), 4), "event_ms_max": round(max(ev), 4),
            "wall_ms_with_upload": [round(x, 2) for x in wall], "bytes": int(by), "model_bytes": int(tb),
            "fraction_of_hbm_rate": round(int(tb) / (med * 1e-3) / HBM_BYTES_PER_S, 6), "sites_per_s": round(n / (med * 1e-3), 0),
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""Measurement: what `bk_known_calls` costs at the bench shape.

The call reads no records, so the sites are drawn directly: one per voted call of the bench shape (126 618), on 24 contigs of 60 to
250 Mb.  The panel is drawn too: `--entries` (200 000) pairs of intervals, the size of a panel of normals of some dozens of samples,
under `--names` (40) names, so that names are shared; four fifths carry a score, half state both strands.  `--placed` of the entries
(0.10) are laid over a site, each interval 1 to 500 bases wide and up to 150 bases off, so that hits and near misses occur; `--crossed`
of those (0.30) are written the other way round; a fifth of them are laid over one of 2000 sites, so that a site has several hits.
`--wide` (8) entries have one interval of 10 Mb: every site behind such an interval's start on its contig walks back to it.  Everything
else is drawn uniformly with intervals of 1 to 500 bases and meets a site only by chance.

After a warm-up call the sites are answered `--reps` times; each repetition gives the HIP-event times of the scopes `known_calls`,
`known_calls_index` (keys, sort, ends, running maximum) and `known_calls_sites` (the walk, the scan with the host's read of the total,
the listing, the sort of the names, the run heads) and the wall clock around the call from Python (that plus the host's check, the two
uploads and the copy back).  The scopes are reported as fractions of 8 TB/s by the library's own byte model (bk_timing_touched).  A
second panel without placed and wide entries (`control`) shows what the index and the launches cost without hits.  Nothing is compared
against a target: the tool only records.

    python tools/gpu_known_bench.py [--sites 126618] [--entries 200000] [--slop 100] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
SCOPES = ("known_calls", "known_calls_index", "known_calls_sites")


def draw_sites(np, abi, n, lens, seed):
    rng = np.random.default_rng(seed)
    s = np.zeros(n, abi.KNOWN_SITE)
    for side in ("1", "2"):
        s["tid" + side] = rng.integers(0, len(lens), n)
        s["pos" + side] = (rng.random(n) * (lens[s["tid" + side]] - 2000)).astype(np.int64) + 1000
        s["right" + side] = rng.integers(0, 2, n)
    return s


def draw_panel(np, abi, sites, lens, n, names, placed, crossed, wide, seed):
    rng = np.random.default_rng(seed)
    e = np.zeros(n, abi.KNOWN_ENTRY)
    for side in ("1", "2"):
        e["tid" + side] = rng.integers(0, len(lens), n)
        e["beg" + side] = (rng.random(n) * (lens[e["tid" + side]] - 2000)).astype(np.int64) + 1000
        e["end" + side] = e["beg" + side] + rng.integers(1, 501, n)
    e["name"] = rng.integers(0, names, n)
    e["score"] = np.where(rng.random(n) < 0.8, rng.integers(0, 100, n), abi.KNOWN_NO_SCORE)
    stated = rng.random(n) < 0.5
    e["strand1"] = np.where(stated, rng.integers(1, 3, n), 0)
    e["strand2"] = np.where(stated, rng.integers(1, 3, n), 0)
    n_placed, n_crossed = int(n * placed), int(n * placed * crossed)
    rows = rng.permutation(n)[:n_placed + wide]
    at = rng.integers(0, len(sites), n_placed) if len(sites) else np.zeros(0, np.int64)
    if len(sites):
        at[:n_placed // 5] = rng.integers(0, min(2000, len(sites)), n_placed // 5)
    for k, (row, site) in enumerate(zip(rows[:n_placed], at)):
        iv = []
        for side in ("1", "2"):
            x = int(sites[site]["pos" + side]) - 1
            b = max(0, x - int(rng.integers(0, 500)) + int(rng.integers(-150, 151)))
            iv.append((int(sites[site]["tid" + side]), b, b + int(rng.integers(1, 501)), int(sites[site]["right" + side]) + 1))
        if k < n_crossed:
            iv.reverse()
        (e[row]["tid1"], e[row]["beg1"], e[row]["end1"], s1), (e[row]["tid2"], e[row]["beg2"], e[row]["end2"], s2) = iv
        if e[row]["strand1"]:
            e[row]["strand1"], e[row]["strand2"] = s1, s2 if rng.random() < 0.8 else 3 - s2
    for row in rows[n_placed:]:
        e[row]["beg1"] = int(rng.integers(1000, 40_000_000))
        e[row]["end1"] = int(e[row]["beg1"]) + 10_000_000
    return e, {"entries": n, "names": names, "placed_on_sites": n_placed, "of_them_crossed": n_crossed, "wide_10mb": wide}


def measure(np, torch, t, entries, sites, slop, reps):
    rows = t.known_calls(entries, sites, slop)  # warm-up: the call's buffers are allocated here
    wall, event, touched = [], {s: [] for s in SCOPES}, {}
    t.timing_enable(True)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = t.known_calls(entries, sites, slop)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched()) if name in SCOPES}  # (the scopes accumulate: the last ones)
        for s in SCOPES:
            event[s].append(seen[s][0])
            touched[s] = int(seen[s][1])
    t.timing_enable(False)
    out = {"wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3)}
    for s in SCOPES:
        med = float(np.median(event[s]))
        out[s] = {"event_ms": [round(x, 4) for x in event[s]], "event_ms_median": round(med, 4), "event_ms_min": round(min(event[s]), 4), "event_ms_max": round(max(event[s]), 4),
                  "model_bytes": touched[s], "fraction_of_8_tb_per_s": round(touched[s] / (med * 1e-3) / HBM_BYTES_PER_S, 6) if med > 0 else None}
    med = out["known_calls"]["event_ms_median"]
    out.update({"sites_per_s": round(len(sites) / (med * 1e-3), 0) if med > 0 else None,
                "hits": int(rows["n_hits"].sum()), "sites_with_a_hit": int((rows["n_hits"] > 0).sum()), "most_hits_at_one_site": int(rows["n_hits"].max()) if len(rows) else 0,
                "crossed_best_hits": int(rows["best_crossed"].sum()), "oriented_hits": int(rows["n_oriented"].sum()), "opposed_hits": int(rows["n_opposed"].sum()),
                "sites_with_shared_names": int((rows["n_names"] < rows["n_hits"]).sum()), "entries_met_by_side": [int(rows["n_side"][:, 0].sum()), int(rows["n_side"][:, 1].sum())]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=126_618)
    ap.add_argument("--entries", type=int, default=200_000)
    ap.add_argument("--names", type=int, default=40)
    ap.add_argument("--placed", type=float, default=0.10)
    ap.add_argument("--crossed", type=float, default=0.30)
    ap.add_argument("--wide", type=int, default=8)
    ap.add_argument("--slop", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi

    lens = np.random.default_rng(args.seed).integers(60_000_000, 250_000_000, 24)
    sites = draw_sites(np, abi, args.sites, lens, args.seed + 1)
    panel, drawn = draw_panel(np, abi, sites, lens, args.entries, args.names, args.placed, args.crossed, args.wide, args.seed + 2)
    control, _ = draw_panel(np, abi, sites, lens, args.entries, args.names, 0.0, 0.0, 0, args.seed + 3)
    t = capi.Context([("c%d" % i, 250_000_000) for i in range(24)], device=0)
    out = {"what": "bk_known_calls of one drawn site per voted call of the bench shape against a drawn panel; `control`: as large a panel without placed and wide entries",
           "sites": int(len(sites)), "slop": args.slop, "reps": args.reps, "drawn": drawn}
    out.update(measure(np, torch, t, panel, sites, args.slop, args.reps))
    out["control"] = measure(np, torch, t, control, sites, args.slop, args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""Measurement: what `bk_link_calls` costs at the bench shape.

The call reads no records, so the sites are drawn directly: one per voted call of the bench shape (126 618), on 24 contigs of 60 to
250 Mb.  `--recip` of the sites (0.10) are the reciprocal junction of another site: both directions flipped, both breakpoints moved by up
to 300 bases.  `--dup` (0.02) are a second call of another site within 5 bases.  `--hot` loci (4) hold `--hot-calls` (250) calls each
inside one window, so that the k * k cost of a crowded locus is in the number.  Everything else is drawn uniformly and meets another
breakend only by chance.  After a warm-up call the sites are answered `--reps` times; each repetition gives the HIP-event time of the
scope `link_calls` (keys, sort, runs, the site kernel, the component rounds with the host's reads of the changed flag, the events) and
the wall clock around the call from Python (that plus the host's check, the upload and the copy back).  The scope is reported as a
fraction of 8 TB/s by the library's own byte model (bk_timing_touched), the hits (breakends of other sites inside a window) are counted
from the sorted table on the host, and one more call with BK_DEBUG=link gives the number of component rounds.  A second list with the
same number of sites and no partner at all (`control`) shows what the sort and the launches cost without hits and with one round.

    python tools/gpu_link_bench.py [--sites 126618] [--dist 1000] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def draw_sites(np, abi, n, recip, dup, hot, hot_calls, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(60_000_000, 250_000_000, 24)
    s = np.zeros(n, abi.LINK_SITE)
    for side in ("1", "2"):
        s["tid" + side] = rng.integers(0, 24, n)
        s["pos" + side] = (rng.random(n) * (lens[s["tid" + side]] - 2000)).astype(np.int64) + 1000
        s["right" + side] = rng.integers(0, 2, n)
    order = rng.permutation(n)
    n_recip, n_dup, n_hot = int(n * recip / 2), int(n * dup / 2), hot * hot_calls
    src, dst = order[:n_recip], order[n_recip:2 * n_recip]
    for side in ("1", "2"):
        s["tid" + side][dst] = s["tid" + side][src]
        s["pos" + side][dst] = s["pos" + side][src] + rng.integers(-300, 301, n_recip)
        s["right" + side][dst] = 1 - s["right" + side][src]
    src, dst = order[2 * n_recip:2 * n_recip + n_dup], order[2 * n_recip + n_dup:2 * n_recip + 2 * n_dup]
    for side in ("1", "2"):
        s["tid" + side][dst] = s["tid" + side][src]
        s["pos" + side][dst] = s["pos" + side][src] + rng.integers(-5, 6, n_dup)
        s["right" + side][dst] = s["right" + side][src]
    hot_rows = order[2 * n_recip + 2 * n_dup:2 * n_recip + 2 * n_dup + n_hot]
    for h in range(hot):
        rows = hot_rows[h * hot_calls:(h + 1) * hot_calls]
        s["tid1"][rows] = h
        s["pos1"][rows] = 30_000_000 + rng.integers(0, 800, len(rows))  # side 2 stays where it was drawn: a locus with many partners
    return s, {"reciprocal_pairs_drawn": n_recip, "duplicate_pairs_drawn": n_dup, "hot_loci": hot, "hot_calls": hot_calls}


def count_hits(np, sites, D):
    """breakends of other sites inside the window of a side, over all sides: what the site kernel's lanes look at"""
    tid = np.concatenate([sites["tid1"], sites["tid2"]]).astype(np.int64)
    pos = np.concatenate([sites["pos1"], sites["pos2"]]).astype(np.int64)
    key = np.sort(((tid + 1) << 32) | pos)
    lo = np.searchsorted(key, ((tid + 1) << 32) | np.maximum(pos - D, 0), "left")
    hi = np.searchsorted(key, ((tid + 1) << 32) | np.minimum(pos + D, 0xFFFFFFFF), "right")
    return int((hi - lo).sum() - len(key)), int((hi - lo).max() - 1)  # (every breakend finds itself)


def rounds_of(t, sites, D):
    """one call with BK_DEBUG=link and file descriptor 2 in a file: the library says how many rounds the components took"""
    old = os.environ.get("BK_DEBUG")
    os.environ["BK_DEBUG"] = "link"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            t.link_calls(sites, D)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            if old is None:
                del os.environ["BK_DEBUG"]
            else:
                os.environ["BK_DEBUG"] = old
        f.seek(0)
        m = re.search(rb"(\d+) rounds", f.read())
    return int(m.group(1)) if m else None


def measure(np, torch, t, sites, D, reps):
    rows = t.link_calls(sites, D)  # warm-up: the call's buffers are allocated here
    wall, event, touched = [], [], 0
    t.timing_enable(True)
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = t.link_calls(sites, D)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched()) if name == "link_calls"}  # (the scopes accumulate: the last one)
        event.append(seen["link_calls"][0])
        touched = int(seen["link_calls"][1])
    t.timing_enable(False)
    med = float(np.median(event))
    hits, widest = count_hits(np, sites, D)
    return rows, {
        "event_ms": [round(x, 4) for x in event], "event_ms_median": round(med, 4), "event_ms_min": round(min(event), 4), "event_ms_max": round(max(event), 4),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": touched, "tb_per_s": round(touched / (med * 1e-3) / 1e12, 5) if med > 0 else None,
        "fraction_of_8_tb_per_s": round(touched / (med * 1e-3) / HBM_BYTES_PER_S, 6) if med > 0 else None,
        "sites_per_s": round(len(sites) / (med * 1e-3), 0) if med > 0 else None,
        "hits": hits, "hits_widest_window": widest, "rounds": rounds_of(t, sites, D),
        "related_pairs": {k: int(rows[f].sum()) // 2 for k, f in (("duplicate", "n_dup"), ("reciprocal", "n_recip"), ("adjacent", "n_adj"))},
        "with_mate": int((rows["mate"] >= 0).sum()), "events_of_more_than_one": int(((rows["event"] == np.arange(len(rows))) & (rows["event_size"] > 1)).sum()),
        "largest_event": int(rows["event_size"].max()) if len(rows) else 0,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=126_618)
    ap.add_argument("--dist", type=int, default=1000)
    ap.add_argument("--recip", type=float, default=0.10)
    ap.add_argument("--dup", type=float, default=0.02)
    ap.add_argument("--hot", type=int, default=4)
    ap.add_argument("--hot-calls", type=int, default=250)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi

    sites, drawn = draw_sites(np, abi, args.sites, args.recip, args.dup, args.hot, args.hot_calls, args.seed)
    control, _ = draw_sites(np, abi, args.sites, 0.0, 0.0, 0, 0, args.seed + 1)
    t = capi.Context([("c%d" % i, 250_000_000) for i in range(24)], device=0)
    _, designed = measure(np, torch, t, sites, args.dist, args.reps)
    _, plain = measure(np, torch, t, control, args.dist, args.reps)
    out = {"what": "bk_link_calls of one drawn site per voted call of the bench shape; `control`: as many sites without designed partners",
           "sites": int(len(sites)), "max_dist": args.dist, "reps": args.reps, "drawn": drawn}
    out.update(designed)
    out["control"] = plain
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

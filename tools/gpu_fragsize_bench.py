"""Measurement: what `bk_fragment_sizes` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it) and one hot-path step run
on it.  Every voted call gets a site at its voted positions with the sides of bk_junction_sides, every other cluster row is skipped, and
the bounds are bk_fragment_bounds of the run's own insert sizes: what the command line's `-fragsize -all` asks.  After a warm-up call the
sites are answered `--reps` times; each repetition gives the HIP-event time of the scope `fragment_sizes` and the wall clock around the
call from Python (that plus the host's check, the upload and the copy back).  The scope is reported as a fraction of 8 TB/s by the
library's own byte model (bk_timing_touched).  One more call with BK_DEBUG=fragsize reads the library's own line about the
equal-position walks: records looked up, records the walks read, the longest walk, walks a whole wavefront finished.

    python tools/gpu_fragsize_bench.py [--records 620000000] [--reps 7] [--out profiles/FILE.json]

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
SCOPE = "fragment_sizes"


def call_sites(np, abi, cl, jn):
    """one site per cluster row: a voted row at its voted positions with the sides of bk_junction_sides (the first largest count of the
    split reads, else of the pairs, else (0, 1)), every other row skipped"""
    splits, pairs = jn["splits"].astype(np.int64), jn["pairs"].astype(np.int64)
    idx = np.where(splits.max(axis=1) > 0, splits.argmax(axis=1), np.where(pairs.max(axis=1) > 0, pairs.argmax(axis=1), 1))
    voted = (cl["flags"] & 2) != 0
    sites = np.zeros(len(cl), abi.FRAG_SITE)
    sites["pos1"], sites["pos2"] = cl["p1_exact"], cl["p2_exact"].astype(np.uint32)
    sites["right1"], sites["right2"] = idx >> 1, idx & 1
    sites["skip"] = ~voted
    for f in ("pos1", "pos2", "right1", "right2"):
        sites[f][~voted] = 0
    return sites, voted


def walk_line(ctx, sites, lo, hi):
    """the library's own line about one call (BK_DEBUG=fragsize, on stderr)"""
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.environ["BK_DEBUG"] = "fragsize"
        try:
            os.dup2(tmp.fileno(), 2)
            ctx.fragment_sizes(sites, lo, hi)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("BK_DEBUG", None)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"(\d+) records looked up, their walks read (\d+) records, the longest (\d+), (\d+) finished by a wavefront", text)
    return [int(x) for x in m.groups()] if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qual", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi, synth_gpu

    dev = torch.device("cuda", 0)
    _, total_b = torch.cuda.mem_get_info(dev)
    n_rec = args.records
    while n_rec * 110 > total_b and n_rec > 1_000_000:  # as bench.py sizes the table
        n_rec //= 2
    contigs, cols = synth_gpu.make_wgs(n_rec, args.seed, dev)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    t = capi.Context(contigs, device=0)
    t.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
    w, n_valid = t.run(qual=args.qual, fast=True)
    mean, sd = t.isize_stats()
    lo, hi = capi.fragment_bounds(mean, sd)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    jn = t.junctions()
    sites, voted = call_sites(np, abi, cl, jn)
    for k in np.flatnonzero(voted)[:100]:
        assert capi.junction_sides(jn[k])[:2] == (int(sites[k]["right1"]), int(sites[k]["right2"]))

    rows = t.fragment_sizes(sites, lo, hi)  # warm-up: the call's buffers are allocated here
    wall, event = [], []
    touched = 0
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.fragment_sizes(sites, lo, hi)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched()) if name == SCOPE}  # (the scopes accumulate: the last one)
        event.append(seen[SCOPE][0])
        touched = int(seen[SCOPE][1])
    t.timing_enable(False)
    walks = walk_line(t, sites, lo, hi)

    used, off, lost = (int(rows[f].astype(np.int64).sum()) for f in ("n_used", "n_off", "n_lost"))
    whole = float(np.median(event))
    with_used = rows[rows["n_used"] > 0]
    z = (with_used["sum"] / with_used["n_used"] - mean) / sd if sd else np.zeros(0)
    out = {
        "what": "bk_fragment_sizes of every voted call of a configs[1]-shaped synthetic table at its voted positions, after one -fast step",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(voted.sum()), "sites": int(len(sites)), "reps": args.reps, "mean": mean, "sd": sd,
        "lo": lo, "hi": hi, "pair_rows_of_voted_calls": used + off + lost, "used": used, "off": off, "lost": lost,
        "event_ms": [round(x, 4) for x in event], "event_ms_median": round(whole, 4), "event_ms_min": round(min(event), 4), "event_ms_max": round(max(event), 4),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": touched, "tb_per_s": round(touched / (whole * 1e-3) / 1e12, 5) if whole > 0 else None,
        "fraction_of_8_tb_per_s": round(touched / (whole * 1e-3) / HBM_BYTES_PER_S, 6) if whole > 0 else None,
        "calls_per_s": round(int(voted.sum()) / (whole * 1e-3), 0) if whole > 0 else None,
        "records_looked_up": walks[0] if walks else None, "records_walked": walks[1] if walks else None, "longest_walk": walks[2] if walks else None,
        "wavefront_walks": walks[3] if walks else None, "mean_walk": round(walks[1] / walks[0], 4) if walks and walks[0] else None,
        "n_short": int(rows["n_short"].astype(np.int64).sum()), "n_long": int(rows["n_long"].astype(np.int64).sum()),
        "z_median": round(float(np.median(z)), 3) if len(z) else None, "z_abs_above_3": int((np.abs(z) > 3).sum()) if len(z) else 0,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

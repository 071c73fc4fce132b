"""Measurement: what `bk_locus_partners` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it) and one hot-path step run
on it.  The sites are the two sides of every voted call (bk_call_partner_sites with the run's w), max_gap = int(w): what the command
line's `-partners -all` asks.  After a warm-up call the sites are answered `--reps` times; each repetition gives the HIP-event time of
the scope `locus_partners` and of the two scopes inside it, `locus_partners_index` (keys of the 2 P ends, their sort, the gather of the
mates' keys) and `locus_partners_sites` (count, scan, the host's read of the row total, expand, the two sorts of the rows, runs), and
the wall clock around the call from Python (that plus the host's check, the upload and the copy back).  The scope is reported as a
fraction of 8 TB/s by the library's own byte model (bk_timing_touched).  The row total, the number of elsewhere ends over all sites,
comes out of that model and is printed with it; so are the totals of the columns.

    python tools/gpu_partners_bench.py [--records 620000000] [--reps 7] [--out profiles/FILE.json]

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
SCOPES = ("locus_partners", "locus_partners_index", "locus_partners_sites")


def call_sites(np, abi, cl, w):
    """bk_call_partner_sites over a whole cluster table: rows 2 k and 2 k + 1 are the two sides of cluster k"""
    W = int(w)
    win = {}
    for s in ("p1", "p2"):
        a = np.clip(cl[s + "_min"].astype(np.int64) - W, 1, 0xFFFFFFFF)
        b = np.minimum(cl[s + "_max"].astype(np.int64) + W, 0xFFFFFFFF)
        bad = b < a
        a[bad], b[bad] = 1, 0
        win[s] = (cl[s + "_tid"], a, b)
    sites = np.zeros(2 * len(cl), abi.PARTNER_SITE)
    for first, (own, mate) in enumerate((("p1", "p2"), ("p2", "p1"))):
        for f, v in zip(("tid", "beg", "end"), win[own]):
            sites[f][first::2] = v
        for f, v in zip(("mtid", "mbeg", "mend"), win[mate]):
            sites[f][first::2] = v
    return sites


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
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    voted = cl[(cl["flags"] & 2) != 0]
    sites = call_sites(np, abi, voted, w)
    for k in range(min(100, len(voted))):
        assert capi.call_partner_sites(voted[k], w).tobytes() == sites[2 * k:2 * k + 2].tobytes()
    gap = max(int(w), 0)

    rows = t.locus_partners(sites, gap)  # warm-up: the call's buffers are allocated here
    wall, event = [], {name: [] for name in SCOPES}
    touched = {}
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.locus_partners(sites, gap)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched()) if name in SCOPES}  # (the scopes accumulate: the last ones)
        for name in SCOPES:
            event[name].append(seen[name][0])
            touched[name] = int(seen[name][1])
    t.timing_enable(False)

    n_rows = int(rows["ends"].astype(np.int64).sum() - rows["to_partner"].astype(np.int64).sum())
    n_pairs = (touched["locus_partners_index"] // 80) if touched else 0  # (56 + 2 * 12 bytes per pair)
    med = {name: float(np.median(event[name])) for name in SCOPES}
    whole, model = med["locus_partners"], touched["locus_partners"]
    out = {
        "what": "bk_locus_partners of the two sides of every voted call of a configs[1]-shaped synthetic table, after one -fast step, max_gap = int(w)",
        "records": int(cols["n"]), "pairs": int(n_pairs), "ends": int(2 * n_pairs), "clusters": int(len(cl)), "voted": int(len(voted)), "sites": int(len(sites)),
        "reps": args.reps, "w": w, "max_gap": gap,
        "event_ms": [round(x, 4) for x in event["locus_partners"]], "event_ms_median": round(whole, 4), "event_ms_min": round(min(event["locus_partners"]), 4),
        "event_ms_max": round(max(event["locus_partners"]), 4),
        "index_ms": [round(x, 4) for x in event["locus_partners_index"]], "index_ms_median": round(med["locus_partners_index"], 4),
        "sites_ms": [round(x, 4) for x in event["locus_partners_sites"]], "sites_ms_median": round(med["locus_partners_sites"], 4),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "elsewhere_rows": n_rows, "model_bytes": model, "model_bytes_index": touched["locus_partners_index"], "model_bytes_sites": touched["locus_partners_sites"],
        "tb_per_s": round(model / (whole * 1e-3) / 1e12, 5) if whole > 0 else None,
        "fraction_of_8_tb_per_s": round(model / (whole * 1e-3) / HBM_BYTES_PER_S, 6) if whole > 0 else None,
        "sites_per_s": round(len(sites) / (whole * 1e-3), 0) if whole > 0 else None,
        "ends_in_windows": int(rows["ends"].astype(np.int64).sum()), "ends_to_partner": int(rows["to_partner"].astype(np.int64).sum()),
        "ends_widest_window": int(rows["ends"].max()) if len(rows) else 0, "loci_total": int(rows["loci"].astype(np.int64).sum()),
        "loci_most": int(rows["loci"].max()) if len(rows) else 0, "top_n_largest": int(rows["top_n"].max()) if len(rows) else 0,
        "sites_with_elsewhere": int((rows["top_n"] > 0).sum()),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""Measurement: what `bk_window_context` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it), one hot-path step
(-fast) gives the calls, and every voted call gets the four flank windows of `bk_call_windows` with its own sides (bk_junctions,
bk_junction_sides), 500-base flanks, as `-context` asks for them.  After a warm-up call the windows are answered `--reps` times; each
repetition gives the HIP-event times of the scopes `window_context` (the whole), `window_context_tiles` (the tile pass and its five
scans) and `window_context_windows` (the window kernel), and the wall clock around the call from Python (that plus the upload of the
windows and the copy back of the rows).  The tile pass is reported as a fraction of 8 TB/s by the library's own byte model
(bk_timing_touched: 19 bytes of every record, 40 bytes per tile).  Its yardstick, `window_coverage_tiles` of `bk_window_coverage`
over the same windows of the same table, is measured in the same process, the two calls alternating.

    python tools/gpu_context_bench.py [--records 620000000] [--reps 7] [--flank 500] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCOPES = ("window_context", "window_context_tiles", "window_context_windows")
YARDSTICK = ("window_coverage", "window_coverage_tiles", "window_coverage_windows")
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--flank", type=int, default=500)
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
    junctions = t.junctions()
    lens = np.asarray([l for _, l in contigs], np.uint32)
    voted = np.flatnonzero((cl["flags"] & 2) != 0)
    windows = np.zeros(4 * len(voted), abi.COV_WINDOW)
    for k, i in enumerate(voted):
        r1, r2, _ = capi.junction_sides(junctions[i])
        windows[4 * k:4 * k + 4] = capi.call_windows(cl[i], r1, r2, args.flank, lens)[:4]
    rows = t.window_context(windows, args.qual)  # warm-up: the call's buffers are allocated here
    cov = t.window_coverage(windows, args.qual)
    size = windows["end"].astype(np.int64) - windows["beg"].astype(np.int64)
    full = size == args.flank
    assert full.sum() > len(windows) // 2 and (rows["reads"][full] > 0).mean() > 0.9  # the table covers its calls
    # adjacent windows add: the two flanks of a side against the one window over both
    both = windows[0::2].copy()
    both["end"] = windows[1::2]["end"]
    joined = (windows[0::2]["end"] == windows[1::2]["beg"]) & (size[0::2] > 0) & (size[1::2] > 0)
    whole = t.window_context(both, args.qual)
    for f in abi.WINDOW_CTX.names:
        assert (whole[f][joined] == rows[f][0::2][joined] + rows[f][1::2][joined]).all(), f
    wall = []
    event = {s: [] for s in SCOPES + YARDSTICK}
    model = {}
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.window_context(windows, args.qual)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        assert t.window_coverage(windows, args.qual).tobytes() == cov.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched())}  # (the scopes accumulate: the last of each)
        for s in SCOPES + YARDSTICK:
            event[s].append(seen[s][0])
            model[s] = int(seen[s][1])
    t.timing_enable(False)
    med = {s: float(np.median(event[s])) for s in event}
    fraction = lambda s: round(model[s] / (med[s] * 1e-3) / HBM_BYTES_PER_S, 4) if med[s] > 0 else None
    reads = int(rows["reads"].sum())
    out = {
        "what": "bk_window_context of four flank windows per voted call of a configs[1]-shaped synthetic table, after one -fast step; "
                "bk_window_coverage over the same windows as the yardstick, alternating",
        "records": int(cols["n"]), "cigar_words": int(cols["n_cigar_words"]), "tiles": (int(cols["n"]) + 255) // 256, "clusters": int(len(cl)), "voted": int(len(voted)),
        "windows": int(len(windows)), "flank": args.flank, "mapq_min": args.qual, "reps": args.reps, "w": w,
        "event_ms": {s: [round(x, 4) for x in event[s]] for s in event}, "event_ms_median": {s: round(med[s], 4) for s in event},
        "event_ms_min": {s: round(min(event[s]), 4) for s in event}, "event_ms_max": {s: round(max(event[s]), 4) for s in event},
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": model, "tiles_tb_per_s": round(model["window_context_tiles"] / (med["window_context_tiles"] * 1e-3) / 1e12, 3),
        "tiles_fraction_of_8_tb_per_s": fraction("window_context_tiles"), "yardstick_tiles_fraction_of_8_tb_per_s": fraction("window_coverage_tiles"),
        "windows_per_s": round(len(windows) / (med["window_context_windows"] * 1e-3), 0) if med["window_context_windows"] > 0 else None,
        "reads_in_windows": reads, "reads_per_full_window_median": float(np.median(rows["reads"][full])),
        "shares": {f: round(int(rows[f].sum()) / reads, 5) for f in ("mq0", "lowq", "clipped", "improper")} if reads else {},
        "counts": {f: int(rows[f].sum()) for f in ("orphan", "dup", "secsup")}, "mean_mapq": round(int(rows["mapq_sum"].sum()) / reads, 3) if reads else None,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

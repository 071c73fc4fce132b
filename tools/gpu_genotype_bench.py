"""Measurement: what `bk_ref_support` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it), one hot-path step
(-fast) gives the calls, and the sample itself is genotyped (`records == calls`): a warm-up call, then `--reps` calls, each with the
HIP-event time of the call's `ref_support` scope (the device work: the sampled search keys and k_ref_support), the wall clock around
the call from Python (that plus the copy back of one row per call), the records visited and the bytes by the
library's model (bk_timing: 19 B per visited record; bk_timing_touched: those, the CIGAR words walked and the rows).

The yardstick is k_bp_depth of the same process (same calls, same searches, a one-base window); it has no scope of its own, so it
is read from a kernel trace:

    python tools/gpu_genotype_bench.py [--records 620000000] [--reps 7] [--anchor 10] [--out profiles/FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o geno -- python tools/gpu_genotype_bench.py --reps 3

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--anchor", type=int, default=10)
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
    sup = t.ref_support(t, args.qual, args.anchor, w)  # warm-up: the call's buffers are allocated here
    wall, event, visited, touched = [], [], [], []
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sup = t.ref_support(t, args.qual, args.anchor, w)
        wall.append((time.perf_counter() - t0) * 1e3)
        rows = [(ms, by, tb) for (name, ms, by), tb in zip(t.timing(), t.timing_touched()) if name == "ref_support"]
        ms, by, tb = rows[-1]  # (the scopes accumulate)
        event.append(ms)
        visited.append(by // 19)
        touched.append(tb)
    t.timing_enable(False)
    voted = (cl["flags"] & 2) != 0
    ev = float(np.median(event))
    gts = np.asarray([capi.genotype_call(int(c["n_sr"]), (int(s["ref_reads1"]) + int(s["ref_reads2"]) + 1) // 2)[0] for c, s in zip(cl[voted], sup[voted])], np.int64)
    out = {
        "what": "bk_ref_support of a configs[1]-shaped synthetic table on itself (records == calls), after one -fast step",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(voted.sum()), "w": w, "anchor": args.anchor, "mapq_min": args.qual, "reps": args.reps,
        "event_ms": [round(x, 4) for x in event], "wall_ms": [round(x, 3) for x in wall],
        "event_ms_median": round(ev, 4), "wall_ms_median": round(float(np.median(wall)), 3),
        "records_visited": int(visited[-1]), "visited_per_window": round(visited[-1] / max(1, 2 * int(voted.sum())), 1),
        "model_bytes": int(touched[-1]), "model_tb_per_s": round(touched[-1] / (ev * 1e-3) / 1e12, 3) if ev > 0 else None,
        "ref_reads_sum": int(sup["ref_reads1"].sum() + sup["ref_reads2"].sum()), "ref_pairs_sum": int(sup["ref_pairs1"].sum() + sup["ref_pairs2"].sum()),
        "gt_counts": {"0/0": int((gts == 0).sum()), "0/1": int((gts == 1).sum()), "1/1": int((gts == 2).sum()), "./.": int((gts == 255).sum())},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""One-off measurement: what `bk_normal_support` costs at the bench shape.

Two configs[1]-shaped tables are generated in HBM (breakid_amd.synth_gpu.make_wgs, as bench.py does), resident together: the
tumour runs the whole hot path (-fast), the normal only its record-level stages (stream pass, mate join with the tumour's w,
split evidence).  The normal is generated with the tumour's seed, so every tumour call finds its own pairs and tuples in the
normal: the windows are as full as they get.  Then `normal_support` is timed `--reps` times: wall clock around the call
(index sort, three kernels, copy back of one 16-byte row per cluster) and the HIP-event time of its stage scope.

    python tools/gpu_normal_cost.py [--records 620000000] [--reps 5] [--out profiles/FILE.json]

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi, synth_gpu

    dev = torch.device("cuda", 0)
    _, total_b = torch.cuda.mem_get_info(dev)
    n_rec = args.records
    while 2 * n_rec * 110 > total_b and n_rec > 1_000_000:  # two tables (bench.py sizes one at ~110 B per record)
        n_rec //= 2
    tables = []
    for _ in range(2):
        contigs, cols = synth_gpu.make_wgs(n_rec, args.seed, dev)
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        tables.append((contigs, cols))

    def attach(contigs, cols):
        ctx = capi.Context(contigs, device=0)
        ctx.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
        return ctx

    t = attach(*tables[0])
    w, n_valid = t.run(qual=20, fast=True)
    n = attach(*tables[1])
    n.isize_stats()
    n_pairs, _ = n.discordant_pairs(20, w)
    n_tuples = n.split_evidence()
    n.sync()
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    sup = t.normal_support(n, w)  # warm-up: the index buffers are allocated here
    wall, event = [], []
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sup = t.normal_support(n, w)
        wall.append((time.perf_counter() - t0) * 1e3)
        event.append([ms for name, ms, _ in t.timing() if name == "normal_support"][-1])  # (the scopes accumulate)
    t.timing_enable(False)
    voted = (cl["flags"] & 2) != 0
    out = {
        "what": "bk_normal_support, tumour and normal = configs[1]-shaped synthetic tables (same seed), both resident",
        "records_per_table": int(tables[0][1]["n"]), "clusters": int(len(cl)), "voted": int(voted.sum()), "normal_pairs": int(n_pairs),
        "normal_tuples": int(n_tuples), "w": w, "reps": args.reps,
        "wall_ms": [round(x, 3) for x in wall], "event_ms": [round(x, 3) for x in event],
        "wall_ms_median": round(float(np.median(wall)), 3), "event_ms_median": round(float(np.median(event)), 3),
        "n_sr_ge_1_voted": bool((sup["n_sr"][voted] >= 1).all()),
        "depth_equal_voted": bool(np.array_equal(sup["depth1"][voted], cl["depth1"][voted]) and np.array_equal(sup["depth2"][voted], cl["depth2"][voted])),
        "n_drp_sum": int(sup["n_drp"].sum()), "n_drp_max": int(sup["n_drp"].max()) if len(sup) else 0,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()
    n.close()


if __name__ == "__main__":
    main()

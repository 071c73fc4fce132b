"""Measurement: what `bk_junctions` costs at the bench shape, with `bk_normal_support` of the same process as the yardstick.

Two configs[1]-shaped tables are generated in HBM (breakid_amd.synth_gpu.make_wgs, as tools/gpu_normal_cost.py does), resident
together: the tumour runs the whole hot path (-fast), the normal only its record-level stages.  After a warm-up of both calls,
`--reps` calls of each: the HIP-event time of the call's scope (`junctions`: the clear and the two kernels; `normal_support`: index
sort, kernels and copy back), the wall clock around the call from Python, and for
`junctions` the bytes by the library's model (bk_timing: 16 B per list entry; bk_timing_touched: 44 B per list entry, 88 B per tuple
searched, the rows).  The normal holds the tumour's own records (same seed), so the four `splits` bins of every row must sum to
its `n_sr`.

    python tools/gpu_junction_bench.py [--records 620000000] [--reps 7] [--out profiles/FILE.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o junc -- python tools/gpu_junction_bench.py --reps 3

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
    junc = t.junctions()  # warm-up: the buffers of both calls are allocated here
    sup = t.normal_support(n, w)
    res = {"junctions": ([], [], [], []), "normal_support": ([], [], [], [])}
    t.timing_enable(True)
    for _ in range(args.reps):
        for name, call in (("junctions", lambda: t.junctions()), ("normal_support", lambda: t.normal_support(n, w))):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = call()
            wall, event, model, touched = res[name]
            wall.append((time.perf_counter() - t0) * 1e3)
            rows = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == name]
            event.append(rows[-1][0])  # (the scopes accumulate)
            model.append(rows[-1][1])
            touched.append(rows[-1][2])
            if name == "junctions":
                junc = out
            else:
                sup = out
    t.timing_enable(False)
    voted = (cl["flags"] & 2) != 0
    ev_j, ev_n = float(np.median(res["junctions"][1])), float(np.median(res["normal_support"][1]))
    list_entries = res["junctions"][2][-1] // 16
    out = {
        "what": "bk_junctions, and bk_normal_support as its yardstick, on two configs[1]-shaped synthetic tables (same seed), both resident",
        "records_per_table": int(tables[0][1]["n"]), "clusters": int(len(cl)), "voted": int(voted.sum()), "clustered_list_entries": int(list_entries),
        "tuples": int(n_tuples), "normal_pairs": int(n_pairs), "w": w, "reps": args.reps,
        "junctions_event_ms": [round(x, 4) for x in res["junctions"][1]], "junctions_wall_ms": [round(x, 3) for x in res["junctions"][0]],
        "junctions_event_ms_median": round(ev_j, 4), "junctions_wall_ms_median": round(float(np.median(res["junctions"][0])), 3),
        "normal_support_event_ms": [round(x, 4) for x in res["normal_support"][1]], "normal_support_wall_ms": [round(x, 3) for x in res["normal_support"][0]],
        "normal_support_event_ms_median": round(ev_n, 4), "normal_support_wall_ms_median": round(float(np.median(res["normal_support"][0])), 3),
        "junctions_model_bytes": int(res["junctions"][3][-1]),
        "junctions_tuples_searched": int((res["junctions"][3][-1] - list_entries * 44 - len(cl) * (72 + 2 * 48 + 4)) // 88),
        "junctions_model_tb_per_s": round(res["junctions"][3][-1] / (ev_j * 1e-3) / 1e12, 3) if ev_j > 0 else None,
        "pairs_sum_equals_n_drp": bool(np.array_equal(junc["pairs"].astype(np.int64).sum(1), cl["n_drp"].astype(np.int64))),
        "splits_sum_equals_normal_n_sr": bool(np.array_equal(junc["splits"].astype(np.int64).sum(1), sup["n_sr"].astype(np.int64))),
        "splits_bins": [int(x) for x in junc["splits"].astype(np.int64).sum(0)], "pairs_bins": [int(x) for x in junc["pairs"].astype(np.int64).sum(0)],
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

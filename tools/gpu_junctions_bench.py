"""Measurement: what `bk_split_junctions` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it) and one hot-path step
(-fast) runs on it; `bk_split_junctions` then works on the step's own BK_STAGE_SPLITS with `--tol` 2 and `--support` 1, so that every
call is returned.  After a warm-up call it is repeated `--reps` times; each repetition gives the HIP-event time of the scope
`split_junctions` (which holds the host's reads of the counts and of the changed flag between the rounds: the device waits for them)
and the wall clock around the call from Python (that plus the upload of the voted rows' sorted breakpoints, which the warm-up call
fetched and sorted once, and the copy back of the rows).  The scope is reported as a fraction of 8 TB/s by the library's own byte
model (bk_timing_touched).  Nothing is compared against a target: the tool only records.

    python tools/gpu_junctions_bench.py [--records 620000000] [--reps 7] [--tol 2] [--support 1] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCOPE = "split_junctions"
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--tol", type=int, default=2)
    ap.add_argument("--support", type=int, default=1)
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
    rows = t.split_junctions(args.qual, args.tol, args.support)  # warm-up: the call's buffers are allocated here
    counts = t.split_junction_counts()
    wall, event, model = [], [], 0
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.split_junctions(args.qual, args.tol, args.support)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched())}  # (the scopes accumulate: the last of each)
        event.append(seen[SCOPE][0])
        model = int(seen[SCOPE][1])
    t.timing_enable(False)
    med = float(np.median(event))
    out = {
        "what": "bk_split_junctions on the BK_STAGE_SPLITS of one -fast step over a configs[1]-shaped synthetic table",
        "records": int(cols["n"]), "voted": int(n_valid), "w": w, "tol": args.tol, "min_reads": args.support, "mapq_min": args.qual, "reps": args.reps,
        "tuples": counts["tuples"], "eligible_tuples": counts["eligible"], "exact_junctions": counts["exact"], "calls": counts["calls"], "returned_calls": int(len(rows)),
        "claimed_calls": counts["claimed"], "component_rounds": counts["rounds"],
        "calls_with_3_reads": int((rows["n_reads"] >= 3).sum()), "unclaimed_with_3_reads": int(((rows["n_reads"] >= 3) & (rows["call"] < 0)).sum()),
        "most_exact_in_a_call": int(rows["n_exact"].max()) if len(rows) else 0,
        "event_ms": [round(x, 4) for x in event], "event_ms_median": round(med, 4), "event_ms_min": round(min(event), 4), "event_ms_max": round(max(event), 4),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": model, "fraction_of_8_tb_per_s": round(model / (med * 1e-3) / HBM_BYTES_PER_S, 6) if med > 0 else None,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""Measurement: what `bk_evidence` costs at the bench shape, with `bk_junctions` on the same context beside it (both cover the
same input: one counts, the other lists).

One configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs) and runs the whole hot path (-fast).  After a
warm-up of both calls, `--reps` calls of each: the HIP-event time of the call's scope (`junctions`: the clear and the two
kernels; `evidence`: those, the scans, the sort of the clustered list and the two emit kernels, with the one 8-byte read-back
that sizes the output), the wall clock around the call from Python (copy back included), and the bytes by the library's model.

    python tools/gpu_evidence_bench.py [--records 620000000] [--reps 7] [--out profiles/FILE.json]

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
    if args.reps < 1:
        raise SystemExit("gpu_evidence_bench.py: --reps must be >= 1")

    import numpy as np
    import torch
    from breakid_amd import abi, capi, synth_gpu

    dev = torch.device("cuda", 0)
    _, total_b = torch.cuda.mem_get_info(dev)
    n_rec = args.records
    while n_rec * 110 > total_b and n_rec > 1_000_000:  # (bench.py sizes a table at ~110 B per record)
        n_rec //= 2
    contigs, cols = synth_gpu.make_wgs(n_rec, args.seed, dev)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    t = capi.Context(contigs, device=0)
    t.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
    w, n_valid = t.run(qual=20, fast=True)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    junc = t.junctions()  # warm-up: the buffers of both calls are allocated here
    rows, off = t.evidence()
    res = {"junctions": ([], [], []), "evidence": ([], [], [])}
    same = True
    t.timing_enable(True)
    for _ in range(args.reps):
        for name, call in (("junctions", t.junctions), ("evidence", t.evidence)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = call()
            wall, event, touched = res[name]
            wall.append((time.perf_counter() - t0) * 1e3)
            got = [(ms, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == name]
            event.append(got[-1][0])  # (the scopes accumulate)
            touched.append(got[-1][1])
            if name == "evidence":
                same = same and out[0].tobytes() == rows.tobytes() and out[1].tobytes() == off.tobytes()
    t.timing_enable(False)
    pe = rows["kind"] == abi.EV_PAIR
    out = {
        "what": "bk_evidence, and bk_junctions on the same context beside it, on one configs[1]-shaped synthetic table",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(((cl["flags"] & 2) != 0).sum()), "rows": int(len(rows)), "pair_rows": int(pe.sum()),
        "split_rows": int((~pe).sum()), "reps": args.reps,
        "evidence_event_ms": [round(x, 4) for x in res["evidence"][1]], "evidence_event_ms_median": round(float(np.median(res["evidence"][1])), 4),
        "evidence_wall_ms_median": round(float(np.median(res["evidence"][0])), 3),
        "junctions_event_ms": [round(x, 4) for x in res["junctions"][1]], "junctions_event_ms_median": round(float(np.median(res["junctions"][1])), 4),
        "junctions_wall_ms_median": round(float(np.median(res["junctions"][0])), 3),
        "evidence_touched_bytes": int(res["evidence"][2][-1]), "junctions_touched_bytes": int(res["junctions"][2][-1]),
        "pair_rows_equal_n_drp": bool(int(pe.sum()) == int(cl["n_drp"].astype(np.int64).sum())),
        "split_rows_equal_junction_splits": bool(int((~pe).sum()) == int(junc["splits"].astype(np.int64).sum())),
        "every_call_gives_the_same_bytes": bool(same),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

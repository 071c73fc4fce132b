"""Measurement: what `bk_unique_support` costs at the bench shape, beside `bk_evidence` on the same context.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it) and one hot-path step
(-fast) gives the clusters.  `bk_evidence` lists the rows once; `bk_unique_support` lists them again (keys instead of rows), sorts the
row indices by the key words and walks the runs.  After a warm-up call each runs `--reps` times, `bk_unique_support` as a listing and
as counts only, each with the HIP-event time of the call's scope (`evidence`, `unique`: the device work, the row-count read-backs
inside it included) and the bytes of the library's model (bk_timing, bk_timing_touched).

    python tools/gpu_unique_bench.py [--records 620000000] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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

    def scope(name):
        rows = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == name]
        return rows[-1]  # (the scopes accumulate)

    def measure(call, name):
        call()  # warm-up: the call's buffers are allocated here
        ev, by, tb = [], 0, 0
        t.timing_enable(True)
        for _ in range(args.reps):
            call()
            ms, by, tb = scope(name)
            ev.append(ms)
        t.timing_enable(False)
        return {"event_ms": [round(x, 4) for x in ev], "event_ms_median": round(float(np.median(ev)), 4), "bytes": int(by), "model_bytes": int(tb)}

    rows, off = t.evidence()
    us, first = t.unique_support()
    n_pair = int((rows["kind"] == abi.EV_PAIR).sum())
    out = {
        "what": "bk_evidence and bk_unique_support of a configs[1]-shaped synthetic table, after one -fast step",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(((cl["flags"] & 2) != 0).sum()), "w": w, "mapq_min": args.qual, "reps": args.reps,
        "rows": int(len(rows)), "pair_rows": n_pair, "split_rows": int(len(rows)) - n_pair,
        "fragments": int((first == np.arange(len(first), dtype=np.uint64)).sum()),
        "uniq_pairs": int(us["uniq_pairs"].sum()), "uniq_splits": int(us["uniq_splits"].sum()),
        "top_pairs_max": int(us["top_pairs"].max()) if len(us) else 0, "top_splits_max": int(us["top_splits"].max()) if len(us) else 0,
        "evidence": measure(lambda: t.evidence(), "evidence"),
        "unique_listing": measure(lambda: t.unique_support(), "unique"),
        "unique_counts_only": measure(lambda: t.unique_support(listing=False), "unique"),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

"""Measurement: what `bk_clip_reads` costs at the bench shape, beside `bk_clip_support` on the same context.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it) and one hot-path step
(-fast) gives the clusters.  `bk_clip_support` runs on the sample itself; its rows give two sets of sites: the rescued ones (the two
peaks of every cluster `bk_clip_rescue` accepts at --support, tol 0: what `-clip -evidence` asks for) and every (row, side, dir) peak
(tol 0: the sites of the first identity).  After a warm-up call each runs `--reps` times as a listing and as counts only, each with the
HIP-event time of the call's scope (`clip_support`, `clip_reads`: the device work), the records visited (bk_timing bytes / 15 per
pass) and the bytes of the library's model (bk_timing_touched).

    python tools/gpu_clip_reads_bench.py [--records 620000000] [--reps 7] [--minclip 10] [--support 3] [--out profiles/FILE.json]

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
    ap.add_argument("--minclip", type=int, default=10)
    ap.add_argument("--support", type=int, default=3)
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
    sup = t.clip_support(t, args.qual, args.minclip, w)  # warm-up: the call's buffers are allocated here
    jn = t.junctions()
    rescued, peaks = [], []
    for c, j, s in zip(cl, jn, sup):
        res = capi.clip_rescue(c, j, s, args.support)
        if res:
            d = capi.junction_sides(j)
            rescued += [(int(c["p1_tid"]), res[0], 0, d[0]), (int(c["p2_tid"]), res[1], 0, d[1])]
        for side in (0, 1):
            for dr in (0, 1):
                peaks.append((int(c["p%d_tid" % (side + 1)]), int(s["peak_pos"][side][dr]), 0, dr))

    def scope(name):
        rows = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == name]
        return rows[-1]  # (the scopes accumulate)

    def measure(call, name):
        call()
        ev, by, tb = [], 0, 0
        t.timing_enable(True)
        for _ in range(args.reps):
            call()
            ms, by, tb = scope(name)
            ev.append(ms)
        t.timing_enable(False)
        return {"event_ms": [round(x, 4) for x in ev], "event_ms_median": round(float(np.median(ev)), 4), "bytes": int(by), "model_bytes": int(tb)}

    out = {
        "what": "bk_clip_support and bk_clip_reads of a configs[1]-shaped synthetic table on itself, after one -fast step",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(((cl["flags"] & 2) != 0).sum()), "w": w, "min_clip": args.minclip, "mapq_min": args.qual,
        "min_support": args.support, "reps": args.reps,
        "clip_support": measure(lambda: t.clip_support(t, args.qual, args.minclip, w), "clip_support"),
    }
    for label, sites in (("rescued_sites", rescued), ("peak_sites", peaks)):
        a = np.zeros(len(sites), abi.CLIP_SITE)
        for k, x in enumerate(sites):
            a[k] = x
        counts, rows, off = t.clip_reads(a, args.qual, args.minclip)
        out[label] = {"sites": len(a), "rows": int(len(rows)),
                      "listing": measure(lambda: t.clip_reads(a, args.qual, args.minclip), "clip_reads"),
                      "counts_only": measure(lambda: t.clip_reads(a, args.qual, args.minclip, listing=False), "clip_reads")}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

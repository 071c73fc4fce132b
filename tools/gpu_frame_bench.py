"""Measurement: what `bk_fusion_frame` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it), one hot-path step
(-fast) gives the calls, and every voted call is one site with its own sides (bk_junctions, bk_junction_sides).  The model:
`synth.random_refgene` over the table's contigs, as many rows as give `--transcripts` coding ones (one row in eleven is NR_ and is
skipped, as the command line skips it).  After a warm-up call the sites are answered `--reps` times; each repetition gives the
HIP-event time of the scope `fusion_frame` (the derived arrays and the site kernel) and the wall clock around the call from Python
(that plus the host's check of the model, the uploads and the copy back).  The scope is also reported as a fraction of 8 TB/s by the
library's own byte model (bk_timing_touched); the kernel is bound by the latency of its dependent searches, not by bytes.

For orientation the host's nested scan is timed on one core: every transcript tested against either side of a site, the form of
annotate_side (numpy over the transcripts, integer contig ids in place of its string compares), on `--host-sites` sites and scaled
to all of them.

    python tools/gpu_frame_bench.py [--records 620000000] [--transcripts 40000] [--reps 7] [--out profiles/FILE.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--transcripts", type=int, default=40_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qual", type=int, default=20)
    ap.add_argument("--host-sites", type=int, default=4000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi, synth, synth_gpu

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
    voted = np.flatnonzero((cl["flags"] & 2) != 0)
    sites = np.zeros(len(voted), abi.FRAME_SITE)
    for k, i in enumerate(voted):
        r1, r2, _ = capi.junction_sides(junctions[i])
        sites[k]["tid1"], sites[k]["pos1"], sites[k]["right1"] = cl[i]["p1_tid"], cl[i]["p1_exact"], r1
        sites[k]["tid2"], sites[k]["pos2"], sites[k]["right2"] = cl[i]["p2_tid"], cl[i]["p2_exact"], r2
    lines = synth.random_refgene(contigs, args.transcripts * 11 // 10, args.seed)
    model, dropped = capi.TxModel.from_refgene(lines, [n for n, _ in contigs])
    m = model.cols

    rows = t.fusion_frame(model, sites)  # warm-up: the call's buffers are allocated here
    wall, event = [], []
    touched = 0
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.fusion_frame(model, sites)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched()) if name == "fusion_frame"}  # (the scopes accumulate: the last one)
        event.append(seen["fusion_frame"][0])
        touched = int(seen["fusion_frame"][1])
    t.timing_enable(False)

    # the host's nested scan on one core, and that it finds what the kernel counted
    torch.set_num_threads(1)
    n_host = min(args.host_sites, len(sites))
    tid, start, end = m["tid"], m["tx_start"].astype(np.int64), m["tx_end"].astype(np.int64)
    t0 = time.perf_counter()
    for k in range(n_host):
        s = sites[k]
        n1 = int(((tid == s["tid1"]) & (start < int(s["pos1"])) & (int(s["pos1"]) <= end)).sum())
        n2 = int(((tid == s["tid2"]) & (start < int(s["pos2"])) & (int(s["pos2"]) <= end)).sum())
        assert [n1, n2] == list(rows[k]["n_tx"])
    host_s = time.perf_counter() - t0

    med = float(np.median(event))
    out = {
        "what": "bk_fusion_frame of one site per voted call of a configs[1]-shaped synthetic table, after one -fast step, against a synth.random_refgene model",
        "records": int(cols["n"]), "clusters": int(len(cl)), "voted": int(len(voted)), "sites": int(len(sites)), "transcripts": len(model), "parts": int(len(m["ex_start"])),
        "refgene_rows": len(lines), "reps": args.reps, "w": w,
        "event_ms": [round(x, 4) for x in event], "event_ms_median": round(med, 4), "event_ms_min": round(min(event), 4), "event_ms_max": round(max(event), 4),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": touched, "tb_per_s": round(touched / (med * 1e-3) / 1e12, 5) if med > 0 else None,
        "fraction_of_8_tb_per_s": round(touched / (med * 1e-3) / HBM_BYTES_PER_S, 6) if med > 0 else None,
        "sites_per_s": round(len(sites) / (med * 1e-3), 0) if med > 0 else None,
        "overlapping_per_side_mean": round(float(rows["n_tx"].mean()), 3), "overlapping_per_side_max": int(rows["n_tx"].max()),
        "pairs_total": int((rows["n_tx"][:, 0].astype(np.int64) * rows["n_tx"][:, 1]).sum()),
        "classes": {abi.FRAME_CLASSES[c]: int((rows["cls"] == c).sum()) for c in range(6)},
        "host_scan_sites": n_host, "host_scan_s": round(host_s, 3), "host_scan_all_sites_s": round(host_s * len(sites) / max(1, n_host), 1),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

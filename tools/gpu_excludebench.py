"""What `bk_exclude_regions` (-x regions.bed) costs at the bench shape.

The configs[1] table is generated in HBM (breakid_amd.synth_gpu.make_wgs, 620 M records, as bench.py does) and handed over by
device pointers (BK_MEM_DEVICE).  The exclude list is seeded and shaped like an hg19 blacklist: 10 kb at each contig end, one 3 Mb
block per contig (centromere-like) and `--random` intervals of 1-50 kb.  Every repetition attaches the table again and runs the
call: the HIP-event time of its steps (k_exclude_classify, the three scans, k_exclude_compact, the bk_side rows) from the context's
timers, their bytes (the library's model, from the column sizes and the kept counts), and the wall clock around the call.

    python tools/gpu_excludebench.py [--records 620000000] [--reps 7] [--random 1000] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out).  Per-kernel statistics: run it under `rocprofv3 --kernel-trace --stats` separately."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = ("k_exclude_classify", "exclude_scan", "k_exclude_compact", "make_side")
HBM_BPS = 8e12


def hg19_like(contigs, seed, n_random):
    import numpy as np
    rng = np.random.default_rng(seed)
    iv = []
    for t, (_, ln) in enumerate(contigs):
        iv += [(t, 0, min(10_000, ln)), (t, max(0, ln - 10_000), ln)]
        blk = min(3_000_000, ln // 10)
        b = int(rng.integers(0, ln - blk))
        iv.append((t, b, b + blk))
    for _ in range(n_random):
        t = int(rng.integers(0, len(contigs)))
        ln = contigs[t][1]
        w = int(rng.integers(1_000, 50_001))
        b = int(rng.integers(0, max(1, ln - w)))
        iv.append((t, b, min(ln, b + w)))
    a = np.asarray(iv, np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=12346)  # bench.py's default: the same table
    ap.add_argument("--random", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from breakid_amd import abi, capi, synth_gpu

    dev = torch.device("cuda", 0)
    _, total_b = torch.cuda.mem_get_info(dev)
    n_rec = args.records
    while n_rec * 200 > total_b and n_rec > 1_000_000:  # the table (~110 B per record) and its kept part
        n_rec //= 2
    contigs, cols = synth_gpu.make_wgs(n_rec, args.seed, dev)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    tid, beg, end = hg19_like(contigs, args.seed, args.random)
    ptrs = abi.device_ptrs(cols)
    ctx = capi.Context(contigs, device=0)

    def once():
        ctx.attach_device(ptrs, cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        removed = ctx.exclude_regions(tid, beg, end)
        return removed, (time.perf_counter() - t0) * 1e3

    once()  # warm-up
    wall, steps = [], []
    removed = 0
    for _ in range(args.reps):
        ctx.timing_enable(True)
        removed, ms = once()
        wall.append(ms)
        t = {name: (ms_, by) for name, ms_, by in ctx.timing() if name in STEPS}
        steps.append(t)
        ctx.timing_enable(False)
    event = [sum(t[s][0] for s in STEPS) for t in steps]
    by = {s: steps[-1][s][1] for s in STEPS}
    total_bytes = sum(by.values())
    med = float(np.median(event))
    out = {
        "what": "bk_exclude_regions on the configs[1]-shaped synthetic table (BK_MEM_DEVICE), hg19-shaped seeded exclude list",
        "records": int(cols["n"]), "cigar_words": int(cols["n_cigar_words"]), "aux_bytes": int(cols["n_aux_bytes"]),
        "intervals": int(len(tid)), "removed": int(removed), "removed_frac": round(removed / max(1, int(cols["n"])), 4), "reps": args.reps,
        "event_ms": [round(x, 3) for x in event], "event_ms_median": round(med, 3),
        "step_ms_median": {s: round(float(np.median([t[s][0] for t in steps])), 3) for s in STEPS},
        "step_bytes": by, "bytes": int(total_bytes),
        "GBps": round(total_bytes / (med * 1e-3) / 1e9, 1), "frac_of_8TBps": round(total_bytes / (med * 1e-3) / HBM_BPS, 4),
        "bound_ms_at_8TBps": round(total_bytes / HBM_BPS * 1e3, 3),
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

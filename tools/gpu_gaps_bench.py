"""Measurement: what `bk_cigar_gaps` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it).  Its CIGAR columns are
then rebuilt on the device: at `--loci` places spread evenly over the table, `--reads` consecutive records (which start within a few
bases of each other: the table is coordinate-sorted) whose CIGAR is the plain 150M get `(70 - d)M 45D (80 + d)M`, d being the distance
of the record's start from the first one's, so that all of them state one deletion.  The share of gapped records and the number of
loci that took are recorded.  No stage runs: `bk_cigar_gaps` works on the attached table, with `--support` 1 so that every call is
returned.  After a warm-up call it is repeated `--reps` times; each repetition gives the HIP-event times of the scopes `cigar_gaps`
(the whole, which holds the host's four reads of a count: the device waits for them), `cigar_gaps_records` (the record pass) and
`cigar_gaps_calls`, and the wall clock around the call from Python.  For orientation the tile pass of `bk_window_context`
(`window_context_tiles`) is timed in the same process.  Scopes are reported as fractions of 8 TB/s by the library's own byte model
(bk_timing_touched).  Nothing is compared against a target: the tool only records.

    python tools/gpu_gaps_bench.py [--records 620000000] [--loci 77500] [--reads 8] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCOPES = ("cigar_gaps", "cigar_gaps_records", "cigar_gaps_calls")
HBM_BYTES_PER_S = 8e12


def add_gaps(cols, loci, reads):
    """rebuilds cigar_off / cigar in place of the old ones; returns the number of gapped records"""
    import torch
    n, dev = cols["n"], cols["tid"].device
    off = cols["cigar_off"].to(torch.int64)
    nops = off[1:] - off[:-1]
    stride = max(reads, n // max(loci, 1))
    first = torch.arange(0, n - reads, stride, device=dev, dtype=torch.int64)[:loci]
    idx = (first[:, None] + torch.arange(reads, device=dev, dtype=torch.int64)[None, :]).reshape(-1)
    head = first.repeat_interleave(reads)
    old = cols["cigar"].to(torch.int64)
    d = cols["pos"][idx].to(torch.int64) - cols["pos"][head].to(torch.int64)
    ok = (nops[idx] == 1) & (old[off[idx]] == (150 << 4)) & (cols["tid"][idx] == cols["tid"][head]) & (cols["tid"][idx] >= 0) & (d >= 0) & (d <= 50)
    idx, d = idx[ok], d[ok]
    new_nops = nops.clone()
    new_nops[idx] = 3
    new_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(new_nops, 0, out=new_off[1:])
    n_words, new_words = cols["n_cigar_words"], int(new_off[-1].item())
    shift = torch.repeat_interleave(new_off[:-1] - off[:-1], nops)
    cigar = torch.zeros(max(new_words, 1), dtype=torch.int64, device=dev)
    cigar[torch.arange(n_words, device=dev, dtype=torch.int64) + shift] = old[:n_words]
    b = new_off[idx]
    cigar[b] = (70 - d) << 4
    cigar[b + 1] = (45 << 4) | 2
    cigar[b + 2] = (80 + d) << 4
    cols["cigar_off"] = new_off.to(torch.int32)
    cols["cigar"] = cigar.to(torch.int32)
    cols["n_cigar_words"] = new_words
    return int(idx.numel()), int(torch.unique(head[ok]).numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--loci", type=int, default=77_500)
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qual", type=int, default=20)
    ap.add_argument("--minlen", type=int, default=20)
    ap.add_argument("--anchor", type=int, default=10)
    ap.add_argument("--tol", type=int, default=2)
    ap.add_argument("--support", type=int, default=1)
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
    gapped, loci = add_gaps(cols, args.loci, args.reads)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    t = capi.Context(contigs, device=0)
    t.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
    params = (args.qual, args.minlen, args.anchor, args.tol, args.support)
    rows = t.cigar_gaps(*params)  # warm-up: the call's buffers are allocated here
    counts = t.cigar_gap_counts()
    windows = np.zeros(1, abi.COV_WINDOW)
    windows["tid"], windows["beg"], windows["end"] = 0, 1000, 2000
    t.window_context(windows, args.qual)
    wall, event, model = [], {s: [] for s in SCOPES + ("window_context_tiles",)}, {}
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.cigar_gaps(*params)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        t.window_context(windows, args.qual)
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched())}  # (the scopes accumulate: the last of each)
        for s in event:
            event[s].append(seen[s][0])
            model[s] = int(seen[s][1])
    t.timing_enable(False)
    med = {s: float(np.median(v)) for s, v in event.items()}
    fraction = lambda s: round(model[s] / (med[s] * 1e-3) / HBM_BYTES_PER_S, 6) if med[s] > 0 else None  # noqa: E731
    out = {
        "what": "bk_cigar_gaps on a configs[1]-shaped synthetic table whose CIGAR columns were rebuilt with three-operation gapped records; no stage ran",
        "records": int(cols["n"]), "cigar_words": int(cols["n_cigar_words"]), "gapped_records": gapped, "gapped_share": round(gapped / max(1, int(cols["n"])), 8), "gapped_loci": loci,
        "reads_per_locus_asked": args.reads, "loci_asked": args.loci,
        "mapq_min": args.qual, "min_len": args.minlen, "anchor": args.anchor, "tol": args.tol, "min_reads": args.support, "reps": args.reps, "counts": counts,
        "returned_calls": int(len(rows)), "calls_with_3_reads": int((rows["n_reads"] >= 3).sum()), "most_rows_in_a_call": int(rows["n_rows"].max()) if len(rows) else 0,
        "event_ms": {s: [round(x, 4) for x in v] for s, v in event.items()}, "event_ms_median": {s: round(v, 4) for s, v in med.items()},
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": model, "fraction_of_8_tb_per_s": {s: fraction(s) for s in event},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

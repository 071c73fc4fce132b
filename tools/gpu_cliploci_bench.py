"""Measurement: what `bk_clip_loci` costs at the bench shape.

The configs[1]-shaped table is generated in HBM (breakid_amd.synth_gpu.make_wgs, sized as bench.py sizes it).  Its CIGAR columns are
then rebuilt on the device: at `--loci` places spread evenly over the table, `--reads` consecutive records (which start within a few
bases of each other: the table is coordinate-sorted) whose CIGAR is the plain 150M and that carry no aux bytes become clipped
alignments.  With d the distance of a record's start from the first one's, the even ones get `(60 - d)M (90 + d)S`, so that all of
them end at one base (a LEFT site at start + 60), and the odd ones get `50S 100M` (a RIGHT site at their own start + 1, which faces the
LEFT site when 10 <= d).  The share of clipped records, the seed and the number of places that took are recorded.  No stage runs:
`bk_clip_loci` works on the attached table without a calls context, with `--support` 1 so that every locus is returned.  After a
warm-up call it is repeated `--reps` times; each repetition gives the HIP-event times of the scopes `clip_loci` (the whole, which holds
the host's three reads of a count: the device waits for them), `clip_loci_records` (the record pass) and `clip_loci_calls`, and the wall
clock around the call from Python.  The yardsticks are timed in the same process, in every repetition: the record pass of
`bk_cigar_gaps` (`cigar_gaps_records`) and the tile pass of `bk_window_context` (`window_context_tiles`).  Scopes are reported as
fractions of 8 TB/s by the library's own byte model (bk_timing_touched).  The dispatch count is worked out from the counts, as the
host code launches: it is not measured.  Nothing is compared against a target: the tool only records.

    python tools/gpu_cliploci_bench.py [--records 620000000] [--loci 77500] [--reads 8] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCOPES = ("clip_loci", "clip_loci_records", "clip_loci_calls")
YARDSTICKS = ("cigar_gaps_records", "window_context_tiles")
HBM_BYTES_PER_S = 8e12


def add_clips(cols, loci, reads):
    """rebuilds cigar_off / cigar in place of the old ones; returns (clipped records, places that took)"""
    import torch
    n, dev = cols["n"], cols["tid"].device
    off = cols["cigar_off"].to(torch.int64)
    aux = cols["aux_off"].to(torch.int64)
    nops = off[1:] - off[:-1]
    stride = max(reads, n // max(loci, 1))
    first = torch.arange(0, n - reads, stride, device=dev, dtype=torch.int64)[:loci]
    lane = torch.arange(reads, device=dev, dtype=torch.int64)
    idx = (first[:, None] + lane[None, :]).reshape(-1)
    odd = (lane[None, :].expand(len(first), reads).reshape(-1) & 1) == 1
    head = first.repeat_interleave(reads)
    old = cols["cigar"].to(torch.int64)
    d = cols["pos"][idx].to(torch.int64) - cols["pos"][head].to(torch.int64)
    ok = (nops[idx] == 1) & (old[off[idx]] == (150 << 4)) & (cols["tid"][idx] == cols["tid"][head]) & (cols["tid"][idx] >= 0) & (d >= 0) & (d <= 50) & (aux[idx + 1] == aux[idx])
    idx, d, odd = idx[ok], d[ok], odd[ok]
    new_nops = nops.clone()
    new_nops[idx] = 2
    new_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(new_nops, 0, out=new_off[1:])
    n_words, new_words = cols["n_cigar_words"], int(new_off[-1].item())
    shift = torch.repeat_interleave(new_off[:-1] - off[:-1], nops)
    cigar = torch.zeros(max(new_words, 1), dtype=torch.int64, device=dev)
    cigar[torch.arange(n_words, device=dev, dtype=torch.int64) + shift] = old[:n_words]
    b = new_off[idx]
    cigar[b] = torch.where(odd, torch.full_like(d, (50 << 4) | 4), (60 - d) << 4)
    cigar[b + 1] = torch.where(odd, torch.full_like(d, 100 << 4), ((90 + d) << 4) | 4)
    cols["cigar_off"] = new_off.to(torch.int32)
    cols["cigar"] = cigar.to(torch.int32)
    cols["n_cigar_words"] = new_words
    return int(idx.numel()), int(torch.unique(head[ok]).numel())


def dispatches(counts, prims, n_targets, longest):
    """the kernel launches of one call without a calls context, as cliploci.hip and prims.h queue them"""
    bits = lambda v: int(v).bit_length()  # noqa: E731
    scan = lambda n: 0 if n == 0 else 1 if n <= prims["SCAN_ONE_MAX"] else 3  # noqa: E731
    sort = lambda n, nbits: ((nbits + 7) // 8) * (2 + scan(256 * ((n + prims["RS_TILE"] - 1) // prims["RS_TILE"])))  # noqa: E731
    tiles, e, loci = (counts["records"] + 255) // 256, counts["events"] - counts["beyond"], counts["loci"]
    records = 1 + 2 * scan(tiles) + 1 + (1 if e else 0)
    if not e:
        return records, 0
    calls = 1 + sort(e, 64) + 1 + scan(e) + 1                            # qhash and the read ranks
    calls += 1 + sort(e, bits(longest) + bits(n_targets - 1) + 1) + 1    # (dir, tid, p) and the sorted copy
    calls += 1 + 3 * scan(e) + 2                                         # heads, scans, start lists
    calls += 1 + sort(e, bits(e) + bits(loci)) + 1 + scan(e)             # the distinct reads of a locus
    calls += 3 + 2 * scan(loci) + 1                                      # rows, facing, mutual; the two scans; the output
    return records, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=620_000_000)
    ap.add_argument("--loci", type=int, default=77_500)
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qual", type=int, default=20)
    ap.add_argument("--minclip", type=int, default=10)
    ap.add_argument("--tol", type=int, default=2)
    ap.add_argument("--pair", type=int, default=50)
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
    clipped, places = add_clips(cols, args.loci, args.reads)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    t = capi.Context(contigs, device=0)
    t.attach_device(abi.device_ptrs(cols), cols["n"], cols["n_cigar_words"], cols["n_aux_bytes"])
    params = (None, args.qual, args.minclip, args.tol, args.pair, args.support)
    gap_params = (args.qual, 20, 10, 2, 1)
    rows = t.clip_loci(*params)  # warm-up: the call's buffers are allocated here
    counts = t.clip_locus_counts()
    t.cigar_gaps(*gap_params)
    windows = np.zeros(1, abi.COV_WINDOW)
    windows["tid"], windows["beg"], windows["end"] = 0, 1000, 2000
    t.window_context(windows, args.qual)
    wall, event, model = [], {s: [] for s in SCOPES + YARDSTICKS}, {}
    t.timing_enable(True)
    for _ in range(args.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = t.clip_loci(*params)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert again.tobytes() == rows.tobytes()
        t.cigar_gaps(*gap_params)
        t.window_context(windows, args.qual)
        seen = {name: (ms, tb) for (name, ms, _), tb in zip(t.timing(), t.timing_touched())}  # (the scopes accumulate: the last of each)
        for s in event:
            event[s].append(seen[s][0])
            model[s] = int(seen[s][1])
    t.timing_enable(False)
    med = {s: float(np.median(v)) for s, v in event.items()}
    fraction = lambda s: round(model[s] / (med[s] * 1e-3) / HBM_BYTES_PER_S, 6) if med[s] > 0 else None  # noqa: E731
    d_records, d_calls = dispatches(counts, capi.prims_info(), len(contigs), max(l for _, l in contigs))
    out = {
        "what": "bk_clip_loci on a configs[1]-shaped synthetic table whose CIGAR columns were rebuilt with two-operation clipped records at planted facing sites; no stage ran, no calls context",
        "records": int(cols["n"]), "cigar_words": int(cols["n_cigar_words"]), "clipped_records": clipped, "clipped_share": round(clipped / max(1, int(cols["n"])), 8), "planted_places": places,
        "reads_per_place_asked": args.reads, "places_asked": args.loci, "seed": args.seed,
        "mapq_min": args.qual, "min_clip": args.minclip, "tol": args.tol, "pair_dist": args.pair, "min_reads": args.support, "reps": args.reps, "counts": counts,
        "returned_loci": int(len(rows)), "loci_with_3_reads": int((rows["n_reads"] >= 3).sum()), "most_rows_in_a_locus": int(rows["n_rows"].max()) if len(rows) else 0,
        "dispatches_worked_out": {"clip_loci_records": d_records, "clip_loci_calls": d_calls, "clip_loci": d_records + d_calls},
        "event_ms": {s: [round(x, 4) for x in v] for s, v in event.items()}, "event_ms_median": {s: round(v, 4) for s, v in med.items()},
        "wall_ms": [round(x, 3) for x in wall], "wall_ms_median": round(float(np.median(wall)), 3),
        "model_bytes": model, "fraction_of_8_tb_per_s": {s: fraction(s) for s in event},
        "records_pass_over_gaps_records_pass": round(med["clip_loci_records"] / med["cigar_gaps_records"], 4) if med["cigar_gaps_records"] > 0 else None,
        "expected_ratio_by_bytes": round(15 / 11, 4),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

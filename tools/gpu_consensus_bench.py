"""Measurement: what `bk_clip_consensus` costs at the bench shape.

The bench shape (configs[1], `-fast`; profiles/r14_unique_620M.json) has 126 618 voted calls and 2 025 888 split rows.  A synthetic
`bk_reads` table of that size is built on the host: one alignment per split row, clipped 40 (trailing, `60M40S`) or 60 bases
(leading, `60S40M`) exactly at one of the 2 x calls sites, which take the alignments in turn (eight each), and half as many
plain mates (`100M`, no event) as a pass over the file would bring along.  A tenth of the clipped bases differ from the site's
sequence.  After a warm-up call the consensus runs `--reps` times; each repetition gives the HIP-event time of the call's scope
(`consensus`: the three kernels, the scan and the read-back that sizes the list; the upload of the table is outside it), the
wall time of the whole call with the upload, and the bytes of the library's model (bk_timing_touched: CIGAR words and
ceil(min(c, max_len) / 2) bytes of SEQ per contribution among them).

    python tools/gpu_consensus_bench.py [--calls 126618] [--split-rows 2025888] [--max-len 64] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8e12  # bytes per second: the rate DESIGN.md measures every stage against


def make_table(calls, split_rows, seed):
    """(reads, sites, clipped alignments): the synthetic bk_reads table and its 2 x calls sites"""
    import numpy as np
    from breakid_amd import abi

    rng = np.random.default_rng(seed)
    n_sites, n_clip = 2 * calls, split_rows
    n = n_clip + n_clip // 2
    sites = np.zeros(n_sites, abi.CLIP_SITE)
    sites["tid"] = np.arange(n_sites) % 24
    sites["pos"] = 10_000 + (np.arange(n_sites) // 24) * 1_000
    sites["dir"] = np.arange(n_sites) & 1
    truth = rng.integers(0, 4, (n_sites, 60))
    is_clip = np.zeros(n, bool)
    is_clip[:n_clip] = True
    rng.shuffle(is_clip)  # (file order is by coordinate, not by site)
    ci = np.flatnonzero(is_clip)
    s = rng.permutation(n_clip) % n_sites  # the site of every clipped alignment
    r = sites["dir"][s] == 1
    clip = (1 << np.where(rng.random((n_clip, 60)) < 0.1, rng.integers(0, 4, (n_clip, 60)), truth[s])).astype(np.uint8)
    codes = np.full((n, 100), 1, np.uint8)  # aligned bases: A
    codes[ci[~r], 60:] = clip[~r, :40]  # a LEFT site's reads end in its first 40 columns,
    codes[ci[r], :60] = clip[r, ::-1]   # a RIGHT site's reads begin with its 60 columns, reversed
    words = np.zeros((n, 2), np.uint32)
    words[:, 0] = (100 << 4) | 0
    words[ci[~r]] = ((60 << 4) | 0, (40 << 4) | 4)
    words[ci[r]] = ((60 << 4) | 4, (40 << 4) | 0)
    n_words = np.where(is_clip, 2, 1)
    tid = rng.integers(0, 24, n)
    pos = rng.integers(0, 1_000_000, n)
    tid[ci] = sites["tid"][s]
    pos[ci] = np.where(r, sites["pos"][s].astype(np.int64) - 1, sites["pos"][s].astype(np.int64) - 60)
    reads = {
        "tid": tid.astype(np.int32), "pos": pos.astype(np.int32), "flag": np.zeros(n, np.uint16), "mapq": np.full(n, 60, np.uint8), "l_seq": np.full(n, 100, np.uint32),
        "cigar_off": np.concatenate([[0], np.cumsum(n_words)]).astype(np.uint32), "cigar": words.reshape(-1)[(np.arange(2 * n) & 1) < np.repeat(n_words, 2)],
        "seq_off": np.arange(n + 1, dtype=np.uint64) * np.uint64(50), "seq": ((codes[:, 0::2] << 4) | codes[:, 1::2]).reshape(-1),
    }
    return reads, sites, n_clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=126_618)
    ap.add_argument("--split-rows", type=int, default=2_025_888)
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--qual", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    from breakid_amd import capi

    reads, sites, n_clip = make_table(args.calls, args.split_rows, args.seed)
    n_sites, n = len(sites), len(reads["tid"])
    t = capi.Context([("chr%d" % (i + 1), 250_000_000) for i in range(24)], device=0)
    call = lambda: t.clip_consensus(reads, sites, args.qual, 10, args.max_len, 2)  # noqa: E731
    rows, bases, depth = call()  # warm-up: the call's buffers are allocated here
    assert int(rows["n_reads"].sum()) == n_clip and (rows["len"] == np.where(sites["dir"] == 1, min(60, args.max_len), min(40, args.max_len))).all()
    ev, wall, by, tb = [], [], 0, 0
    t.timing_enable(True)
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, by, tb = [(ms, by, tb) for (nm, ms, by), tb in zip(t.timing(), t.timing_touched()) if nm == "consensus"][-1]
        ev.append(ms)
    t.timing_enable(False)
    med = float(np.median(ev))
    out = {
        "what": "bk_clip_consensus of a synthetic bk_reads table sized from the calls and split rows of configs[1] after one -fast step",
        "calls": args.calls, "sites": n_sites, "reads": n, "clipped_reads": n_clip, "max_len": args.max_len, "min_depth": 2, "mapq_min": args.qual, "reps": args.reps,
        "table_bytes": int(sum(v.nbytes for v in reads.values())), "agree": round(float(rows["match"].sum()) / float(rows["total"].sum()), 4),
        "event_ms": [round(x, 4) for x in ev], "event_ms_median": round(med, 4), "wall_ms_with_upload": [round(x, 2) for x in wall],
        "bytes": int(by), "model_bytes": int(tb), "model_gbps": round(tb / med / 1e6, 1), "frac_of_hbm_peak": round(tb / (med * 1e-3) / HBM_PEAK, 4),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    t.close()


if __name__ == "__main__":
    main()

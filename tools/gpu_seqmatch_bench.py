"""Measurement: what `bk_sequence_match` costs at the shape `-cliploci` leaves on the bench table.

One query per locus of the `-cliploci` bench shape (tools/gpu_cliploci_bench.py: 351 516 loci), 64 bases each.  A third of them are
cut from the panel, substituted at a rate drawn per query between 0 and `--divergence`, every other one reverse-complemented; the rest
are drawn bases.  The panel is drawn too: `--seqs` sequences of 300 to 6000 bases, each with a poly-A tail of 10 to 30.  No record
table and no stage: the call needs neither.  After a warm-up call it is repeated `--reps` times; each repetition gives the HIP-event
times of the scopes `sequence_match` (the whole, which holds the host's one read of the k-mer count: the device waits for it),
`sequence_match_index` and `sequence_match_probes`, and the wall clock around the call from Python (uploads and the copy of the rows
included).  The same is then done with drawn queries only, which meet the index but start next to no extension: the difference is
what the extension walks cost.  Scopes are reported as fractions of 8 TB/s by the library's own byte model (bk_timing_touched).  The
dispatch count of the index is worked out as the host code launches it: it is not measured.  Nothing is compared against a target:
the tool only records.

    python tools/gpu_seqmatch_bench.py [--probes 351516] [--qlen 64] [--seqs 50] [--seed 12] [--reps 7] [--out profiles/FILE.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCOPES = ("sequence_match", "sequence_match_index", "sequence_match_probes")
HBM_BYTES_PER_S = 8e12
ACGT = np.frombuffer(b"ACGT", np.uint8)


def draw_panel(rng, n_seqs):
    seqs = []
    for _ in range(n_seqs):
        body = rng.integers(0, 4, int(rng.integers(300, 6001)))
        seqs.append(np.concatenate([body, np.zeros(int(rng.integers(10, 31)), np.int64)]))  # (code 0 is A)
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return off, np.concatenate(seqs)


def draw_queries(rng, off, codes, n, qlen, share, divergence):
    """uint8 [n, qlen] ASCII; the first n * share rows are cut from the panel (then all rows are shuffled)"""
    q = rng.integers(0, 4, (n, qlen))
    n_cut = int(n * share)
    lens = np.diff(off.astype(np.int64))
    s = rng.integers(0, len(lens), n_cut)
    a = off[s].astype(np.int64) + (rng.random(n_cut) * (lens[s] - qlen + 1)).astype(np.int64)
    cut = codes[a[:, None] + np.arange(qlen)[None, :]]
    rate = rng.random(n_cut)[:, None] * divergence
    cut = np.where(rng.random((n_cut, qlen)) < rate, (cut + rng.integers(1, 4, (n_cut, qlen))) % 4, cut)
    flip = np.arange(n_cut) % 2 == 1
    cut[flip] = 3 - cut[flip][:, ::-1]
    q[:n_cut] = cut
    return np.ascontiguousarray(ACGT[q[rng.permutation(n)]])


def measure(t, abi, panel, probes, query, seed, reps):
    call = lambda: t.sequence_match(panel, probes, query, seed)  # noqa: E731
    got = call()
    ms = {k: [] for k in SCOPES}
    wall, touched = [], {}
    for _ in range(reps):
        t.timing_enable(True)
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        names = [nm for nm, _, _ in t.timing()]
        for (nm, v, _), tb in zip(t.timing(), t.timing_touched()):
            if nm in ms:
                ms[nm].append(v)
                touched[nm] = int(tb)
        assert names == list(SCOPES), names
    out = {"found": int(got["found"].sum()), "seeds": int(got["n_seeds"].astype(np.int64).sum()), "wall_ms": summary(wall)}
    for k in SCOPES:
        out[k] = dict(summary(ms[k]), touched_bytes=touched[k], of_8_TBps=touched[k] / (float(np.median(ms[k])) * 1e-3) / HBM_BYTES_PER_S)
    return out


def scan_dispatches(n):
    return 1 if n <= 32768 else 3


def summary(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probes", type=int, default=351516)
    ap.add_argument("--qlen", type=int, default=64)
    ap.add_argument("--seqs", type=int, default=50)
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--share", type=float, default=1 / 3)
    ap.add_argument("--divergence", type=float, default=0.15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rng", type=int, default=29)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from breakid_amd import abi, capi
    rng = np.random.default_rng(a.rng)
    off, codes = draw_panel(rng, a.seqs)
    panel = (off, np.ascontiguousarray(ACGT[codes]))
    probes = np.zeros(a.probes, abi.SEQ_PROBE)
    probes["qlen"] = a.qlen
    mixed = draw_queries(rng, off, codes, a.probes, a.qlen, a.share, a.divergence)
    drawn = draw_queries(rng, off, codes, a.probes, a.qlen, 0.0, 0.0)
    t = capi.Context([("chr1", 1000)])
    kmers = int(sum(max(0, int(n) - a.seed + 1) for n in np.diff(off.astype(np.int64))))
    passes = (2 * a.seed + 7) // 8
    out = {"what": "bk_sequence_match of one 64-base query per locus of the -cliploci bench shape against a drawn panel with poly-A tails",
           "probes": a.probes, "qlen": a.qlen, "seed": a.seed, "sequences": a.seqs, "panel_bases": int(off[-1]), "kmers": kmers, "share_cut": a.share, "divergence": a.divergence,
           "reps": a.reps, "rng": a.rng,
           # the index as the host launches it: codes and flags, their scan, the k-mers, then a histogram, its scan and a scatter per pass
           # (a scan of at most 32 768 entries is one dispatch, a longer one three)
           "index_dispatches": 2 + scan_dispatches(int(off[-1])) + passes * (2 + scan_dispatches(256 * ((kmers + 2047) // 2048))), "index_host_reads": 1,
           "mixed": measure(t, abi, panel, probes, mixed, a.seed, a.reps), "drawn_only": measure(t, abi, panel, probes, drawn, a.seed, a.reps)}
    t.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

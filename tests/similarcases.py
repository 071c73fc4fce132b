"""Shared cases of the locus-similarity tests (test_cpu_similar, test_gpu_similar): the numpy definition of bk_locus_similarity
(include/breakid_hip.h), vectorised over the pairs and over every diagonal of both orientations with one step per column of window A;
a brute force over every segment for small windows; and references built directly as nib-code arrays (homologycases.make_refseq)
with planted copies, contig ends and segment gaps."""
import numpy as np

from breakid_amd import abi
from tests import homologycases as hc

COLUMNS = ["Sim_Score", "Sim_Len", "Sim_Mism", "Sim_Run", "Sim_Strand", "Sim_Pos1", "Sim_Pos2"]


def as_pairs(rows):
    """abi.LOCUS_PAIR from [(tid_a, pos_a, tid_b, pos_b)]"""
    out = np.zeros(len(rows), abi.LOCUS_PAIR)
    for k, r in enumerate(rows):
        out[k] = tuple(r)
    return out


def windows(ref, pairs, flank):
    """(a, b0, b1) of the contract as indices into "ACGTN", each [n, L]"""
    R = int(flank)
    i = np.arange(2 * R + 1, dtype=np.int64)[None, :]
    ta, pa = pairs["tid_a"].astype(np.int64)[:, None], pairs["pos_a"].astype(np.int64)[:, None]
    tb, pb = pairs["tid_b"].astype(np.int64)[:, None], pairs["pos_b"].astype(np.int64)[:, None]
    a = hc.ref_codes(ref, ta, pa - R + i)
    b0 = hc.ref_codes(ref, tb, pb - R + i)
    b1 = hc.ref_codes(ref, tb, pb + R - i)
    return a, b0, np.where(b1 < 4, 3 - b1, b1)


def excluded_diagonal(pairs):
    """pos_a - pos_b where tid_a == tid_b, else a value no diagonal has"""
    return np.where(pairs["tid_a"] == pairs["tid_b"], pairs["pos_a"].astype(np.int64) - pairs["pos_b"].astype(np.int64), 1 << 40)


def _key(score, n, o, d, i0):
    """the contract's order (score, -n, -o, -|d|, [d >= 0], -i0) as one integer; every field is below 1024"""
    return ((((score * 1024 + (1023 - n)) * 2 + (1 - o)) * 1024 + (1023 - np.abs(d))) * 2 + (d >= 0)) * 1024 + (1023 - i0)


def _block(ref, pairs, flank, out):
    n, L = len(pairs), 2 * int(flank) + 1
    a, b0, b1 = windows(ref, pairs, flank)
    pad = np.full((n, 2, 3 * L), 4, np.int64)  # b_o[j] at column L + j, N around it
    pad[:, 0, L:2 * L], pad[:, 1, L:2 * L] = b0, b1
    d = np.arange(-(L - 1), L)
    o = np.arange(2)
    dead = (o[None, :, None] == 0) & (d[None, None, :] == excluded_diagonal(pairs)[:, None, None])  # [n, 2, D]
    shape = (n, 2, len(d))
    total, since, cur, run = (np.zeros(shape, np.int64) for _ in range(4))
    best_score, best_len, best_start = (np.zeros(shape, np.int64) for _ in range(3))
    for i in range(L):
        live = ((i + d >= 0) & (i + d < L))[None, None, :] & ~dead
        ai = a[:, i][:, None, None]
        match = live & (ai < 4) & (ai == pad[:, :, L + i + d])
        again = live & (total <= 0)
        total[again], since[again] = 0, 0
        total += np.where(live, np.where(match, 1, -2), 0)
        since += live
        cur = np.where(match, cur + 1, 0)
        run = np.maximum(run, cur)
        better = live & ((total > best_score) | ((total == best_score) & (total > 0) & (since < best_len)))
        best_score[better], best_len[better], best_start[better] = total[better], since[better], i + 1 - since[better]
    key = np.where(best_score > 0, _key(best_score, best_len, o[None, :, None], d[None, None, :], best_start), -1).reshape(n, -1)
    at = key.argmax(1)
    for k in range(n):
        if key[k, at[k]] < 0:
            continue
        oo, di = divmod(int(at[k]), len(d))
        s, ln = int(best_score[k, oo, di]), int(best_len[k, oo, di])
        out[k] = (s, ln, (ln - s) // 3, int(run[k].max()), int(d[di]), int(best_start[k, oo, di]), oo, 1)


def expected_sim(ref, pairs, flank, block=64):
    """the abi.LOCUS_SIM rows of bk_locus_similarity"""
    pairs = np.ascontiguousarray(pairs, abi.LOCUS_PAIR)
    out = np.zeros(len(pairs), abi.LOCUS_SIM)
    for s in range(0, len(pairs), block):
        _block(ref, pairs[s:s + block], flank, out[s:s + block])
    return out


def brute_force(ref, pair, flank):
    """one row, from every segment (o, d, i0, n) there is: for small windows"""
    pairs = as_pairs([pair])
    L = 2 * int(flank) + 1
    a, b0, b1 = (x[0] for x in windows(ref, pairs, flank))
    ex = int(excluded_diagonal(pairs)[0])
    best, run = None, 0
    for o, b in enumerate((b0, b1)):
        for d in range(-(L - 1), L):
            if o == 0 and d == ex:
                continue
            cols = [i for i in range(L) if 0 <= i + d < L]
            hit = {i: bool(a[i] < 4 and a[i] == b[i + d]) for i in cols}
            for i0 in cols:
                for n in range(1, cols[-1] - i0 + 2):
                    m = sum(hit[i] for i in range(i0, i0 + n))
                    if m == n:
                        run = max(run, n)
                    key = (m - 2 * (n - m), -n, -o, -abs(d), int(d >= 0), -i0)
                    if best is None or key > best[0]:
                        best = (key, (o, d, i0, n, n - m))
    row = np.zeros(1, abi.LOCUS_SIM)
    if best is not None and best[0][0] > 0:
        o, d, i0, n, mm = best[1]
        row[0] = (best[0][0], n, mm, run, d, i0, o, 1)
    return row[0]


def twin_fields(pair, flank, row):
    """the seven twin-file fields of one call: Sim_Score Sim_Len Sim_Mism Sim_Run Sim_Strand Sim_Pos1 Sim_Pos2"""
    if not int(row["found"]):
        return ["0", "0", "0", "0", ".", ".", "."]
    R, start, diag, n = int(flank), int(row["start"]), int(row["diag"]), int(row["len"])
    p1 = int(pair["pos_a"]) - R + start
    p2 = int(pair["pos_b"]) - R + start + diag if int(row["orient"]) == 0 else int(pair["pos_b"]) + R - (start + diag + n - 1)
    return [str(int(row["score"])), str(n), str(int(row["mism"])), str(int(row["run"])), "-" if int(row["orient"]) else "+", str(p1), str(p2)]


# ---- references as nib-code arrays ----------------------------------------------------------------------------------------------------
COMP = np.asarray([3, 2, 1, 0, 4], np.int64)  # on indices into "ACGTN"


def codes_to_ref(contigs):
    """a bk_refseq table of whole contigs from [an array of indices into "ACGTN"], tid = its place in the list"""
    return hc.make_refseq([(t, 0, hc.NIB_OF[np.asarray(c, np.int64)]) for t, c in enumerate(contigs)])


def plant(contig_a, at_a, contig_b, at_b, n, reverse, subs=(), ns=()):
    """copy n bases of contig_a from the 0-based at_a into contig_b at at_b, reverse-complemented if asked; then substitute the copy's
    bases at the offsets `subs` (each by the next base) and set those at `ns` to N.  Returns the copy as it lies in contig_b."""
    src = np.asarray(contig_a[at_a:at_a + n], np.int64).copy()
    copy = COMP[src][::-1] if reverse else src
    copy = copy.copy()
    for x in subs:
        copy[x] = (copy[x] + 1) % 4 if copy[x] < 4 else 0
    for x in ns:
        copy[x] = 4
    contig_b[at_b:at_b + n] = copy
    return copy


_CASES = {}


def random_case(flank, n_pairs, seed=None):
    """(ref, pairs, planted) at one flank, computed once: every pair has two random contigs of 2 L + 40 bases of its own; half of
    the pairs have a stretch of window A copied into window B (forward or reverse-complemented, at a random offset, 0 to 4
    substitutions, now and then an N), a tenth have a window over a contig end, another tenth contigs in two segments with a gap of
    seven bases in the middle.  planted[k]: pair k has a copy, and the copy does not lie over a gap."""
    key = (flank, n_pairs)
    if key in _CASES:
        return _CASES[key]
    R = int(flank)
    L = 2 * R + 1
    rng = np.random.default_rng(5000 + R if seed is None else seed)
    size = 2 * L + 40
    contigs, rows, planted = [], [], []
    for k in range(n_pairs):
        a = rng.integers(0, 4, size)
        b = rng.integers(0, 4, size)
        pa, pb = int(rng.integers(R + 10, size - R - 10)), int(rng.integers(R + 10, size - R - 10))  # 1-based centres, windows inside
        if k % 10 == 9:  # a window that runs over a contig end
            pa = int(rng.choice([rng.integers(1, R + 1), size - rng.integers(0, R)]))
            pb = int(rng.choice([rng.integers(1, R + 1), size - rng.integers(0, R)]))
        want = False
        if k % 2 == 0 and L >= 3:
            n = int(rng.integers(min(L, 12) // 2 + 1, max(min(L, 12) // 2 + 2, (3 * L) // 4)))
            n = min(n, L)
            ia, ib = int(rng.integers(0, L - n + 1)), int(rng.integers(0, L - n + 1))  # offsets into the two windows
            sa, sb = pa - 1 - R + ia, pb - 1 - R + ib  # 0-based in the contigs
            if sa >= 0 and sb >= 0 and sa + n <= size and sb + n <= size:
                subs = sorted(set(int(x) for x in rng.integers(0, n, int(rng.integers(0, 5))))) if n >= 20 else []
                ns = [int(rng.integers(0, n))] if k % 8 == 0 and n >= 20 else []
                plant(a, sa, b, sb, n, reverse=bool((k // 2) % 2), subs=subs, ns=ns)
                cut = size // 2  # (the gap of the contigs that have one: see below)
                want = k % 10 != 4 or (not (sa < cut + 7 and sa + n > cut) and not (sb < cut + 7 and sb + n > cut))
        contigs += [a, b]
        rows.append((2 * k, pa, 2 * k + 1, pb))
        planted.append(want)
    segs = []
    for t, c in enumerate(contigs):
        nib = hc.NIB_OF[np.asarray(c, np.int64)]
        if (t // 2) % 10 == 4:  # two segments with a gap between them, the second on an odd start
            cut = size // 2
            segs += [(t, 0, nib[:cut]), (t, cut + 7, nib[cut + 7:])]
        else:
            segs.append((t, 0, nib))
    _CASES[key] = (hc.make_refseq(segs), as_pairs(rows), np.asarray(planted))
    return _CASES[key]

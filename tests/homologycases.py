"""Shared cases of the junction-fit tests (test_cpu_homology, test_gpu_homology): the numpy definition of bk_junction_fit
(include/breakid_hip.h), the seeded genome of consensuscases with a small dict of patched positions, a nib writer, a bk_refseq
packer, and the designed tables: the nine loci of consensuscases.designed(), an insertion locus, a microhomology locus, repeat
references where many placements tie, and reference edges."""
import os
import re
import struct

import numpy as np

from breakid_amd import abi
from tests import callcases as cc
from tests import consensuscases as kc

LEFT, RIGHT = 0, 1
MAX_SHIFT, MAX_INS, MAX_HOM = 32, 32, 32  # the command line's defaults
NIB_OF = np.asarray([2, 1, 3, 0, 4], np.uint8)  # index into "ACGTN" -> nib code (T=0 C=1 A=2 G=3, 4 = N)
IDX_OF_NIB = np.asarray([3, 1, 0, 2, 4, 4, 4, 4] * 2, np.int64)  # nib code -> index into "ACGTN"; bit 3 is the soft-mask
ASCII = np.full(256, 4, np.int64)
for _i, _c in enumerate(b"ACGT"):
    ASCII[_c] = _i


# ---- the reference: a genome, nib files, bk_refseq tables -----------------------------------------------------------------------
class Genome:
    """consensuscases.base_index on contigs of the given lengths, with patches {(tid, 1-based pos): one of 'ACGTN'}"""

    def __init__(self, lengths, patches=None):
        self.lengths = list(lengths)
        self.patches = dict(patches or {})

    def codes(self, tid, pos1):
        """index into "ACGTN" at the 1-based positions pos1 (an array) of contig tid; N outside the contig"""
        p = np.asarray(pos1, np.int64)
        if tid < 0 or tid >= len(self.lengths):
            return np.full(p.shape, 4, np.int64)
        inside = (p >= 1) & (p <= self.lengths[tid])
        out = np.where(inside, kc.base_index(tid, np.where(inside, p - 1, 0)), 4)
        for (t, q), b in self.patches.items():
            if t == tid:
                out[(p == q) & inside] = "ACGTN".index(b)
        return out

    def text(self, tid, first, last):
        """the bases first .. last (1-based, inclusive) as text"""
        return "".join("ACGTN"[c] for c in self.codes(tid, np.arange(first, last + 1)))

    def nibbles(self, tid, start0, n):
        return NIB_OF[self.codes(tid, start0 + 1 + np.arange(n))]

    def write_nib(self, path, tid):
        n = self.lengths[tid]
        with open(path, "wb") as f:
            f.write(struct.pack("<II", 0x6BE93D3A, n))
            f.write(pack_nibbles(self.nibbles(tid, 0, n)).tobytes())

    def refseq(self, windows):
        """a bk_refseq table (a dict of its columns) of the windows [(tid, 0-based start, len)], which must be sorted and disjoint"""
        return make_refseq([(t, s, self.nibbles(t, s, n)) for t, s, n in windows])


def pack_nibbles(nib):
    v = np.asarray(nib, np.uint8)
    if len(v) & 1:
        v = np.concatenate([v, np.zeros(1, np.uint8)])
    return ((v[0::2] << 4) | v[1::2]).astype(np.uint8)


def make_refseq(segs):
    """a bk_refseq table from [(tid, 0-based start, nib codes)]: every segment starts on a byte"""
    n = len(segs)
    r = {"tid": np.zeros(n, np.int32), "start": np.zeros(n, np.uint32), "len": np.zeros(n, np.uint32), "off": np.zeros(n + 1, np.uint64)}
    parts = []
    for g, (t, s, nib) in enumerate(segs):
        r["tid"][g], r["start"][g], r["len"][g] = t, s, len(nib)
        parts.append(pack_nibbles(nib))
        r["off"][g + 1] = r["off"][g] + np.uint64(len(parts[-1]))
    r["bases"] = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return r


def read_nib(path):
    """(nBases, the payload) of a nib file: the payload is a valid segment as it lies"""
    raw = open(path, "rb").read()
    magic, n = struct.unpack_from("<II", raw, 0)
    assert magic == 0x6BE93D3A
    return n, np.frombuffer(raw, np.uint8, (n + 1) // 2, 8)


def merged_windows(probes, radius, lengths):
    """the windows [pos - radius, pos + radius] around every probe position, clamped to the contig and merged where they touch:
    [(tid, 0-based start, len)] in ascending order, as the command line reads them"""
    spans = {}
    for p in probes:
        for t, q in ((int(p["tid_own"]), int(p["pos_own"])), (int(p["tid_mate"]), int(p["pos_mate"]))):
            if 0 <= t < len(lengths):
                a, b = max(1, q - radius), min(lengths[t], q + radius)
                if a <= b:
                    spans.setdefault(t, []).append((a, b))
    out = []
    for t in sorted(spans):
        cur = None
        for a, b in sorted(spans[t]):
            if cur and a <= cur[1] + 1:
                cur[1] = max(cur[1], b)
            else:
                cur = [a, b]
                out.append(cur)
                cur.append(t)
    return [(t, a - 1, b - a + 1) for a, b, t in out]


def ref_codes(ref, tid, pos1):
    """ref(t, p) of the contract as an index into "ACGTN", on arrays that broadcast"""
    tid, p0 = np.broadcast_arrays(np.asarray(tid, np.int64), np.asarray(pos1, np.int64) - 1)
    out = np.full(p0.shape, 4, np.int64)
    n = len(ref["tid"])
    if n == 0 or len(ref["bases"]) == 0:
        return out
    st, ln, off = ref["start"].astype(np.int64), ref["len"].astype(np.int64), ref["off"].astype(np.int64)
    stid = ref["tid"].astype(np.int64)
    ok = (tid >= 0) & (p0 >= 0)
    g = np.searchsorted((stid << 33) | st, (np.where(ok, tid, 0) << 33) | np.where(ok, p0, 0), "right") - 1
    gi = np.clip(g, 0, n - 1)
    i = p0 - st[gi]
    hit = ok & (g >= 0) & (stid[gi] == tid) & (i < ln[gi])
    byte = np.asarray(ref["bases"], np.int64)[np.where(hit, off[gi] + i // 2, 0)]
    nib = np.where(i & 1, byte & 15, byte >> 4)
    out[hit] = IDX_OF_NIB[nib[hit]]
    return out


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def walks(ref, p, max_len, max_shift, max_hom):
    """(M over the indices -(max_shift + max_hom) .. max_len + max_shift - 1, O over -max_hom .. max_len - 1) of the probes p"""
    S, H, L = max_shift, max_hom, max_len
    mi = np.arange(-(S + H), L + S)
    step = np.where(p["dir_mate"] == RIGHT, 1, -1).astype(np.int64)
    M = ref_codes(ref, p["tid_mate"].astype(np.int64)[:, None], p["pos_mate"].astype(np.int64)[:, None] + step[:, None] * mi[None, :])
    M = np.where((p["dir_own"] == p["dir_mate"])[:, None] & (M < 4), 3 - M, M)
    oi = np.arange(-H, L)
    po = p["pos_own"].astype(np.int64)[:, None]
    O = ref_codes(ref, p["tid_own"].astype(np.int64)[:, None], np.where((p["dir_own"] == LEFT)[:, None], po + 1 + oi[None, :], po - 1 - oi[None, :]))
    return M, O


def _fit_block(ref, p, query, out, L, S, I, H):
    n = len(p)
    qlen = p["qlen"].astype(np.int64)
    placed = (qlen >= 1) & (p["tid_own"] >= 0) & (p["tid_mate"] >= 0)
    col = np.arange(L)
    Q = np.where(col[None, :] < qlen[:, None], ASCII[query], 4)
    M, O = walks(ref, p, L, S, H)
    d = np.arange(-S - I, S + 1)  # the diagonals shift - ins
    Md = M[:, np.clip(col[None, :] + d[:, None] + (S + H), 0, M.shape[1] - 1)]  # [n, D, L]; (every entry a placement reads is unclipped)
    mm = ~((Q[:, None, :] < 4) & (Q[:, None, :] == Md)) & (col[None, :] < qlen[:, None])[:, None, :]
    suf = np.zeros((n, len(d), L + 1), np.int64)  # mismatches of a diagonal from column j on
    suf[:, :, :L] = np.cumsum(mm[:, :, ::-1], axis=2)[:, :, ::-1]
    ins, sh = np.arange(I + 1), np.arange(-S, S + 1)
    mism = suf[:, (sh[None, :] - ins[:, None] + S + I), np.minimum(ins, L)[:, None]]  # [n, I + 1, 2 S + 1]
    score = (qlen[:, None, None] - ins[None, :, None]) - 2 * mism
    valid = ins[None, :, None] <= np.minimum(I, qlen - 1)[:, None, None]
    rank = ins[:, None] * 1000 + np.abs(sh)[None, :] * 2 + (sh < 0)[None, :]  # the tie order: the smaller wins
    key = np.where(valid, score * 100000 - rank[None, :, :], -10 ** 12)
    best = key.reshape(n, -1).argmax(1)
    for k in np.flatnonzero(placed):
        bi, bs = divmod(int(best[k]), len(sh))
        s = int(sh[bs])
        r = out[k]
        r["shift"], r["ins"], r["aligned"], r["mism"], r["score"], r["placed"] = s, bi, qlen[k] - bi, mism[k, bi, bs], score[k, bi, bs], 1
        if bi == 0:
            f = 0
            while f < qlen[k] and Q[k, f] < 4 and Q[k, f] == O[k, H + f] == M[k, S + H + f + s]:
                f += 1
            b = 0
            while b < H and O[k, H - 1 - b] < 4 and O[k, H - 1 - b] == M[k, S + H + s - 1 - b]:
                b += 1
            r["hom_fwd"], r["hom_back"] = f, b


def expected_fit(ref, probes, query, max_len, max_shift=MAX_SHIFT, max_ins=MAX_INS, max_hom=MAX_HOM):
    """the abi.JUNCTION_FIT rows of bk_junction_fit; query: uint8 [n, max_len] (or flat), ASCII"""
    probes = np.ascontiguousarray(probes, abi.JUNCTION_PROBE)
    n = len(probes)
    query = np.asarray(query, np.uint8).reshape(n, max_len)
    out = np.zeros(n, abi.JUNCTION_FIT)
    for a in range(0, n, 64):
        _fit_block(ref, probes[a:a + 64], query[a:a + 64], out[a:a + 64], max_len, max_shift, max_ins, max_hom)
    return out


def as_probes(rows):
    """abi.JUNCTION_PROBE from [(tid_own, pos_own, dir_own, tid_mate, pos_mate, dir_mate, qlen)]"""
    out = np.zeros(len(rows), abi.JUNCTION_PROBE)
    for k, r in enumerate(rows):
        out[k] = tuple(r) + (0,)
    return out


def as_query(texts, max_len):
    q = np.zeros((len(texts), max_len), np.uint8)
    for k, t in enumerate(texts):
        q[k, :len(t)] = np.frombuffer(t.encode(), np.uint8)
    return q


def mate_text(genome, own_dir, tid_mate, pos_mate, dir_mate, first, n):
    """M[first .. first + n - 1] of a probe as text, from the genome itself"""
    i = first + np.arange(n)
    c = genome.codes(tid_mate, pos_mate + i if dir_mate == RIGHT else pos_mate - i)
    if own_dir == dir_mate:
        c = np.where(c < 4, 3 - c, c)
    return "".join("ACGTN"[x] for x in c)


def hom_seq(genome, tid, pos, d, fwd, back):
    """J_HomSeq: the own contig's bases over the homologous stretch, reference-forward"""
    if fwd + back == 0:
        return "."
    return genome.text(tid, pos - back + 1, pos + fwd) if d == LEFT else genome.text(tid, pos - fwd, pos + back - 1)


def side_fields(genome, probe, qtext, row):
    """the seven twin-file fields of one side"""
    if not int(row["placed"]):
        return ["."] * 7
    n = int(row["ins"])
    d = int(probe["dir_own"])
    ins = qtext[:n][::-1] if d == RIGHT else qtext[:n]
    return [str(int(row["shift"])), str(n), str(int(row["aligned"])), str(int(row["mism"])), str(int(row["hom_fwd"]) + int(row["hom_back"])),
            hom_seq(genome, int(probe["tid_own"]), int(probe["pos_own"]), d, int(row["hom_fwd"]), int(row["hom_back"])), ins or "."]


# ---- designed tables ------------------------------------------------------------------------------------------------------------------
LENGTHS = [ln for _, ln in cc.CONTIGS]
DIR = {"L": LEFT, "R": RIGHT}
INS_LOCUS = ("INS_x", 0, 1_850_000, "L", 1, 1_850_000, "R")
HOM_LOCUS = ("HOM_x", 2, 200_000, "L", 3, 200_000, "R")
INSERTED, INS_SHIFT = "GATTACC", 3
HOM_PATCHED = 5


def ins_locus_inserted():
    """the bases inserted at side A of INS_LOCUS: as long as INSERTED, each unlike the partner's base on the diagonal of the
    continuation (M[j - len + INS_SHIFT] under column j), so that no shorter insertion on that diagonal scores as well"""
    _, ta, bpa, da, tb, bpb, db = INS_LOCUS
    n = len(INSERTED)
    m = Genome(LENGTHS).codes(tb, bpb + INS_SHIFT - n + np.arange(n))  # (da != db: the walk runs forward and is not complemented)
    return "".join("ACGT"[(int(c) + 1 + j % 3) % 4] for j, c in enumerate(m))


def hom_patches():
    """the own contig behind the breakpoint of HOM_LOCUS's side A made equal to the mate walk, HOM_PATCHED bases long"""
    _, ta, bpa, _, tb, bpb, _ = HOM_LOCUS
    plain = Genome(LENGTHS)
    return {(ta, bpa + 1 + j): "ACGT"[int(plain.codes(tb, [bpb + j])[0])] for j in range(HOM_PATCHED)}


def genome():
    return Genome(LENGTHS, hom_patches())


def locus_probe(L, own_a, qlen):
    _, ta, bpa, da, tb, bpb, db = L
    a, b = (ta, bpa, DIR[da]), (tb, bpb, DIR[db])
    return (a + b if own_a else b + a) + (qlen,)


def designed_table():
    """(probes, query texts) of the 18 sides of consensuscases.designed(): the query of a side is its designed truth"""
    truth = kc.designed()["truth"]
    rows, texts = [], []
    for L in kc.ALL_LOCI:
        for own_a in (True, False):
            r = locus_probe(L, own_a, 0)
            t = truth[r[:3]]
            rows.append(r[:6] + (len(t),))
            texts.append(t)
    return as_probes(rows), texts


def insertion_query(g, last="C", n=40):
    """side A of the first locus with seven inserted bases and the mate walk from M[3] on"""
    r = locus_probe(cc.LOCI[0], True, n)
    ins = INSERTED[:-1] + last
    return r, ins + mate_text(g, r[2], r[3], r[4], r[5], INS_SHIFT, n - len(ins))


def repeat_ref(unit, n=600, tid=0):
    """one segment of `unit` repeated over the first n bases of contig tid"""
    text = (unit * (n // len(unit) + 1))[:n]
    return make_refseq([(tid, 0, NIB_OF[["ACGTN".index(c) for c in text]])]), text


def random_table(g, rng, n, max_len, qlen_max, near_edges=False):
    """(probes, query): n probes over all four direction pairs; the query is cut from the mate walk with a random shift, inserted
    bases, substitutions and N, so that the best placement is not the trivial one"""
    rows, q = [], np.zeros((n, max_len), np.uint8)
    for k in range(n):
        to, tm = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        if near_edges:
            po = int(rng.choice([rng.integers(1, 71), LENGTHS[to] - rng.integers(0, 70)]))
            pm = int(rng.choice([rng.integers(1, 71), LENGTHS[tm] - rng.integers(0, 70)]))
        else:
            po, pm = int(rng.integers(1000, LENGTHS[to] - 1000)), int(rng.integers(1000, LENGTHS[tm] - 1000))
        do, dm = k & 1, (k >> 1) & 1
        qlen = qlen_max if k % 5 else int(rng.integers(1, qlen_max + 1))
        shift = int(rng.integers(-70, 71)) if k % 3 else 0
        n_ins = min(int(rng.integers(0, 71)) if k % 4 == 0 else 0, qlen - 1)
        text = "".join("ACGT"[x] for x in rng.integers(0, 4, n_ins)) + mate_text(g, do, tm, pm, dm, shift, qlen - n_ins)
        b = np.frombuffer(text.encode(), np.uint8).copy()
        for j in rng.integers(0, qlen, int(rng.integers(0, 4))):
            b[j] = b"ACGTN"[int(rng.integers(0, 5))]
        q[k, :qlen] = b
        rows.append((to, po, do, tm, pm, dm, qlen))
    return as_probes(rows), q


_TABLES = {}


def edge_table():
    """(ref, probes, query): segments that abut, a gap inside a walk, a contig without a segment, an odd segment length, soft-masked
    nibbles and the N codes 4..7; probes at the ends of the contigs; a mate with tid -1"""
    if "edge" not in _TABLES:
        g = Genome(LENGTHS, {(0, 520): "N", (1, 33): "N"})
        rng = np.random.default_rng(77)
        segs = []
        for t, s, n in [(0, 0, 301), (0, 301, 99), (0, 400, 64), (0, 480, 261), (0, LENGTHS[0] - 333, 333), (1, 0, 777), (1, LENGTHS[1] - 150, 150), (3, 10, 1), (3, 11, 500)]:
            nib = g.nibbles(t, s, n).copy()
            hit = rng.random(n) < 0.02
            nib[hit] = rng.integers(4, 8, int(hit.sum()))  # N, in every code it has
            nib[rng.random(n) < 0.3] |= 8  # soft-masked, N among them
            segs.append((t, s, nib))
        ref = make_refseq(segs)
        rows = []
        for k in range(96):
            to, tm = int(rng.choice([0, 1, 2, 3])), int(rng.choice([0, 1, 3]))
            po = int(rng.choice([rng.integers(1, 71), rng.integers(380, 500), LENGTHS[to] - rng.integers(0, 70)]))
            pm = int(rng.choice([rng.integers(1, 71), rng.integers(380, 500), LENGTHS[tm] - rng.integers(0, 70)]))
            rows.append((to, po, k & 1, tm, pm, (k >> 1) & 1, int(rng.integers(1, 101))))
        rows += [(0, 450, 0, -1, 450, 1, 50), (-1, 450, 0, 0, 450, 1, 50), (0, 450, 0, 0, 450, 1, 0), (0, 1, 1, 0, 1, 0, 100), (0, 0, 0, 0, 0, 1, 100)]
        probes = as_probes(rows)
        # queries: what the table itself holds at the mate walk (N where it has none), so that most columns match
        M, _ = walks(ref, probes, 100, 0, 0)
        query = np.frombuffer(b"ACGTN", np.uint8)[M]
        _TABLES["edge"] = (ref, probes, np.ascontiguousarray(query))
    return _TABLES["edge"]


# ---- the designed BAM with the two extra loci --------------------------------------------------------------------------------------
_PLUS = {}


def designed_plus():
    """{"ds", "codes"}: callcases.designed_tumor with INS_LOCUS and HOM_LOCUS behind its own loci and real bases: the clip of every
    split read is the partner locus; at side A of INS_LOCUS it is ins_locus_inserted() and then the partner from M[INS_SHIFT] on"""
    if _PLUS:
        return _PLUS
    loci = list(cc.LOCI) + [INS_LOCUS, HOM_LOCUS]
    ds = cc.designed_tumor(loci=loci)
    by_name = {L[0]: L for L in loci + [kc.ALL_LOCI[-1]]}
    codes = {}
    for r in ds.recs:
        m = re.match(r"(\w+)S_(\d+)$", r.qname)
        if not (m and m.group(1) in by_name and r.sa):
            codes[id(r)] = kc.record_codes(r)
            continue
        name, ta, bpa, da, tb, bpb, db = by_name[m.group(1)]
        own_a = not r.flag & 0x100
        (t, bp, d), (t2, bp2, d2) = ((ta, bpa, da), (tb, bpb, db)) if own_a else ((tb, bpb, db), (ta, bpa, da))
        words = [w for w in kc.bamio.parse_cigar(r.cigar) if (w & 15) != kc.OP_H]
        c = (words[-1] if d == "L" else words[0]) >> 4
        clip = kc.partner_codes(d, t2, bp2, d2, c + INS_SHIFT)
        if name == INS_LOCUS[0] and own_a:
            clip = np.concatenate([np.asarray([kc.CODE[x] for x in ins_locus_inserted()], np.uint8), clip[INS_SHIFT:]])
        clip = clip[:c]
        codes[id(r)] = kc.record_codes(r, trail=clip) if d == "L" else kc.record_codes(r, lead=clip[::-1])
    _PLUS.update(ds=ds, codes=codes)
    return _PLUS


def write_plus_bam(path):
    d = designed_plus()

    def gen():
        for r in d["ds"].recs:
            aux = ([("SA", r.sa)] if r.sa else []) + ([("OC", r.oc)] if r.oc else [])
            c = d["codes"][id(r)]
            yield kc.bamio.encode_record(r.qname, r.flag, r.tid, r.pos, r.mapq, kc.bamio.parse_cigar(r.cigar), r.mtid, r.mpos, r.isize, aux, seq=bytes(kc.pack_codes(c)),
                                         qual=b"\x1e" * len(c))
    kc.bamio.write_bam(path, d["ds"].contigs, gen())


def plus_reads():
    d = designed_plus()
    return kc.make_reads([(r.tid, r.pos, r.flag, r.mapq, r.cigar, d["codes"][id(r)]) for r in d["ds"].recs])


def write_nib_dir(nib_dir, g, skip=()):
    """the genome's nib files over those synth.write_side_files wrote; the contigs in `skip` lose theirs"""
    for tid, (name, _) in enumerate(cc.CONTIGS):
        path = os.path.join(nib_dir, "hg19_%s.nib" % name)
        if tid in skip:
            if os.path.exists(path):
                os.remove(path)
        else:
            g.write_nib(path, tid)


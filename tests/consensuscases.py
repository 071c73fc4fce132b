"""Shared cases of the junction-consensus tests (test_cpu_consensus, test_gpu_consensus): the numpy / Python definition of
bk_clip_consensus (include/breakid_hip.h) over a bk_reads table, a seeded genome, the designed BAM (callcases.designed_tumor with
real bases: the clipped bases of every designed split read are the partner locus, so each side's truth is known without the
model, plus the designed variations) and numpy-only tables."""
import re
import struct

import numpy as np

from breakid_amd import abi, bamio, synth
from tests import callcases as cc

LEFT, RIGHT = 0, 1
NEVER = 0x4 | 0x200 | 0x400
OP_S, OP_H = 4, 5
REF_OPS, QUERY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)
CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "R": 5}
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}
MIN_CLIP, MAX_LEN, MIN_DEPTH = 10, 64, 2  # the command line's defaults


# ---- the definition -----------------------------------------------------------------------------------------------------------
def read_codes(reads, i):
    """the l_seq 4-bit codes of read i"""
    n = int(reads["l_seq"][i])
    o = int(reads["seq_off"][i])
    b = np.asarray(reads["seq"][o:o + (n + 1) // 2], np.uint8)
    return np.stack([b >> 4, b & 15], 1).reshape(-1)[:n]


def read_events(reads, i, mapq_min, min_clip):
    """[(tid, p, dir, clipped codes counted away from the junction)] of alignment i: the events bk_clip_support defines, on an
    alignment that is eligible for the consensus"""
    tid, flag, l_seq = int(reads["tid"][i]), int(reads["flag"][i]), int(reads["l_seq"][i])
    if tid < 0 or flag & NEVER or int(reads["mapq"][i]) < mapq_min or l_seq == 0:
        return []
    words = [int(w) for w in reads["cigar"][int(reads["cigar_off"][i]):int(reads["cigar_off"][i + 1])]]
    ops = [(w & 15, w >> 4) for w in words]
    reflen = sum(n for op, n in ops if op in REF_OPS)
    if reflen <= 0 or sum(n for op, n in ops if op in QUERY_OPS) != l_seq:
        return []
    body = [x for x in ops if x[0] != OP_H]
    codes = read_codes(reads, i)
    pos, out = int(reads["pos"][i]), []
    if body and body[0][0] == OP_S and body[0][1] >= min_clip:
        c = body[0][1]
        out.append((tid, pos + 1, RIGHT, codes[:c][::-1]))
    if body and body[-1][0] == OP_S and body[-1][1] >= min_clip:
        c = body[-1][1]
        out.append((tid, pos + reflen, LEFT, codes[l_seq - c:]))
    return out


def expected_consensus(reads, sites, mapq_min, min_clip, max_len, min_depth):
    """(rows, bases, depth) of bk_clip_consensus: abi.CONSENSUS per site, uint8 and uint32 [n_sites, max_len]"""
    sites = np.ascontiguousarray(sites, abi.CLIP_SITE)
    at = {}
    for k, s in enumerate(sites):
        assert int(s["tol"]) == 0
        if s["tid"] >= 0:
            at.setdefault((int(s["tid"]), int(s["pos"]), int(s["dir"])), []).append(k)
    counts = np.zeros((len(sites), max_len, 16), np.int64)
    n_reads = np.zeros(len(sites), np.int64)
    off = np.asarray(reads["cigar_off"], np.int64)
    cig = np.asarray(reads["cigar"], np.int64)
    has_s = np.zeros(len(reads["tid"]), bool)  # (only a read with an S op can have an event)
    if len(cig):
        s_at = np.concatenate([[0], np.cumsum((cig[:off[-1]] & 15) == OP_S)])
        has_s = s_at[off[1:]] > s_at[off[:-1]]
    for i in np.flatnonzero(has_s):
        for tid, p, d, codes in read_events(reads, int(i), mapq_min, min_clip):
            for k in at.get((tid, p, d), ()):
                n_reads[k] += 1
                m = min(len(codes), max_len)
                counts[k, np.arange(m), codes[:m]] += 1
    rows = np.zeros(len(sites), abi.CONSENSUS)
    bases = np.zeros((len(sites), max_len), np.uint8)
    depth = counts.sum(2).astype(np.uint32)
    for k in range(len(sites)):
        rows[k]["n_reads"] = n_reads[k]
        for j in range(max_len):
            if depth[k, j] < min_depth:
                continue
            four = [int(counts[k, j, c]) for c in (1, 2, 4, 8)]
            w = max(four)
            bases[k, j] = ord("N") if w == 0 else ord("ACGT"[four.index(w)])  # index(): the first, so the smaller base, on a tie
            rows[k]["len"] += 1
            rows[k]["match"] += w
            rows[k]["total"] += int(depth[k, j])
    return rows, bases, depth


def check_invariants(rows, bases, depth, max_len):
    d = depth.astype(np.int64)
    assert (np.diff(d, axis=1) <= 0).all()  # depth does not increase with j
    assert (rows["match"] <= rows["total"]).all() and (rows["len"] <= max_len).all()
    assert (d[:, 0] == rows["n_reads"]).all()  # every event has at least one column
    for k in range(len(rows)):
        n = int(rows[k]["len"])
        assert (bases[k, n:] == 0).all() and all(chr(b) in "ACGTN" for b in bases[k, :n])
        assert int(rows[k]["total"]) == int(d[k, :n].sum())


def as_sites(sites):
    out = np.zeros(len(sites), abi.CLIP_SITE)
    for k, s in enumerate(sites):
        out[k] = tuple(s)
    return out


def side_text(row, bases_k, d):
    """the four twin-file fields of one side: Cons_N, Cons_Len, Cons_Agree, Cons_Seq"""
    n = int(row["len"])
    seq = bytes(bases_k[:n]).decode()
    if d == RIGHT:
        seq = seq[::-1]
    agree = "%.3f" % (int(row["match"]) / int(row["total"])) if row["total"] else "."
    return [str(int(row["n_reads"])), str(n), agree, seq or "."]


# ---- reads tables ---------------------------------------------------------------------------------------------------------------
def pack_codes(codes):
    c = np.asarray(codes, np.uint8)
    if len(c) & 1:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)


def make_reads(items):
    """a bk_reads table (dict of abi.READS_COLS, without `key`) from [(tid, pos, flag, mapq, cigar text, codes)]"""
    n = len(items)
    t = {"tid": np.zeros(n, np.int32), "pos": np.zeros(n, np.int32), "flag": np.zeros(n, np.uint16), "mapq": np.zeros(n, np.uint8), "l_seq": np.zeros(n, np.uint32),
         "cigar_off": np.zeros(n + 1, np.uint32), "seq_off": np.zeros(n + 1, np.uint64)}
    cig, seq = [], []
    for i, (tid, pos, flag, mapq, cigar, codes) in enumerate(items):
        t["tid"][i], t["pos"][i], t["flag"][i], t["mapq"][i], t["l_seq"][i] = tid, pos, flag, mapq, len(codes)
        cig += bamio.parse_cigar(cigar)
        t["cigar_off"][i + 1] = len(cig)
        seq.append(pack_codes(codes))
        t["seq_off"][i + 1] = t["seq_off"][i] + np.uint64(len(seq[-1]))
    t["cigar"] = np.asarray(cig, np.uint32)
    t["seq"] = np.concatenate(seq) if seq else np.zeros(0, np.uint8)
    return t


def permuted(reads, perm):
    """the table with its rows in the order perm (CIGAR words and bases repacked)"""
    out = {k: np.ascontiguousarray(np.asarray(reads[k])[perm]) for k in ("tid", "pos", "flag", "mapq", "l_seq") + (("key",) if "key" in reads else ())}
    for blob, off, dt in (("cigar", "cigar_off", np.uint32), ("seq", "seq_off", np.uint64)):
        o = np.asarray(reads[off], np.int64)
        parts = [np.asarray(reads[blob])[o[i]:o[i + 1]] for i in perm]
        out[blob] = np.concatenate(parts) if parts else np.zeros(0, np.asarray(reads[blob]).dtype)
        out[off] = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(dt)
    return out


def reads_of_bam(path):
    """(every record of the file as a bk_reads table, in file order; their read names)"""
    _, recs = bamio.read_records(path)
    n = len(recs)
    t = {"tid": np.zeros(n, np.int32), "pos": np.zeros(n, np.int32), "flag": np.zeros(n, np.uint16), "mapq": np.zeros(n, np.uint8), "l_seq": np.zeros(n, np.uint32),
         "cigar_off": np.zeros(n + 1, np.uint32), "seq_off": np.zeros(n + 1, np.uint64)}
    cig, seq, names = [], [], []
    for i, r in enumerate(recs):
        tid, pos, l_name, mapq, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", r, 0)
        t["tid"][i], t["pos"][i], t["flag"][i], t["mapq"][i], t["l_seq"][i] = tid, pos, flag, mapq, l_seq
        names.append(r[32:32 + l_name].split(b"\0")[0])
        p = 32 + l_name
        cig.append(np.frombuffer(r, "<u4", n_cig, p))
        seq.append(np.frombuffer(r, np.uint8, (l_seq + 1) // 2, p + 4 * n_cig))
        t["cigar_off"][i + 1] = t["cigar_off"][i] + n_cig
        t["seq_off"][i + 1] = t["seq_off"][i] + np.uint64((l_seq + 1) // 2)
    t["cigar"] = np.concatenate(cig).astype(np.uint32) if cig else np.zeros(0, np.uint32)
    t["seq"] = np.concatenate(seq) if seq else np.zeros(0, np.uint8)
    return t, names


def selected(reads, names, keys):
    """what bk_bam_reads returns for abi.READ_KEY `keys`: the rows whose name a key selects, with the first such key"""
    rows, key = [], []
    for i, nm in enumerate(names):
        h, c = synth.fnv1a64(nm), synth.qname_check(nm)
        hit = [k for k in range(len(keys)) if int(keys[k]["qhash"]) == h and int(keys[k]["qcheck"]) in (0, c)]
        if hit:
            rows.append(i)
            key.append(hit[0])
    out = permuted(reads, rows)
    out["key"] = np.asarray(key, np.uint32)
    return out


def keys_of(names, qcheck=True):
    k = np.zeros(len(names), abi.READ_KEY)
    for i, nm in enumerate(names):
        nm = nm if isinstance(nm, bytes) else nm.encode()
        k[i]["qhash"] = synth.fnv1a64(nm)
        k[i]["qcheck"] = synth.qname_check(nm) if qcheck else 0
    return k


# ---- a seeded genome ------------------------------------------------------------------------------------------------------------
def base_index(tid, pos):
    """0..3 = A C G T at 0-based positions `pos` (an array) of contig tid"""
    with np.errstate(over="ignore"):
        x = (np.asarray(pos, np.int64).astype(np.uint64) + (np.uint64(tid + 1) << np.uint64(40))) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(29)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(32)
    return (x & np.uint64(3)).astype(np.int64)


def base(tid, pos):
    return "ACGT"[int(base_index(tid, [pos])[0])]


def partner_codes(d, t2, bp2, d2, n):
    """the designed truth of a side with direction d: columns 0 .. n-1 walk into the retained sequence of the partner side (t2, 1-based
    bp2, d2): bp2 + j when it lies right of its breakpoint, bp2 - j when left; complemented when both sides have the same direction"""
    j = np.arange(n)
    idx = base_index(t2, (bp2 + j if d2 == "R" else bp2 - j) - 1)
    if d == d2:
        idx = 3 - idx
    return (1 << idx).astype(np.uint8)


def record_codes(rec, lead=None, trail=None):
    """the 4-bit codes of a synth.Rec: aligned bases are the genome's, clipped ones `lead` / `trail` (in read order) or seeded filler"""
    out, p = [], rec.pos
    words = bamio.parse_cigar(rec.cigar)
    body = [k for k, w in enumerate(words) if (w & 15) != OP_H]
    for k, w in enumerate(words):
        op, n = w & 15, w >> 4
        if op in (0, 7, 8):
            out.append((1 << base_index(rec.tid, p + np.arange(n))).astype(np.uint8))
            p += n
        elif op in (2, 3):
            p += n
        elif op in (1, 4):
            given = lead if (op == OP_S and k == body[0]) else trail if (op == OP_S and k == body[-1]) else None
            if given is None:
                given = (1 << base_index(7, synth.fnv1a64(rec.qname.encode()) % 1_000_003 + np.arange(n))).astype(np.uint8)
            assert len(given) == n
            out.append(np.asarray(given, np.uint8))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


# ---- the designed BAM -----------------------------------------------------------------------------------------------------------
ALL_LOCI = list(cc.LOCI) + [(cc.MIX[0], cc.MIX[1], cc.MIX[2], "L", cc.MIX[3], cc.MIX[4], "L")]
# a read with a leading clip at side B of the third locus and a trailing one 39 bp further: the site of its other end
TWO_CLIP_SITE = (3, 900_039, 0, LEFT)
_DESIGNED = {}


def _clip_rec(q, t, bp, d, cigar, mapq=60, flag_extra=0, shift=0):
    """a read without an SA tag whose alignment ends at 1-based bp + shift (d = 'L') or starts there ('R'), and its plain mate"""
    words = bamio.parse_cigar(cigar)
    pos = bp + shift - bamio.cigar_reflen(words) if d == "L" else bp + shift - 1
    return [synth.Rec(q, 0x1 | 0x2 | 0x40 | 0x20 | flag_extra, t, pos, mapq, cigar, t, pos + 200, 300), synth.Rec(q, 0x1 | 0x2 | 0x80 | 0x10, t, pos + 200, 60, "100M", t, pos, -300)]


def designed():
    """{"ds": the Dataset, "codes": per record its codes (None: l_seq 0), "truth": {(tid, pos, dir): expected bases as text at the
    command line's defaults}, "sites": every locus side and TWO_CLIP_SITE}.  The variations are listed where they are made."""
    if _DESIGNED:
        return _DESIGNED
    ds = cc.designed_tumor()
    by_name = {L[0]: L for L in ALL_LOCI}
    codes = {}

    def side(L, own_a):
        name, ta, bpa, da, tb, bpb, db = L
        return ((ta, bpa, da), (tb, bpb, db)) if own_a else ((tb, bpb, db), (ta, bpa, da))

    def clipped_codes(rec, own, other):
        """the record's clip is the partner's retained sequence"""
        (t, bp, d), (t2, bp2, d2) = own, other
        words = [w for w in bamio.parse_cigar(rec.cigar) if (w & 15) != OP_H]
        if d == "L":
            return record_codes(rec, trail=partner_codes(d, t2, bp2, d2, words[-1] >> 4))
        return record_codes(rec, lead=partner_codes(d, t2, bp2, d2, words[0] >> 4)[::-1])

    split_recs = {}
    for r in ds.recs:
        m = re.match(r"(\w+)S_(\d+)$", r.qname)
        if m and m.group(1) in by_name and r.sa:
            own, other = side(by_name[m.group(1)], not r.flag & 0x100)
            codes[id(r)] = clipped_codes(r, own, other)
            split_recs[(m.group(1), not r.flag & 0x100, int(m.group(2)))] = r
        else:
            codes[id(r)] = record_codes(r)
    truth = {}
    for L in ALL_LOCI:
        for own, other in (side(L, True), side(L, False)):
            n = 40 if own == side(L, True)[0] else 60  # the clip of the primary is m2 = 40, that of its partner m1 = 60
            truth[(own[0], own[1], RIGHT if own[2] == "R" else LEFT)] = [LETTER[c] for c in partner_codes(own[2], *other, n)]

    def col(rec, d, j):
        """index into the codes of rec of column j of its clip on a side of direction d"""
        words = [w for w in bamio.parse_cigar(rec.cigar) if (w & 15) != OP_H]
        return (words[0] >> 4) - 1 - j if d == "R" else len(codes[id(rec)]) - (words[-1] >> 4) + j

    extras = []

    def extra(recs, own=None, other=None, wrong=False, n_seq=None):
        r = recs[0]
        c = clipped_codes(r, own, other) if own else record_codes(r)
        if wrong:  # a read that must not count: were it counted, it would vote against every column
            c = np.where(c == 1, 8, np.where(c == 8, 1, np.where(c == 2, 4, 2))).astype(np.uint8)
        codes[id(r)] = c if n_seq is None else (None if n_seq == 0 else c[:n_seq])
        codes[id(recs[1])] = record_codes(recs[1])
        extras.extend(recs)

    # locus 0, side A (LEFT, 8 primaries clipped 40): a read with a minority base in column 5; clips of 25, 12 and 9 (9 < min_clip)
    A0, B0 = side(cc.LOCI[0], True)
    extra(_clip_rec("xMinor", A0[0], A0[1], "L", "60M40S"), A0, B0)
    r = extras[-2]
    codes[id(r)][col(r, "L", 5)] = CODE["A"] if truth[(A0[0], A0[1], LEFT)][5] != "A" else CODE["C"]
    for c in (25, 12, 9):
        extra(_clip_rec("xClip%d" % c, A0[0], A0[1], "L", "%dM%dS" % (100 - c, c)), A0, B0)
    # locus 0, side B (RIGHT, 8 partners clipped 60): leading H ops, and a clip of 70 whose columns 60 .. 63 have depth 1 (len stops)
    extra(_clip_rec("xHard", B0[0], B0[1], "R", "5H40S60M"), B0, A0)
    extra(_clip_rec("xLong", B0[0], B0[1], "R", "70S30M"), B0, A0)
    # locus 1, side A: 4 : 4 ties in columns 7 and 9, against T (or A) and against A (or T): the smaller base wins
    A1, B1 = side(cc.LOCI[1], True)
    for j, alt in ((7, "T"), (9, "A")):
        t = truth[(A1[0], A1[1], LEFT)]
        other_base = alt if t[j] != alt else ("A" if alt == "T" else "T")
        for k in range(4):
            r = split_recs[(cc.LOCI[1][0], True, k)]
            codes[id(r)][col(r, "L", j)] = CODE[other_base]
        t[j] = min(t[j], other_base)
    # locus 1, side B (LEFT, partners 40M60S): an N and an IUPAC code in column 3: they count in the depth only
    for k, code in ((0, "N"), (1, "R")):
        r = split_recs[(cc.LOCI[1][0], False, k)]
        codes[id(r)][col(r, "L", 3)] = CODE[code]
    # locus 2, side A (RIGHT): reads that do not count: 1 bp off, below -q, a duplicate, l_seq 0, l_seq that disagrees with the CIGAR
    A2, B2 = side(cc.LOCI[2], True)
    extra(_clip_rec("xOff", A2[0], A2[1], "R", "40S60M", shift=1), A2, B2, wrong=True)
    extra(_clip_rec("xLowq", A2[0], A2[1], "R", "40S60M", mapq=10), A2, B2, wrong=True)
    extra(_clip_rec("xDup", A2[0], A2[1], "R", "40S60M", flag_extra=0x400), A2, B2, wrong=True)
    extra(_clip_rec("xNoseq", A2[0], A2[1], "R", "40S60M"), A2, B2, wrong=True, n_seq=0)
    extra(_clip_rec("xShort", A2[0], A2[1], "R", "40S60M"), A2, B2, wrong=True, n_seq=90)
    # locus 2, side B (RIGHT): a read clipped on both ends: its leading clip at the site, its trailing one at TWO_CLIP_SITE
    recs = _clip_rec("xBoth", B2[0], B2[1], "R", "30S40M30S")
    assert (recs[0].tid, recs[0].pos + 40) == TWO_CLIP_SITE[:2]
    extra(recs, B2, A2)
    # locus 3, side B (LEFT): a clip that starts on an odd base, and an odd l_seq
    A3, B3 = side(cc.LOCI[3], True)
    extra(_clip_rec("xOdd", B3[0], B3[1], "L", "61M39S"), B3, A3)
    extra(_clip_rec("xOddLen", B3[0], B3[1], "L", "60M39S"), B3, A3)
    ds.recs += extras
    ds.sort()
    sites = [(t, p, 0, d) for (t, p, d) in truth] + [TWO_CLIP_SITE]
    _DESIGNED.update(ds=ds, codes=codes, truth={k: "".join(v) for k, v in truth.items()}, sites=as_sites(sites))
    return _DESIGNED


def write_designed_bam(path, aligned=True):
    """the designed tumour with its bases (l_seq = 0 where the design says so), SA / OC tags as Dataset.write_bam writes them"""
    d = designed()

    def gen():
        for r in d["ds"].recs:
            aux = ([("SA", r.sa)] if r.sa else []) + ([("OC", r.oc)] if r.oc else [])
            c = d["codes"][id(r)]
            seq, qual = (b"", b"") if c is None else (bytes(pack_codes(c)), b"\x1e" * len(c))
            yield bamio.encode_record(r.qname, r.flag, r.tid, r.pos, r.mapq, bamio.parse_cigar(r.cigar), r.mtid, r.mpos, r.isize, aux, seq=seq, qual=qual)
    bamio.write_bam(path, d["ds"].contigs, gen(), aligned=aligned)


def designed_reads(recs=None):
    """the records of the designed tumour (or those given) as a bk_reads table, without a file"""
    d = designed()
    empty = np.zeros(0, np.uint8)
    return make_reads([(r.tid, r.pos, r.flag, r.mapq, r.cigar, empty if d["codes"][id(r)] is None else d["codes"][id(r)]) for r in (d["ds"].recs if recs is None else recs)])


# ---- numpy-only tables ----------------------------------------------------------------------------------------------------------
def crowd_table(seed=3):
    """(reads, sites): a LEFT site with 300 reads clipped 90 (two rounds of 64 columns at max_len 100, many contributions) with a
    tenth of the bases off, N among them; a RIGHT site with 50 reads clipped 20 .. 90; an empty site; a site with tid = -1; the
    first site again"""
    rng = np.random.default_rng(seed)
    t_left = rng.choice([1, 2, 4, 8], 90)
    t_right = rng.choice([1, 2, 4, 8], 90)
    items = []
    for i in range(300):
        clip = np.where(rng.random(90) < 0.1, rng.choice([1, 2, 4, 8, 15, 5], 90), t_left).astype(np.uint8)
        items.append((0, 4990, 0x1 if i & 1 else 0, 60, "10M90S", np.concatenate([np.full(10, 1, np.uint8), clip])))
    for i in range(50):
        c = int(rng.integers(20, 91))
        clip = np.where(rng.random(c) < 0.1, rng.choice([1, 2, 4, 8], c), t_right[:c]).astype(np.uint8)
        items.append((0, 6999, 0, 30, "%dS%dM" % (c, 100 - c), np.concatenate([clip[::-1], np.full(100 - c, 2, np.uint8)])))
    order = rng.permutation(len(items))
    sites = as_sites([(0, 5000, 0, LEFT), (1, 123, 0, LEFT), (-1, 5000, 0, LEFT), (0, 5000, 0, LEFT), (0, 7000, 0, RIGHT), (0, 5000, 0, RIGHT)])
    return make_reads([items[i] for i in order]), sites

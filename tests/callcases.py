"""Shared cases of the per-call GPU tests (test_gpu_normal, _exclude, _genotype, _vcf, _evidence): the seeded and designed
datasets, copies of a record table on and off the device, and the numpy definitions more than one of those modules checks against."""
import os

import numpy as np

from breakid_amd import abi, bamio, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")
QUAL = 20
CONTIGS = [("chr1", 2_000_000), ("chr2", 2_000_000), ("chr3", 2_000_000), ("chr4", 2_000_000)]
NAMES = [n for n, _ in CONTIGS]


# ---- record tables: an exclude list applied on the host, copies on and off the device ------------------------------------------------
FIXED = ("tid", "pos", "mtid", "mpos", "isize", "flag", "mapq", "qhash", "qcheck")


def excluded_mask(cols, tid, beg, end):
    ep = rec_endpos(cols)
    t = cols["tid"]
    p = cols["pos"].astype(np.int64)
    ex = np.zeros(len(t), bool)
    for T, b, e in zip(tid, beg, end):
        ex |= (t == T) & (p < e) & (ep > b)
    return ex


def filtered(cols, keep):
    """the table without the records where keep is False, CIGAR words and aux bytes repacked"""
    out = {k: np.ascontiguousarray(cols[k][keep]) for k in FIXED if k in cols}
    for blob, off in (("cigar", "cigar_off"), ("aux", "aux_off")):
        o = cols[off].astype(np.int64)
        ln = np.diff(o)
        out[blob] = np.ascontiguousarray(cols[blob][:o[-1]][np.repeat(keep, ln)])
        out[off] = np.concatenate([[0], np.cumsum(ln[keep])]).astype(np.uint32)
    return out


def to_device(cols, qcheck=True):
    """torch copies of the columns on cuda:0 (same bits; unsigned columns as their signed twins) and their device pointers"""
    import torch
    dev = torch.device("cuda", 0)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    t = {}
    for k, dt in abi.SOA_COLS_ALL:
        if k == "qcheck" and (not qcheck or k not in cols):
            continue
        a = np.ascontiguousarray(cols[k], dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        s = signed.get(np.dtype(dt))
        t[k] = torch.from_numpy(a.view(s) if s is not None else a).to(dev)
    return t, abi.device_ptrs(t)


def make_ctx(contigs, cols, where, qcheck=True):
    """(context, what must stay alive); where = 'host' (bk_upload_records) or 'device' (BK_MEM_DEVICE)"""
    ctx = capi.Context(contigs)
    c = dict(cols)
    if not qcheck:
        c.pop("qcheck", None)
    if where == "host":
        ctx.upload(c)
        return ctx, None
    t, ptrs = to_device(c, qcheck)
    ctx.attach_device(ptrs, len(c["tid"]), int(c["cigar_off"][-1]), int(c["aux_off"][-1]))
    return ctx, t


def device_cols(table):
    import torch
    from breakid_amd.sharded import tensor_from_ptr
    dev = torch.device("cuda", 0)
    s = table.soa
    n = s.n
    sizes = {"cigar_off": n + 1, "aux_off": n + 1, "cigar": s.n_cigar_words, "aux": s.n_aux_bytes}
    out = {}
    for name, dt in abi.SOA_COLS_ALL:
        cnt = sizes.get(name, n)
        nb = cnt * np.dtype(dt).itemsize
        out[name] = tensor_from_ptr(getattr(s, name), nb, dev).cpu().numpy().view(dt).copy() if nb else np.zeros(0, dt)
    return out


# ---- bk_normal_support: its definition, a tumour / normal pair ------------------------------------------------------------------------
def pair_type(p):
    """orientation bit of every pair, as k_accumulate folds it into type_mask"""
    r1, r2 = p["p1_rev"] != 0, p["p2_rev"] != 0
    same = (np.where(r1 & ~r2, 4, 0) | np.where(r1 == r2, 2, 0) | np.where(~r1 & r2, 8, 0)).astype(np.uint32)
    return np.where(p["p1_tid"] != p["p2_tid"], np.uint32(1), same)


def rec_endpos(cols):
    """bam_endpos of every record: pos + reference length of the CIGAR (M D N = X), pos + 1 without CIGAR or when unmapped"""
    cig = cols["cigar"].astype(np.int64)
    off = cols["cigar_off"].astype(np.int64)
    cons = np.isin(cig & 15, [0, 2, 3, 7, 8])
    csum = np.concatenate([[0], np.cumsum(np.where(cons, cig >> 4, 0))])
    pos = cols["pos"].astype(np.int64)
    has = (off[1:] > off[:-1]) & ((cols["flag"] & 4) == 0)
    return np.where(has, pos + csum[off[1:]] - csum[off[:-1]], pos + 1)


def single_base_depth(cols, endpos, tid, bp):
    """cal_single_base_depth: records overlapping [bp - 1, bp) with mapq > 0, not 0x400, 0x1 set"""
    beg, end = max(0, bp - 1), bp
    if end < beg or tid < 0:
        return 0
    f = cols["flag"]
    m = (cols["tid"] == tid) & (cols["pos"].astype(np.int64) < end) & (endpos > beg) & (cols["mapq"] > 0) & ((f & 0x400) == 0) & ((f & 1) != 0)
    return int(m.sum())


def expected_support(cl, scan, splits, cols, w):
    """(the synthetic reference lists have unique names: the interned id of the call's chromosome is its tid)"""
    W = int(w)  # (int) w, truncation toward zero like the C conversion
    out = np.zeros(len(cl), abi.NORMAL_SUPPORT)
    pt = pair_type(scan)
    p1 = scan["p1_pos"].astype(np.int64)
    p2 = scan["p2_pos"].astype(np.int64)
    ok_sp = (splits["flags"] & 2) == 0
    pb, sb = splits["prim_bp"].astype(np.int64), splits["sec_bp"].astype(np.int64)
    endpos = rec_endpos(cols)
    for i, c in enumerate(cl):
        m = ((scan["p1_tid"] == c["p1_tid"]) & (scan["p2_tid"] == c["p2_tid"]) & (p1 >= int(c["p1_min"]) - W) & (p1 <= int(c["p1_max"]) + W)
             & (p2 >= int(c["p2_min"]) - W) & (p2 <= int(c["p2_max"]) + W) & ((pt & c["type_mask"]) != 0))
        out[i]["n_drp"] = int(m.sum())
        if not c["flags"] & 2:
            continue
        e1, e2 = int(c["p1_exact"]), int(c["p2_exact"])
        t1, t2 = int(c["p1_tid"]), int(c["p2_tid"])
        own = (splits["tid"] == t1) | (splits["tid"] == t2)  # tuples whose own record lies on the call's chromosomes
        f1 = (splits["prim_chr"] == t1) & (splits["sec_chr"] == t2) & (np.abs(pb - e1) <= 2) & (np.abs(sb - e2) <= 2)
        f2 = (splits["prim_chr"] == t2) & (splits["sec_chr"] == t1) & (np.abs(pb - e2) <= 2) & (np.abs(sb - e1) <= 2)
        out[i]["n_sr"] = int((own & ok_sp & (f1 | f2)).sum())
        out[i]["depth1"] = single_base_depth(cols, endpos, t1, e1)
        out[i]["depth2"] = single_base_depth(cols, endpos, t2, e2)
    return out


# (ta, pa, tb, pb, rev_a, rev_b): split reads break at 1-based pa + 30 / pb + 30, as in synth.make_cfg
GERMLINE = [(0, 300_000, 1, 700_000, False, True), (0, 900_000, 0, 1_400_000, False, True), (2, 400_000, 2, 1_200_000, True, False),
            (1, 1_500_000, 3, 250_000, True, True)]
DENSE = (3, 800_000, 3, 1_600_000, False, True)  # germline deletion whose window holds > 256 of the normal's pairs (several k_normal_drp steps)
SOMATIC = [(0, 1_700_000, 2, 900_000, False, True), (1, 300_000, 1, 1_100_000, False, True), (3, 1_200_000, 2, 1_600_000, True, False)]


def tumor_normal(seed=7, extra_contigs=0, names4=("chr1", "chr2", "chr3", "chr4")):
    """Tumour: every locus with 14 discordant pairs and 6 split reads.  Normal: the germline loci again with fresh read names
    and jitter (fewer pairs, 3 split reads, plus split reads 2 and 3 bp off the breakpoints and pairs of the wrong orientation),
    the dense locus with 700 pairs, no somatic locus.  `extra_contigs` pads the reference list (records stay on the first four);
    `names4` names the first four contigs."""
    rng = np.random.default_rng(seed)
    contigs = [(nm, 2_000_000) for nm in names4] + [("u%d" % i, 10_000) for i in range(extra_contigs)]
    names = [n for n, _ in contigs]
    tum, nor = synth.Dataset(list(contigs)), synth.Dataset(list(contigs))
    for ds, prefix, n in ((tum, "tp", 12000), (nor, "np", 12000)):
        for i in range(n):
            t = int(rng.integers(0, 4))
            ds.recs += synth._proper_pair(rng, i, t, 1000, 1_999_000, 100, 350, 40, prefix=prefix)

    def locus(ds, tag, L, n_pairs, n_splits, jitter=300, bp_shift=0, rev=None):
        ta, pa, tb, pb, ra, rb = L
        if rev is not None:
            ra, rb = rev
        for k in range(n_pairs):
            ds.recs += synth._discordant_pair("%s_%d" % (tag, k), ta, pa + int(rng.integers(-jitter, jitter + 1)), tb, pb + int(rng.integers(-jitter, jitter + 1)),
                                              100, ra, rb)
        for k in range(n_splits):
            ds.recs += synth._split_pair("%sS_%d" % (tag, k), names, ta, pa + 30 + bp_shift, tb, pb + 30 + bp_shift, 60, 40)

    for li, L in enumerate(GERMLINE):
        locus(tum, "TG%d" % li, L, 14, 6)
        locus(nor, "NG%d" % li, L, 6 + li, 3)
        locus(nor, "NGa%d" % li, L, 0, 1, bp_shift=2)  # inside the +-2 bp of the vote
        locus(nor, "NGb%d" % li, L, 0, 1, bp_shift=3)  # outside
        locus(nor, "NGo%d" % li, L, 3, 0, rev=(not L[4], not L[5]) if L[0] != L[2] else (True, True))  # other orientation
    locus(tum, "TD", DENSE, 14, 6)
    locus(nor, "ND", DENSE, 700, 3, jitter=400)
    for li, L in enumerate(SOMATIC):
        locus(tum, "TS%d" % li, L, 14, 6)
    tum.sort()
    nor.sort()
    return tum, nor


# ---- bk_ref_support: its definition, a seeded tumour ----------------------------------------------------------------------------------
NEVER = 0x4 | 0x100 | 0x200 | 0x400 | 0x800


def side_masks(cols, T, e, mapq_min, anchor, w, endpos=None, ignore_aux=False):
    """(ref_reads mask, ref_pairs mask) over the records for one side: chromosome T, exact 1-based breakpoint e"""
    W = int(w)  # (int) w
    n = len(cols["tid"])
    if T < 0:
        return np.zeros(n, bool), np.zeros(n, bool)
    endpos = rec_endpos(cols) if endpos is None else endpos
    b = int(e) - 1
    A = int(anchor)
    flag = cols["flag"].astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    isize = cols["isize"].astype(np.int64)
    aux_off = cols["aux_off"].astype(np.int64)
    elig = (cols["tid"] == T) & ((flag & 1) != 0) & ((flag & NEVER) == 0) & (cols["mapq"].astype(np.int64) >= mapq_min) & (pos <= b - A)
    if not ignore_aux:
        elig &= aux_off[1:] == aux_off[:-1]
    reads = elig & (endpos >= b + 1 + A)
    pairs = elig & ((flag & 2) != 0) & ((flag & 8) == 0) & (isize > 0) & (isize <= W) & (pos + isize >= b + 1 + A)
    return reads, pairs


def expected_ref_support(cl, cols, mapq_min, anchor, w):
    out = np.zeros(len(cl), abi.REF_SUPPORT)
    endpos = rec_endpos(cols)
    for i, c in enumerate(cl):
        if not c["flags"] & 2:
            continue
        for s, (T, e) in enumerate(((int(c["p1_tid"]), int(c["p1_exact"])), (int(c["p2_tid"]), int(c["p2_exact"]))), 1):
            reads, pairs = side_masks(cols, T, e, mapq_min, anchor, w, endpos)
            out[i]["ref_reads%d" % s] = int(reads.sum())
            out[i]["ref_pairs%d" % s] = int(pairs.sum())
    return out


# (name, ta, pa, tb, pb, split reads, local proper pairs per side, truth); split reads break at 1-based pa + 30 / pb + 30
GENOTYPE_LOCI = [("het1", 0, 300_000, 1, 700_000, 10, 200, 1), ("het2", 2, 400_000, 2, 1_200_000, 10, 200, 1), ("hom", 1, 1_500_000, 3, 250_000, 10, 0, 2),
                 ("sub", 0, 1_700_000, 2, 900_000, 4, 3000, 0), ("deep", 3, 1_200_000, 0, 1_000_000, 10, 12000, 0)]


def genotype_tumor(seed=11, loci=GENOTYPE_LOCI, prefix="t", n_background=12000):
    """12 000 background pairs; per locus 14 discordant pairs, its split reads, and local proper pairs within +-2 kb of either
    breakpoint (the reference allele).  The homozygous locus has no reference allele: its discordant reads stay off the breakpoint
    base (left of it on side a, right of it on side b), and no background fragment lies within 1 kb of its breakpoints."""
    rng = np.random.default_rng(seed)
    names = [n for n, _ in CONTIGS]
    ds = synth.Dataset(list(CONTIGS))
    hom = [(L[1], L[2] + 30) for L in loci if L[7] == 2] + [(L[3], L[4] + 30) for L in loci if L[7] == 2]
    for i in range(n_background):
        t = int(rng.integers(0, 4))
        pr = synth._proper_pair(rng, i, t, 1000, 1_999_000, 100, 350, 40, prefix=prefix + "p")
        if any(t == ht and pr[0].pos - 1000 < hb < pr[1].pos + 1100 for ht, hb in hom):
            continue
        ds.recs += pr
    k = 0
    for name, ta, pa, tb, pb, n_split, n_local, truth in loci:
        for j in range(14):
            if truth == 2:
                da, db = -int(rng.integers(80, 300)), int(rng.integers(40, 300))  # a: ends before pa + 30; b: starts behind pb + 30
            else:
                da, db = int(rng.integers(-300, 301)), int(rng.integers(-300, 301))
            ds.recs += synth._discordant_pair("%s%sD_%d" % (prefix, name, j), ta, pa + da, tb, pb + db, 100, False, True)
        for j in range(n_split):
            ds.recs += synth._split_pair("%s%sS_%d" % (prefix, name, j), names, ta, pa + 30, tb, pb + 30, 60, 40)
        for t, p in ((ta, pa), (tb, pb)):
            for j in range(n_local):
                ds.recs += synth._proper_pair(rng, k, t, p - 2000, p + 2000, 100, 350, 40, prefix=prefix + name + "L")
                k += 1
    ds.sort()
    return ds


_TUMOR = {}


def tumor():
    if "t" not in _TUMOR:
        ds = genotype_tumor()
        _TUMOR["t"] = (ds, ds.to_soa())
    return _TUMOR["t"]


# ---- bk_junctions: its definition, the datasets and the designed loci -----------------------------------------------------------------
def expected_junctions(cl, clustered, splits):
    """(the synthetic reference lists have unique names: the interned id of a header contig is its tid)"""
    out = np.zeros(len(cl), abi.JUNCTION)
    key = (clustered["group"].astype(np.int64) << 32) | (clustered["cluster"].astype(np.int64) & 0xFFFFFFFF)
    strands = 2 * clustered["p1_rev"].astype(np.int64) + clustered["p2_rev"].astype(np.int64)
    q1, q2 = clustered["p1_mapq"].astype(np.int64), clustered["p2_mapq"].astype(np.int64)
    ok_sp = (splits["flags"] & 2) == 0
    pb, sb = splits["prim_bp"].astype(np.int64), splits["sec_bp"].astype(np.int64)
    prim_right = (splits["prim_bp"] == splits["prim_start"]).astype(np.int64)
    sec_right = (splits["sec_bp"] == splits["sec_start"]).astype(np.int64)
    for i, c in enumerate(cl):
        m = key == ((int(c["group"]) << 32) | (int(c["id"]) & 0xFFFFFFFF))
        out["pairs"][i] = np.bincount(strands[m], minlength=4)
        out["mapq_sum1"][i] = int(q1[m].sum())
        out["mapq_sum2"][i] = int(q2[m].sum())
        if not c["flags"] & 2:
            continue
        e1, e2 = int(c["p1_exact"]), int(c["p2_exact"])
        t1, t2 = int(c["p1_tid"]), int(c["p2_tid"])
        own = ((splits["tid"] == t1) | (splits["tid"] == t2)) & ok_sp
        f1 = own & (splits["prim_chr"] == t1) & (splits["sec_chr"] == t2) & (np.abs(pb - e1) <= 2) & (np.abs(sb - e2) <= 2)
        f2 = own & ~f1 & (splits["prim_chr"] == t2) & (splits["sec_chr"] == t1) & (np.abs(pb - e2) <= 2) & (np.abs(sb - e1) <= 2)
        out["splits"][i] = (np.bincount((2 * prim_right + sec_right)[f1], minlength=4) + np.bincount((2 * sec_right + prim_right)[f2], minlength=4))
    return out


def call_dataset(name):
    if name == "genotype":
        return tumor()
    if name == "edge":
        ds = synth.make_edge()
    else:
        contigs = [("chr%d" % i, 3_000_000) for i in range(1, 9)]
        ds = synth.make_cfg(17, contigs, 120_000, 300, 16, 200, split_every=1, splits_per_locus=6, jitter=250, read_len=100)
    return ds, ds.to_soa()


# (name, ta, bpa, da, tb, bpb, db): d = 'L' the retained sequence lies left of the breakpoint (the alignment ends at it), 'R' right
LOCI = [("LR_x", 0, 300_000, "L", 1, 700_000, "R"), ("LL_x", 0, 600_000, "L", 2, 500_000, "L"), ("RR_x", 1, 300_000, "R", 3, 900_000, "R"),
        ("RL_x", 2, 900_000, "R", 3, 400_000, "L"),
        ("LR_s", 0, 1_000_000, "L", 0, 1_400_000, "R"), ("LL_s", 1, 1_000_000, "L", 1, 1_400_000, "L"), ("RR_s", 2, 1_200_000, "R", 2, 1_600_000, "R"),
        ("RL_s", 3, 1_200_000, "R", 3, 1_600_000, "L")]
MIX = ("MIX", 0, 1_700_000, 2, 1_300_000)  # pairs of strands (forward, reverse), split reads clipped as (L, L)


def designed_split(q, ta, bpa, da, tb, bpb, db, m1=60, m2=40, names=NAMES):
    """own record m1M m2S ending at 1-based bpa (left) or m2S m1M starting at it (right); the 0x100 partner m2M m1S ending at / m1S m2M
    starting at bpb; SA strings as synth._split_pair writes them"""
    ca = "%dM%dS" % (m1, m2) if da == "L" else "%dS%dM" % (m2, m1)
    pa = bpa - m1 if da == "L" else bpa - 1
    cb = "%dM%dS" % (m2, m1) if db == "L" else "%dS%dM" % (m1, m2)
    pb = bpb - m2 if db == "L" else bpb - 1
    st = "-" if da == db else "+"
    sa1 = "%s,%d,%s,%s,60,0;" % (names[tb], pb + 1, st, cb)
    sa2 = "%s,%d,%s,%s,60,0;" % (names[ta], pa + 1, st, ca)
    prim = synth.Rec(q, 0x1 | 0x2 | 0x40 | 0x20, ta, pa, 60, ca, ta, pa + 200, 300, sa=sa1)
    part = synth.Rec(q, 0x1 | 0x40 | 0x20 | 0x100, tb, pb, 60, cb, ta, pa + 200, 0, sa=sa2)
    mate = synth.Rec(q, 0x1 | 0x2 | 0x80 | 0x10, ta, pa + 200, 60, "100M", ta, pa, -300)
    return [prim, part, mate]


def designed_tumor(mix=True, contigs=CONTIGS, loci=LOCI, n_proper=12000):
    rng = np.random.default_rng(5)
    ds = synth.Dataset(list(contigs))
    names = [n for n, _ in contigs]
    for i in range(n_proper):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, len(contigs))), 1000, 1_999_000, 100, 350, 40)
    for name, ta, bpa, da, tb, bpb, db in loci:
        for j in range(14):
            oa = -int(rng.integers(100, 400)) if da == "L" else int(rng.integers(0, 300))
            ob = -int(rng.integers(100, 400)) if db == "L" else int(rng.integers(0, 300))
            ds.recs += synth._discordant_pair("%sD_%d" % (name, j), ta, bpa + oa, tb, bpb + ob, 100, rev_a=(da == "R"), rev_b=(db == "R"))
        for j in range(8):
            ds.recs += designed_split("%sS_%d" % (name, j), ta, bpa, da, tb, bpb, db, names=names)
    if mix:
        _, ta, bpa, tb, bpb = MIX
        for j in range(14):
            ds.recs += synth._discordant_pair("MIXD_%d" % j, ta, bpa - int(rng.integers(100, 400)), tb, bpb + int(rng.integers(0, 300)), 100, rev_a=False, rev_b=True)
        for j in range(8):
            ds.recs += designed_split("MIXS_%d" % j, ta, bpa, "L", tb, bpb, "L")
    ds.sort()
    return ds


def rows_of(cl, ta, bpa, tb, bpb):
    """voted rows whose exact breakpoints are the two given ones: [(row, True when side 1 is A)]"""
    out = []
    for i, c in enumerate(cl):
        if not c["flags"] & 2:
            continue
        s1, s2 = (int(c["p1_tid"]), int(c["p1_exact"])), (int(c["p2_tid"]), int(c["p2_exact"]))
        if (s1, s2) == ((ta, bpa), (tb, bpb)):
            out.append((i, True))
        elif (s1, s2) == ((tb, bpb), (ta, bpa)):
            out.append((i, False))
    return out


def quiet_tumor():
    tum = synth.Dataset(list(CONTIGS))
    rng = np.random.default_rng(3)
    for i in range(4000):
        tum.recs += synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40)
    tum.sort()
    return tum


def designed_refgene():
    """a gene on either side of the four loci that join two contigs (they pass the gene-pair filter); none at the other loci"""
    rows = []
    for name, ta, bpa, da, tb, bpb, db in LOCI[:4]:
        for tag, t, bp in (("A", ta, bpa), ("B", tb, bpb)):
            s, e = bp - 10_000, bp + 10_000
            rows.append("0\tNM_%s%s\t%s\t+\t%d\t%d\t%d\t%d\t2\t%d,%d,\t%d,%d,\t0\tG%s_%s\tcmpl\tcmpl\t0,0," % (
                name, tag, NAMES[t], s, e, s + 50, e - 50, s, bp + 2_000, bp - 2_000, e, tag, name))
    return rows


def fusion_rows(path):
    lines = open(path).read().split("\n")
    return [l.split("\t") for l in lines[1:] if l]


def designed_normal():
    """a normal with background, the first locus again (fewer reads) and nothing else"""
    rng = np.random.default_rng(23)
    ds = synth.Dataset(list(CONTIGS))
    for i in range(8000):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, 4)), 1000, 1_999_000, 100, 350, 40, prefix="np")
    name, ta, bpa, da, tb, bpb, db = LOCI[0]
    for j in range(6):
        ds.recs += synth._discordant_pair("n%sD_%d" % (name, j), ta, bpa - int(rng.integers(100, 400)), tb, bpb + int(rng.integers(0, 300)), 100, rev_a=False, rev_b=True)
    for j in range(3):
        ds.recs += designed_split("n%sS_%d" % (name, j), ta, bpa, da, tb, bpb, db)
    ds.sort()
    return ds


def write_indexed(ds, path, aligned=True):
    ds.write_bam(path, aligned=aligned)
    bamio.write_bai(path)


EXCLUDE = (np.asarray([0, 3], np.int32), np.asarray([50_000, 100_000], np.int32), np.asarray([60_000, 120_000], np.int32))

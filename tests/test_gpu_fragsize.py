"""Fragment sizes (`bk_fragment_sizes`, `-fragsize`): the kernels against the definition in tests/fragcases.py byte for byte, the
expectations taken from the fetched tables (bk_evidence's rows and the record columns).  Calls of 3 to 258 member pairs with skipped sites
between them; the end of a reverse mate under every kind of CIGAR and every side combination; pile-ups of 0 to 1100 records at the mate's
position, the wanted record first, last and on either side of a multiple of the sampled keys' stride; sites that put rows off, in front of
their reads and at the ends of the coordinate range; bounds on a length and one off it; every table form; every refusal; timing; a seeded
sample against the brute-force statement; and the command line's files."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import fragcases as fc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
STAGES = (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)
SIZES = [3, 63, 64, 65, 127, 128, 129, 257]  # member pairs of the calls: the smallest the stages keep, a ballot, a workgroup, one more
LOCUS_PAIRS = [2, 2, 3, 63, 64, 65, 127, 128, 129, 258, 257, 5]  # pairs drawn per locus (two pairs are no cluster; the last locus loses some)
CIGARS = ["100M", "40S60M", "60M40S", "50M10D50M", "50M1000N50M", "50M5I45M", "30=2X68="]
FWD1, REV1 = 0x1 | 0x40, 0x1 | 0x40 | 0x10
FWD2, REV2 = 0x1 | 0x80, 0x1 | 0x80 | 0x10


def pair(q, ta, pa, ca, rev_a, tb, pb, cb, rev_b, mapq=60):
    """a discordant pair with CIGARs of its own; pa, pb are 0-based starts"""
    fa = (REV1 if rev_a else FWD1) | (0x20 if rev_b else 0)
    fb = (REV2 if rev_b else FWD2) | (0x20 if rev_a else 0)
    return [synth.Rec(q, fa, ta, pa, mapq, ca, tb, pb, 0), synth.Rec(q, fb, tb, pb, mapq, cb, ta, pa, 0)]


def background(ds, n, seed, hi=1_999_000):
    rng = np.random.default_rng(seed)
    for i in range(n):
        ds.recs += synth._proper_pair(rng, i, int(rng.integers(0, len(ds.contigs))), 1000, hi, 100, 350, 40)


class Run:
    """a context after the stages, with what the expectations need: bk_evidence's rows, the record columns, the library's bounds"""

    def __init__(self, ds=None, cols=None, ctx=None, hold=None, contigs=None):
        self.cols = ds.to_soa() if cols is None else cols
        if ctx is None:
            ctx = capi.Context(ds.contigs if contigs is None else contigs)
            ctx.upload(self.cols)
            ctx.run(qual=QUAL, fast=True)
        self.ctx, self.hold = ctx, hold
        self.ev, self.off = ctx.evidence()
        self.cl = ctx.fetch(abi.STAGE_CLUSTERS)[0]
        self.mean, self.sd = ctx.isize_stats()
        self.lo, self.hi = capi.fragment_bounds(self.mean, self.sd)
        self.n_pair = np.asarray([int((self.ev["kind"][int(self.off[c]):int(self.off[c + 1])] == abi.EV_PAIR).sum()) for c in range(len(self.cl))], np.int64)

    def close(self):
        self.ctx.close()

    def sites(self, rights=None, skip=None, at=None):
        """one site per call: the sides its first pair row fits (or `rights`), at the call's mean positions (or at = (pos1, pos2) arrays)"""
        s = np.zeros(len(self.cl), abi.FRAG_SITE)
        for c in range(len(self.cl)):
            first = self.ev[int(self.off[c])] if self.n_pair[c] else None
            s[c]["right1"] = rights[0] if rights else (0 if first is None else int((first["flag1"] & 0x10) != 0))
            s[c]["right2"] = rights[1] if rights else (0 if first is None else int((first["flag2"] & 0x10) != 0))
        s["pos1"] = self.cl["p1_mean"] if at is None else at[0]
        s["pos2"] = self.cl["p2_mean"] if at is None else at[1]
        if skip is not None:
            s["skip"] = skip
        return s

    def check(self, sites, lo=None, hi=None, brute=True, lost=0):
        lo, hi = self.lo if lo is None else lo, self.hi if hi is None else hi
        exp = fc.expected_sorted(self.ev, self.off, self.cols, sites, lo, hi)
        if brute:
            assert exp.tobytes() == fc.expected(self.ev, self.off, self.cols, sites, lo, hi).tobytes()
        got = self.ctx.fragment_sizes(sites, lo, hi)
        assert got.dtype == abi.FRAG_SIZES and len(got) == len(exp)
        bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
        assert not bad, [(k, sites[k], got[k], exp[k]) for k in bad[:5]]
        live = sites["skip"] == 0
        total = got["n_used"].astype(np.int64) + got["n_off"] + got["n_lost"]
        assert np.all(total[live] == self.n_pair[live]) and not total[~live].any() and int(got["n_lost"].sum()) == lost
        return got


# ---- 1. calls by size ----------------------------------------------------------------------------------------------------------------------
def sized_sample(sizes=LOCUS_PAIRS):
    """background, and one locus per size on chr1 -> chr2, 20 kb apart: forward reads left of a breakpoint, reverse mates right of the other"""
    ds = synth.Dataset(list(cc.CONTIGS))
    background(ds, 3000, 40)
    for k, m in enumerate(sizes):
        bpa, bpb = 200_000 + 20_000 * k, 300_000 + 20_000 * k
        for j in range(m):
            # (every read on a position of its own: the stages then keep each pair once)
            ds.recs += pair("s%d_%d" % (m, j), 0, bpa - 100 - j * 7 % 300, "100M", False, 1, bpb + j * 11 % 300, CIGARS[j % len(CIGARS)], True)
    ds.sort()
    return ds


@pytest.fixture(scope="module")
def sized():
    r = Run(sized_sample())
    yield r
    r.close()


def test_calls_by_size(sized):
    """a ballot, a workgroup, one more: every size is kept as one call, and every call is answered between skipped neighbours"""
    assert set(SIZES) <= set(sized.n_pair.tolist()) and sized.n_pair.min() == min(SIZES), sorted(sized.n_pair.tolist())
    n = len(sized.cl)
    for skip in (np.zeros(n, np.uint8), np.arange(n) % 2, (np.arange(n) + 1) % 2, np.ones(n, np.uint8)):
        got = sized.check(sized.sites(rights=(0, 1), skip=skip, at=(sized.cl["p1_max"] + 120, sized.cl["p2_min"] - 20)))
        assert np.all(got["n_used"][skip == 0] == sized.n_pair[skip == 0]) and all(r.tobytes() == bytes(48) for r in got[skip != 0])
    again = sized.ctx.fragment_sizes(sized.sites(rights=(0, 1)), sized.lo, sized.hi)
    assert again.tobytes() == sized.ctx.fragment_sizes(sized.sites(rights=(0, 1)), sized.lo, sized.hi).tobytes()  # two calls: the same bytes


def test_zero_and_one_cluster():
    quiet = Run(cc.quiet_tumor())
    assert len(quiet.cl) == 0 and len(quiet.ctx.fragment_sizes(np.zeros(0, abi.FRAG_SITE), 0, 10)) == 0
    with pytest.raises(capi.BreakIDError, match="1 sites for 0 clusters"):
        quiet.ctx.fragment_sizes(np.zeros(1, abi.FRAG_SITE), 0, 10)
    quiet.close()
    one = Run(sized_sample([12]))
    assert len(one.cl) == 1 and one.n_pair[0] >= 3
    got = one.check(one.sites())
    assert int(got[0]["n_used"]) == one.n_pair[0]
    one.check(one.sites(skip=np.ones(1, np.uint8)))
    one.close()


# ---- 2. the end of the reverse mate, and the sites ---------------------------------------------------------------------------------------------
def cigar_sample():
    """four loci, one per side combination, 14 pairs each, both reads going through the CIGARs"""
    rng = np.random.default_rng(43)
    ds = synth.Dataset(list(cc.CONTIGS))
    background(ds, 3000, 42)
    for k, (ra, rb) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        bpa, bpb = 400_000 + 50_000 * k, 900_000 + 50_000 * k
        for j in range(14):
            oa = int(rng.integers(0, 300)) if ra else -int(rng.integers(100, 400))
            ob = int(rng.integers(0, 300)) if rb else -int(rng.integers(100, 400))
            ds.recs += pair("c%d_%d" % (k, j), 2, bpa + oa, CIGARS[j % len(CIGARS)], ra, 3, bpb + ob, CIGARS[(j + 3) % len(CIGARS)], rb)
    ds.sort()
    return ds


@pytest.fixture(scope="module")
def cigars():
    r = Run(cigar_sample())
    yield r
    r.close()


def test_end_of_the_reverse_mate(cigars):
    assert len(cigars.cl) == 4 and np.all(cigars.n_pair >= 10)  # (the stages drop some pairs of a group's last cluster)
    got = cigars.check(cigars.sites())
    combos = [(int(s["right1"]), int(s["right2"])) for s in cigars.sites()]
    assert sorted(combos) == [(0, 0), (0, 1), (1, 0), (1, 1)] and np.all(got["n_used"] == cigars.n_pair)
    # a reverse read's retained bases end at bam_endpos: the records of the right-hand sides cover every CIGAR, and their ends differ
    seen = set()
    for c, s in enumerate(cigars.sites()):
        for row in cigars.ev[int(cigars.off[c]):int(cigars.off[c + 1])]:
            for side in (1, 2):
                if s["right%d" % side]:
                    at = np.flatnonzero((cigars.cols["tid"] == row["tid%d" % side]) & (cigars.cols["pos"] == int(row["pos%d" % side]) - 1) & (cigars.cols["qhash"] == row["qhash"]))
                    seen.add(int(fc.rec_endpos(cigars.cols)[at[0]]) - int(cigars.cols["pos"][at[0]]))
    assert seen == {100, 60, 110, 1100, 95}
    # every other combination of sides: each call is used under one and off under three
    for rights in ((0, 0), (0, 1), (1, 0), (1, 1)):
        got = cigars.check(cigars.sites(rights=rights))
        fits = np.asarray([c == rights for c in combos])
        assert np.all(got["n_used"] == np.where(fits, cigars.n_pair, 0)) and np.all(got["n_off"] == np.where(fits, 0, cigars.n_pair))


def test_sites(sized):
    base = sized.sites(rights=(0, 1))
    n = len(base)
    # strands against the site on side 1, on side 2 and on both
    for rights in ((1, 1), (0, 0), (1, 0)):
        got = sized.check(sized.sites(rights=rights))
        assert np.all(got["n_off"] == sized.n_pair) and not got["n_used"].any()
    # a breakpoint in front of the reads' starts, and behind the mates' ends: negative retained lengths and negative sums
    front = sized.check(sized.sites(rights=(0, 1), at=(sized.cl["p1_min"] - 700, sized.cl["p2_max"] + 900)))
    assert np.all(front["max"] < 0) and np.all(front["sum"] < 0) and np.all(front["n_short"] == sized.n_pair)
    assert any((2 * int(r["sum"]) + int(r["n_used"])) % (2 * int(r["n_used"])) for r in front)  # a centre that is floored
    # pos 0 and 0xFFFFFFFF: the clamp at both ends
    for p1, p2, mn in ((fc.U32, fc.U32, None), (0, 0, None), (fc.U32, 0, fc.I32_MAX), (0, fc.U32, -fc.I32_MAX)):
        got = sized.check(sized.sites(rights=(0, 1), at=(np.full(n, p1, np.uint32), np.full(n, p2, np.uint32))))
        assert mn is None or (np.all(got["min"] == mn) and np.all(got["max"] == mn))
    # lo / hi exactly on a length and one off it; lo == hi
    detail = []
    fc.expected(sized.ev, sized.off, sized.cols, base, 0, 0, detail)
    L0 = sorted(L for c, kind, L, a in detail if kind == "used")[len(detail) // 2]
    counts = {}
    for lo, hi in ((L0, L0), (L0 + 1, L0 + 1), (L0 - 1, L0 - 1), (L0, L0 + 1), (L0 - 1, L0), (-5, fc.I32_MAX), (-fc.I32_MAX - 1, fc.I32_MAX)):
        got = sized.check(base, lo, hi)
        counts[(lo, hi)] = (int(got["n_short"].sum()), int(got["n_long"].sum()))
    on = sum(L == L0 for c, kind, L, a in detail if kind == "used")
    total = int(sized.n_pair.sum())
    assert on >= 1 and sum(counts[(L0, L0)]) == total - on and counts[(L0 + 1, L0 + 1)][0] == counts[(L0, L0)][0] + on
    assert counts[(L0 - 1, L0 - 1)][1] == counts[(L0, L0)][1] + on and counts[(-fc.I32_MAX - 1, fc.I32_MAX)] == (0, 0)


def test_invariants(sized):
    t = sized.ctx
    C = capi.C
    ev, off = t.evidence()
    data, n, coff = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
    t._check(t.L.bk_evidence(t.h, C.byref(data), C.byref(n), C.byref(coff)))  # the library's own buffers, looked at again below
    before = [t.fetch(st)[0] for st in STAGES]
    a = sized.check(sized.sites())
    b = sized.check(sized.sites())
    assert a.tobytes() == b.tobytes() and not a["n_lost"].any()
    for x, y in zip(before, [t.fetch(st)[0] for st in STAGES]):
        assert np.array_equal(x, y)
    buf = (C.c_char * (n.value * abi.EVIDENCE.itemsize)).from_address(data.value)
    assert np.frombuffer(buf, dtype=abi.EVIDENCE, count=n.value).tobytes() == ev.tobytes()
    assert np.ctypeslib.as_array(coff, shape=(len(sized.cl) + 1,)).tobytes() == off.tobytes()
    ev2, off2 = t.evidence()
    assert ev2.tobytes() == ev.tobytes() and off2.tobytes() == off.tobytes()


# ---- 3. pile-ups at the mate's position -----------------------------------------------------------------------------------------------------------
PILE = [("alone", 0, "front"), ("k63_last", 63, "front"), ("k63_first", 63, "behind"), ("k64_last", 64, "front"), ("k64_first", 64, "behind"), ("k65_last", 65, "front"),
        ("k65_first", 65, "behind"), ("big", 1100, "around"), ("tail", 0, "front")]  # (the stages drop some pairs of a group's last cluster)
PILE_PAIRS = 6


def pile_sample():
    """more records than 64 strides of the sampled keys.  Per locus PILE_PAIRS pairs whose reverse mates all start at one position X, and
    fillers there too (mapq 0: no stage takes them): records of the mates' flag and another name, so that a wanted record shares (tid, pos)
    with K others.  In front of every mate stands a record of its own name and position with another flag.  `front` puts the fillers in
    front of the mates (the wanted records come last), `behind` behind them; `around` splits them, and the table is padded so that the
    first mate of that locus is record 1023 of its stride and the second one record 0 of the next"""
    ds = synth.Dataset(list(cc.CONTIGS))
    background(ds, 33_000, 44)
    rng = np.random.default_rng(45)
    marks = {}
    for k, (name, K, where) in enumerate(PILE):
        bpa, X = 500_000 + 30_000 * k, 1_000_000 + 30_000 * k
        fillers = [synth.Rec("f%s_%d" % (name, i), REV2, 1, X, 0, "100M", 0, bpa, 0) for i in range(max(K - (PILE_PAIRS - 1), 0))]
        mates, heads = [], []
        for j in range(PILE_PAIRS):
            q = "%s_%d" % (name, j)
            a, b = pair(q, 0, bpa - int(rng.integers(100, 400)), "100M", False, 1, X, CIGARS[j % len(CIGARS)], True)
            heads.append(a)
            mates += [synth.Rec(q, REV2 | 0x400, 1, X, 0, "55M", 0, a.pos, 0), b]  # the same name and position, another flag, in front
        n_front = {"front": len(fillers), "behind": 0, "around": len(fillers) // 2}[where]
        marks[name] = mates[1]
        ds.recs += heads + fillers[:n_front] + mates + fillers[n_front:]
    ds.sort()
    at = next(i for i, r in enumerate(ds.recs) if r is marks["big"])
    n_pad = (1023 - at) % fc.SAMPLE_STRIDE
    ds.recs += [synth.Rec("pad%d" % i, FWD1, 0, 5, 0, "100M", 0, 5, 0) for i in range(n_pad)]
    ds.sort()
    return ds, marks


@pytest.fixture(scope="module")
def piles():
    ds, marks = pile_sample()
    r = Run(ds)
    r.recs, r.marks = ds.recs, marks
    yield r
    r.close()


def test_pile_ups_at_the_mates_position(piles):
    cols = piles.cols
    assert len(cols["tid"]) >= 64 * fc.SAMPLE_STRIDE  # the sampled keys are in use
    at = {name: next(i for i, r in enumerate(piles.recs) if r is m) for name, m in piles.marks.items()}
    assert at["big"] % fc.SAMPLE_STRIDE == fc.SAMPLE_STRIDE - 1
    assert piles.recs[at["big"] + 2].qname == "big_1" and (at["big"] + 2) % fc.SAMPLE_STRIDE == 1  # (its other-flag record is record 0 of the stride)
    run_len = {}
    for name, K, where in PILE:
        X = piles.marks[name].pos
        same = np.flatnonzero((cols["tid"] == 1) & (cols["pos"] == X))
        run_len[name] = len(same)
        assert len(same) == max(K - (PILE_PAIRS - 1), 0) + 2 * PILE_PAIRS
        first_mate = at[name] - int(same[0])
        assert first_mate == {"front": len(same) - 2 * PILE_PAIRS + 1, "behind": 1, "around": (len(same) - 2 * PILE_PAIRS) // 2 + 1}[where]
    assert run_len["big"] > fc.SAMPLE_STRIDE and run_len["k64_last"] > 64 > fc.LANE_WALK
    by_call = {}
    for c in range(len(piles.cl)):
        for name, K, where in PILE:
            if piles.cl[c]["p2_min"] == piles.marks[name].pos + 1 == piles.cl[c]["p2_max"]:
                by_call[name] = c
    assert set(by_call) == {name for name, _, _ in PILE}
    got = piles.check(piles.sites())
    for name, c in by_call.items():
        assert int(got[c]["n_used"]) == piles.n_pair[c] >= (PILE_PAIRS if name != "tail" else 1), (name, got[c])
    # the mates' CIGARs differ, so a walk that stopped at a neighbour of equal flag shows as another length
    assert all(int(got[c]["max"]) - int(got[c]["min"]) >= 100 for name, c in by_call.items() if name != "tail")
    piles.check(piles.sites(rights=(0, 1), at=(piles.cl["p1_max"] + 150, piles.cl["p2_min"])), brute=False)


# ---- 4. a seeded sample -----------------------------------------------------------------------------------------------------------------------------
def test_seeded_sample_against_the_brute_force_statement():
    """120 000 records, 300 loci: every call against the vectorised statement, every seventh against the brute-force one"""
    ds, cols = cc.call_dataset("cfg")
    r = Run(ds, cols=cols)
    assert len(cols["tid"]) >= 100_000 and len(r.cl) >= 250
    sites = r.sites()
    got = r.check(sites, brute=False)
    assert int(got["n_used"].sum()) > 2000
    flipped = sites.copy()
    flipped["right1"][::3] ^= 1
    flipped["right2"][1::3] ^= 1
    assert int(r.check(flipped, brute=False)["n_off"].sum()) > 1000
    some = sites.copy()
    some["skip"] = (np.arange(len(sites)) % 7 != 0).astype(np.uint8)
    r.check(some)
    exact = sites.copy()
    voted = (r.cl["flags"] & 2) != 0
    exact["pos1"], exact["pos2"], exact["skip"] = r.cl["p1_exact"], r.cl["p2_exact"].astype(np.uint32), (~voted).astype(np.uint8)
    assert voted.sum() >= 100
    r.check(exact, brute=False)
    r.close()


# ---- 5. table forms, refusals, timing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "device_side", "exclude_host", "decode_ctx"])
def test_fragment_sizes_table_forms(form):
    import torch
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
        cols = {k: dcols[k].cpu().numpy().view(dt) for k, dt in (("tid", np.int32), ("pos", np.int32), ("flag", np.uint16), ("qhash", np.uint64), ("cigar_off", np.uint32),
                                                                   ("cigar", np.uint32))}
        cols["cigar"] = cols["cigar"][:int(dcols["n_cigar_words"])]
        cols["cigar_off"] = cols["cigar_off"][:int(dcols["n"]) + 1]
    elif form == "decode_ctx":
        ds = cigar_sample()
        cols = ds.to_soa()
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        ds = cc.designed_tumor()
        cols = ds.to_soa()
        t, hold = cc.make_ctx(ds.contigs, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            assert t.exclude_regions(*cc.EXCLUDE) > 0
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, *cc.EXCLUDE))  # the table the context searches holds the kept records
    w, n_valid = t.run(qual=QUAL, fast=True)
    r = Run(cols=cols, ctx=t)
    assert len(r.cl) >= 4
    got = r.check(r.sites(), brute=form != "device_side")
    assert int(got["n_used"].sum()) >= 40
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


def test_fragment_sizes_call_order_and_refusals():
    ds = cigar_sample()
    cols = ds.to_soa()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    four = np.zeros(4, abi.FRAG_SITE)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.fragment_sizes(four, 0, 10)
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    t.mask_and_cluster(w, True)
    t.split_evidence()
    t.cluster_summary(w)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints") as e:
        t.fragment_sizes(four, 0, 10)
    assert e.value.code == abi.BK_ERR_ARG
    t.split_breakpoints(w)
    r = Run(cols=cols, ctx=t)  # (it needs no earlier bk_evidence call: Run asks for the rows, the check below answers from buffers of its own)
    assert len(r.cl) == 4
    sites = r.sites()
    r.check(sites)
    C = capi.C
    out = C.c_void_p()
    f = t.L.bk_fragment_sizes
    assert f(t.h, sites.ctypes.data, 4, 0, 10, None) == abi.BK_ERR_ARG and b"null out" in t.L.bk_last_error(t.h)
    assert f(t.h, None, 4, 0, 10, C.byref(out)) == abi.BK_ERR_ARG and b"null sites" in t.L.bk_last_error(t.h)
    assert f(None, sites.ctypes.data, 4, 0, 10, C.byref(out)) == abi.BK_ERR_ARG
    for n in (0, 3, 5):
        assert f(t.h, np.zeros(8, abi.FRAG_SITE).ctypes.data, n, 0, 10, C.byref(out)) == abi.BK_ERR_ARG and b"sites for 4 clusters" in t.L.bk_last_error(t.h)
    assert f(t.h, sites.ctypes.data, 4, 11, 10, C.byref(out)) == abi.BK_ERR_ARG and b"lo above hi" in t.L.bk_last_error(t.h)
    assert f(t.h, sites.ctypes.data, 4, 10, 10, C.byref(out)) == abi.BK_OK
    for field, value, word in (("right1", 2, b"above 1"), ("right2", 255, b"above 1"), ("skip", 2, b"above 1"), ("reserved", 1, b"reserved")):
        for k in (0, 3):
            bad = sites.copy()
            if field == "reserved":
                bad[k]["reserved"][4 if k else 0] = value
            else:
                bad[k][field] = value
            assert f(t.h, bad.ctypes.data, 4, 0, 10, C.byref(out)) == abi.BK_ERR_ARG and word in t.L.bk_last_error(t.h), (field, k)
    r.check(sites)  # a refusal leaves the context usable
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.fragment_sizes(four, 0, 10)
    assert e.value.code == abi.BK_ERR_ARG
    t.close()
    s.close()


def test_fragment_sizes_is_timed():
    ds = cigar_sample()
    t = capi.Context(ds.contigs)
    t.upload(ds.to_soa())
    t.timing_enable(True)
    t.run(qual=QUAL, fast=True)
    r = Run(cols=ds.to_soa(), ctx=t)
    sites = r.sites()
    sites[1]["right1"] ^= 1  # one call off
    got = t.fragment_sizes(sites, r.lo, r.hi)
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "fragment_sizes" in tm and tm["fragment_sizes"][0] > 0 and tm["fragment_sizes"][1] > 0
    n_rows, used = int(r.n_pair.sum()), int(got["n_used"].sum())
    assert n_rows >= 40 and used == n_rows - int(r.n_pair[1]) and int(got["n_off"].sum()) == int(r.n_pair[1])
    own = fc.touched_rows(n_rows, 2 * used, 2 * used, used, len(sites))  # every looked-up record is found by a walk of one record here
    assert own == n_rows * 120 + 2 * used * (80 + 18 + 8) + 4 * 80
    assert own < touched["fragment_sizes"] < own + 200 * n_rows + 1000 * len(sites)  # the rest is the listing's, as bk_evidence models it
    t.close()


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------------------
FG_INFO = ("##INFO=<ID=FGN,Number=1,Type=Integer,", "##INFO=<ID=FGMEAN,Number=1,Type=Float,", "##INFO=<ID=FGZ,Number=1,Type=Float,")
# (name, ta, bpa, tb, bpb): side A keeps its left, side B its right; the lengths of their pairs are designed below
FG_LOCI = [("library", 0, 300_000, 1, 700_000), ("inserted", 0, 1_000_000, 0, 1_400_000), ("stacked", 1, 1_700_000, 3, 1_700_000)]
INSERTION = 100


def cli_sample():
    """background; three voted calls (pairs plus split reads) whose pairs have the library's own lengths, lengths short by INSERTION, and one
    length; and three loci of callcases with other sides, their pairs as designed_tumor draws them"""
    rng = np.random.default_rng(47)
    ds = synth.Dataset(list(cc.CONTIGS))
    background(ds, 12_000, 46)
    for name, ta, bpa, tb, bpb in FG_LOCI:
        for j in range(14):
            L = {"library": int(round(rng.normal(350, 40))), "inserted": int(round(rng.normal(350, 40))) - INSERTION, "stacked": 352}[name]
            L = max(L, 200)
            a1 = int(rng.integers(100, L - 99)) if name != "stacked" else 170 + j
            a2 = L - a1
            ds.recs += pair("%sD_%d" % (name, j), ta, bpa - a1, "100M", False, tb, bpb + a2 - 101, "100M", True)
        for j in range(8):
            ds.recs += cc.designed_split("%sS_%d" % (name, j), ta, bpa, "L", tb, bpb, "R")
    for name, ta, bpa, da, tb, bpb, db in cc.LOCI[1:4]:
        for j in range(14):
            oa = -int(rng.integers(100, 400)) if da == "L" else int(rng.integers(0, 300))
            ob = -int(rng.integers(100, 400)) if db == "L" else int(rng.integers(0, 300))
            ds.recs += synth._discordant_pair("%sD_%d" % (name, j), ta, bpa + oa, tb, bpb + ob, 100, rev_a=(da == "R"), rev_b=(db == "R"))
        for j in range(8):
            ds.recs += cc.designed_split("%sS_%d" % (name, j), ta, bpa, da, tb, bpb, db)
    ds.sort()
    return ds


def outputs(tmp, prefix):
    return sorted(f[len(prefix):] for f in os.listdir(tmp) if f.startswith(prefix + "_"))


@pytest.mark.parametrize("variant", ["plain", "all_vcf"])
def test_cli_fragsize(variant):
    ds = cli_sample()
    cols = ds.to_soa()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(ds, tb)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        extra = ["-fast"] + (["-all", "-vcf"] if variant != "plain" else [])
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        ra = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
        assert ra.returncode == 0, ra.stderr[-2000:]
        rb = subprocess.run(base + ["-o", b, "-fragsize"], env=env, capture_output=True, text=True)
        assert rb.returncode == 0, rb.stderr[-2000:]
        r = subprocess.run([BIN, "-i", tb, "-n", side["nib"], "-fast", "-o", os.path.join(tmp, "c"), "-fragsize", "-gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-fragsize cannot be combined with -gpus" in r.stderr and not outputs(tmp, "c"), r.stderr[-2000:]
        # the API on the same table: the sites the command line builds, and the definition on them
        run = Run(ds, cols=cols)
        cl, jn = run.cl, run.ctx.junctions()
        last = "_fusion_all.txt" if variant != "plain" else "_fusion.txt"
        calls = written_calls(cl, b + last)
        sites = np.zeros(len(cl), abi.FRAG_SITE)
        sites["skip"] = 1
        for i in calls:
            r1, r2, _ = capi.junction_sides(jn[i])
            sites[i]["pos1"], sites[i]["pos2"], sites[i]["right1"], sites[i]["right2"], sites[i]["skip"] = cl[i]["p1_exact"], cl[i]["p2_exact"], r1, r2, 0
        rows = run.check(sites)
        mean, sd, lo, hi = run.mean, run.sd, run.lo, run.hi
        run.close()
        # 1. the files: the twins are new, params / performance (and the VCF) change, every other file is byte-identical
        twins = ["_fusion_fragsize.txt"] + (["_fusion_all_fragsize.txt"] if variant != "plain" else [])
        fa, fb = outputs(tmp, "a"), outputs(tmp, "b")
        assert fb == sorted(fa + twins), (fa, fb)
        changed = {"_params.txt", "_performance.txt"} | ({"_fusion.vcf"} if variant != "plain" else set())
        for suffix in fa:
            if suffix not in changed:
                assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
        pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
        assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "fragsize\n", (pa, pb)
        line = "fragsize: %d calls, %d pairs used, %d off the junction's sides, library %d-%d" % (len(calls), rows["n_used"].sum(), rows["n_off"].sum(), lo, hi)
        assert line in rb.stdout.split("\n") and "fragsize" not in ra.stdout and "Warning" not in rb.stderr, rb.stdout[-2000:]
        # 2. the twins: the rows of their fusion table in its order, and the nine columns of the call's row
        for twin in twins:
            plain = twin.replace("_fragsize", "")
            lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
            assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(fc.FRAG_NAMES)
            here = written_calls(cl, b + plain)
            assert len(here) == len(lines) - 2 and len(here) >= (1 if plain == "_fusion.txt" else 6)
            by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in here}
            for text, s in zip(lines[1:-1], src[1:-1]):
                f = text.split("\t")
                assert text == s + "\t" + "\t".join(fc.call_fields(rows[by_key[(f[1], f[2])]], mean, sd)), text
        # 3. the designed calls say what they were built to say
        named = {}
        for name, ta, bpa, tb_, bpb in FG_LOCI:
            at = cc.rows_of(cl, ta, bpa, tb_, bpb)
            if at and at[0][0] in calls:
                named[name] = rows[at[0][0]]
        if variant != "plain":
            assert set(named) == {"library", "inserted", "stacked"}
            z = {name: (float(r["sum"]) / float(r["n_used"]) - mean) / sd for name, r in named.items()}
            assert all(int(r["n_used"]) >= 10 and int(r["n_off"]) == 0 for r in named.values())
            assert abs(z["library"]) < 1 and z["inserted"] < z["library"] - 1.5 and named["stacked"]["min"] == named["stacked"]["max"] == 352
            assert int(named["stacked"]["abs_dev"]) == 0 and int(named["library"]["abs_dev"]) > 10 * int(named["library"]["n_used"])
        if variant == "plain":
            return
        # 4. the VCF: FGN (and FGMEAN / FGZ where the columns have a value) last in INFO on both breakends, their header lines
        va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
        assert len(vb) == len(va) + 3 and all(sum(l.startswith(i) for l in vb) == 1 for i in FG_INFO)
        assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(FG_INFO)]
        body_a = [l for l in va if l and not l.startswith("#")]
        body_b = [l for l in vb if l and not l.startswith("#")]
        assert len(body_a) == len(body_b) == 2 * len(calls)
        for la, lb in zip(body_a, body_b):
            x, y = la.split("\t"), lb.split("\t")
            u = rows[int(y[2][2:].split("_")[0])]
            assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + fc.info_fields(u, mean, sd), lb
        assert any(";FGZ=" in l for l in body_b)


def test_cli_fragsize_of_a_sample_without_calls():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        r = subprocess.run([BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast", "-fragsize", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_fragsize.txt", "_fusion_all_fragsize.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(fc.FRAG_NAMES) + "\n"
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in FG_INFO)
        assert open(prefix + "_params.txt").read().endswith("fragsize\n")
        assert any(l.startswith("fragsize: 0 calls, 0 pairs used, 0 off the junction's sides, library ") for l in r.stdout.split("\n"))

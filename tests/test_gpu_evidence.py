"""Evidence export (`bk_evidence`, `bk_bam_extract`, `-evidence`): every row against a numpy evaluation of its definition
(include/breakid_hip.h) over the fetched stage tables and the record columns, order and `call_off` included; the counts tied to
`bk_junctions`; the designed truth of loci whose supporting reads are known by name, one read shared between two calls; every table
form a context can hold; and the command line's two files compared with the C ABI and with the extraction rule applied to the
input."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL


# ---- the definition, in numpy -----------------------------------------------------------------------------------------------
def expected_evidence(cl, clustered, splits, qhash, qcheck, mapq):
    """(rows, call_off); qhash / qcheck / mapq: the columns of the context's table (qcheck None: the table has none).
    (the synthetic reference lists have unique names: the interned id of a header contig is its tid)"""
    key = (clustered["group"].astype(np.int64) << 32) | (clustered["cluster"].astype(np.int64) & 0xFFFFFFFF)
    ok_sp = (splits["flags"] & 2) == 0
    pb, sb = splits["prim_bp"].astype(np.int64), splits["sec_bp"].astype(np.int64)
    prim_right = (splits["prim_bp"] == splits["prim_start"]).astype(np.int64)
    sec_right = (splits["sec_bp"] == splits["sec_start"]).astype(np.int64)
    parts, off = [], [0]
    for i, c in enumerate(cl):
        m = np.flatnonzero(key == ((int(c["group"]) << 32) | (int(c["id"]) & 0xFFFFFFFF)))  # ascending BK_STAGE_CLUSTERED row
        p = clustered[m]
        r = np.zeros(len(m), abi.EVIDENCE)
        rec = p["rec"].astype(np.int64)
        r["rec"], r["qhash"] = p["rec"], qhash[rec]
        r["qcheck"] = qcheck[rec] if qcheck is not None else 0
        r["call"], r["kind"] = i, abi.EV_PAIR
        for a, b in (("tid1", "p1_tid"), ("pos1", "p1_pos"), ("tid2", "p2_tid"), ("pos2", "p2_pos"), ("flag1", "p1_flag"), ("flag2", "p2_flag"),
                     ("mapq1", "p1_mapq"), ("mapq2", "p2_mapq")):
            r[a] = p[b]
        r["sides"] = 2 * (p["p1_rev"] != 0) + (p["p2_rev"] != 0)
        parts.append(r)
        n_rows = len(r)
        if c["flags"] & 2:
            e1, e2 = int(c["p1_exact"]), int(c["p2_exact"])
            t1, t2 = int(c["p1_tid"]), int(c["p2_tid"])
            own = ((splits["tid"] == t1) | (splits["tid"] == t2)) & ok_sp
            f1 = own & (splits["prim_chr"] == t1) & (splits["sec_chr"] == t2) & (np.abs(pb - e1) <= 2) & (np.abs(sb - e2) <= 2)
            f2 = own & ~f1 & (splits["prim_chr"] == t2) & (splits["sec_chr"] == t1) & (np.abs(pb - e2) <= 2) & (np.abs(sb - e1) <= 2)
            t = np.flatnonzero(f1 | f2)  # ascending BK_STAGE_SPLITS row
            s, sw = splits[t], f2[t]
            r = np.zeros(len(t), abi.EVIDENCE)
            r["rec"], r["qhash"], r["qcheck"] = s["rec"], s["qhash"], s["qcheck"]
            r["call"], r["kind"] = i, abi.EV_SPLIT
            r["tid1"], r["tid2"] = t1, t2
            r["pos1"] = np.where(sw, s["sec_bp"], s["prim_bp"])
            r["pos2"] = np.where(sw, s["prim_bp"], s["sec_bp"])
            r["flag1"], r["flag2"] = s["flags"] & 0xFFFF, sw
            r["mapq1"] = mapq[s["rec"].astype(np.int64)]
            r["sides"] = np.where(sw, 2 * sec_right[t] + prim_right[t], 2 * prim_right[t] + sec_right[t])
            parts.append(r)
            n_rows += len(r)
        off.append(off[-1] + n_rows)
    rows = np.concatenate(parts) if parts else np.zeros(0, abi.EVIDENCE)
    return rows, np.asarray(off, np.uint64)


def check_context(t, qhash, qcheck, mapq):
    """bk_evidence of a context that has run, against the definition over its own fetched tables, and the ties to bk_junctions"""
    stages = (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)
    before = [t.fetch(st)[0] for st in stages]
    got, off = t.evidence()
    clustered, splits, cl = [t.fetch(st)[0] for st in stages]
    for a, b in zip(before, (clustered, splits, cl)):
        assert np.array_equal(a, b)  # the call changes nothing a fetch returns
    exp, exp_off = expected_evidence(cl, clustered, splits, qhash, qcheck, mapq)
    assert got.dtype == abi.EVIDENCE and off.dtype == np.uint64
    assert np.array_equal(off, exp_off), (off[:10], exp_off[:10])
    bad = [i for i in range(min(len(got), len(exp))) if got[i].tobytes() != exp[i].tobytes()]
    assert len(got) == len(exp) and not bad, (len(got), len(exp), [(got[i], exp[i]) for i in bad[:5]])
    # order: call ascending, pairs before splits
    assert np.all(np.diff(got["call"].astype(np.int64)) >= 0)
    junc = t.junctions()
    assert len(junc) == len(cl) == len(off) - 1
    for c in range(len(cl)):
        r = got[int(off[c]):int(off[c + 1])]
        assert np.all(r["call"] == c) and np.all(np.diff(r["kind"].astype(np.int64)) >= 0)
        pe, sr = r[r["kind"] == abi.EV_PAIR], r[r["kind"] == abi.EV_SPLIT]
        assert len(pe) + len(sr) == len(r) and len(pe) == int(cl[c]["n_drp"])
        assert np.array_equal(np.bincount(pe["sides"], minlength=4), junc[c]["pairs"]), c
        assert np.array_equal(np.bincount(sr["sides"], minlength=4), junc[c]["splits"]), c
    again, off2 = t.evidence()  # two calls in one process: the same bytes
    assert again.tobytes() == got.tobytes() and off2.tobytes() == off.tobytes()
    return got, off, cl


def columns(cols):
    return cols["qhash"], cols.get("qcheck"), cols["mapq"]


# ---- 1. the definition, every row ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["genotype", "edge", "cfg"])
@pytest.mark.parametrize("fast", [True, False])
def test_evidence_equals_its_definition(fast, name):
    ds, cols = cc.call_dataset(name)
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    got, off, cl = check_context(t, *columns(cols))
    if name != "edge":
        assert n_valid >= (5 if name == "genotype" else 100) and (got["kind"] == abi.EV_SPLIT).any() and (got["kind"] == abi.EV_PAIR).any()
    t.close()


@pytest.mark.parametrize("fast", [True, False])
def test_evidence_renamed_reference_list(fast):
    tum, _ = cc.tumor_normal(extra_contigs=300, names4=("chr2", "chr1", "chr3", "chr4"))
    cols = tum.to_soa()
    t = capi.Context(tum.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    # (here a header contig's interned id is not its tid: the rows are tied to bk_junctions, which is checked against its own
    # definition in test_gpu_vcf, and the pair rows to the definition)
    got, off = t.evidence()
    junc, cl = t.junctions(), t.fetch(abi.STAGE_CLUSTERS)[0]
    assert n_valid >= 3 and len(off) == len(cl) + 1 and int(off[-1]) == len(got)
    for c in range(len(cl)):
        r = got[int(off[c]):int(off[c + 1])]
        assert np.array_equal(np.bincount(r["sides"][r["kind"] == abi.EV_PAIR], minlength=4), junc[c]["pairs"])
        assert np.array_equal(np.bincount(r["sides"][r["kind"] == abi.EV_SPLIT], minlength=4), junc[c]["splits"])
    assert (got["kind"] == abi.EV_SPLIT).any()
    t.close()


# ---- 2. designed truth: the reads by name ---------------------------------------------------------------------------------------
SHARED = ("SH", 0, 300_150, "L", 2, 1_000_000, "R")  # a second call whose side A lies 150 bp from that of LOCI[0], on another contig pair
N_SHARE = 3


def shared_tumor():
    """the designed tumour of test_gpu_vcf, one more locus, and N_SHARE reads that belong to two calls: their first mate is a
    split read of SH (60M40S ending at its breakpoint on chr1, the rest on chr3) and their second mate lies on chr2 beside LOCI[0]'s
    breakpoint, so the pair is a member pair of LOCI[0]"""
    rng = np.random.default_rng(11)
    ds = cc.designed_tumor()
    name, ta, bpa, da, tb, bpb, db = SHARED
    for j in range(14):
        ds.recs += synth._discordant_pair("%sD_%d" % (name, j), ta, bpa - int(rng.integers(100, 400)), tb, bpb + int(rng.integers(0, 300)), 100, rev_a=False, rev_b=True)
    for j in range(8):
        ds.recs += cc.designed_split("%sS_%d" % (name, j), ta, bpa, da, tb, bpb, db)
    _, _, _, _, t2, bp2, _ = cc.LOCI[0]
    for j in range(N_SHARE):
        q = "SHARE_%d" % j
        pa, pb, pm = bpa - 60, bpb - 1, bp2 + 40 + 30 * j
        sa1 = "%s,%d,+,60S40M,60,0;" % (cc.NAMES[tb], pb + 1)
        sa2 = "%s,%d,+,60M40S,60,0;" % (cc.NAMES[ta], pa + 1)
        ds.recs += [synth.Rec(q, 0x1 | 0x40 | 0x20, ta, pa, 60, "60M40S", t2, pm, 0, sa=sa1),
                    synth.Rec(q, 0x1 | 0x40 | 0x20 | 0x100, tb, pb, 60, "60S40M", t2, pm, 0, sa=sa2),
                    synth.Rec(q, 0x1 | 0x80 | 0x10, t2, pm, 60, "100M", ta, pa, 0)]
    ds.sort()
    return ds


_SHARED = {}


def shared():
    if "t" not in _SHARED:
        ds = shared_tumor()
        _SHARED["t"] = (ds, ds.to_soa())
    return _SHARED["t"]


def names_of_call(got, off, c, names):
    r = got[int(off[c]):int(off[c + 1])]
    return (sorted(names[int(x)] for x in r["rec"][r["kind"] == abi.EV_PAIR]), sorted(set(names[int(x)] for x in r["rec"][r["kind"] == abi.EV_SPLIT])))


# Member pairs the reference's own stages leave of the 14 designed pairs of a locus (17 at LOCI[0]: the shared reads), counted on
# the CPU oracle (oracle/oracle.cc, the restatement of the reference): remove_isolated_pairs drops some and lists others twice
# (BK_STAGE_ISO holds 12 rows of 10 different pairs where BK_STAGE_SCAN held 14), the AHC clustering keeps those rows and the fast
# strategy drops two more.  `n_drp` counts these rows, and bk_evidence lists exactly them: rows, different pairs.
KEPT = {True: {"LR_x": (13, 11), "LL_x": (14, 13), "RR_x": (10, 9), "RL_x": (10, 8), "LR_s": (10, 8), "LL_s": (10, 8), "RR_s": (10, 8), "RL_s": (10, 8), "SH": (14, 13)},
        False: {"LR_x": (15, 13), "LL_x": (14, 13), "RR_x": (12, 11), "RL_x": (12, 10), "LR_s": (12, 10), "LL_s": (12, 10), "RR_s": (12, 10), "RL_s": (12, 10), "SH": (14, 13)}}


@pytest.mark.parametrize("fast", [True, False])
def test_designed_reads(fast):
    """The split reads listed for a designed locus are exactly its designed split reads.  The pairs listed are exactly the designed
    pairs that the stages before left in the call's cluster, each as often as the cluster holds it: every designed pair is in
    BK_STAGE_SCAN once, a designed pair that is not listed is in no row of BK_STAGE_CLUSTERED (the isolation and clustering stages
    took it out, not the listing), the listed names are those of the cluster's rows in the CPU oracle's BK_STAGE_CLUSTERED, and
    their number is the one recorded from the oracle in KEPT."""
    from collections import Counter
    from oracle import pyoracle
    ds, cols = shared()
    names = [r.qname for r in ds.recs]
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.run(qual=QUAL, fast=fast)
    got, off, cl = check_context(t, *columns(cols))
    scan, clustered = t.fetch(abi.STAGE_SCAN)[0], t.fetch(abi.STAGE_CLUSTERED)[0]
    o = pyoracle.Oracle(ds.contigs, {k: v for k, v in cols.items() if k != "target_len"})
    o.run(QUAL, fast=fast)
    o_cl, o_clustered = o.fetch(abi.STAGE_CLUSTERS)[0], o.fetch(abi.STAGE_CLUSTERED)[0]
    o.close()
    assert np.array_equal(cl, o_cl)
    in_scan = Counter(names[int(x)] for x in scan["rec"])
    in_clustered = Counter(names[int(x)] for x in clustered["rec"])
    for k in range(len(got)):  # a row's hashes are those of the read it names
        n = names[int(got["rec"][k])].encode()
        assert int(got["qhash"][k]) == capi.lib().bk_qname_hash(n, len(n)) and int(got["qcheck"][k]) == capi.lib().bk_qname_check(n, len(n))
    share = ["SHARE_%d" % j for j in range(N_SHARE)]
    calls_of_share = set()
    for name, ta, bpa, da, tb, bpb, db in cc.LOCI + [SHARED]:
        rows = cc.rows_of(cl, ta, bpa, tb, bpb)
        assert rows, "locus %s is not called" % name
        pe_exp = sorted(["%sD_%d" % (name, j) for j in range(14)] + (share if name == cc.LOCI[0][0] else []))
        sr_exp = sorted(["%sS_%d" % (name, j) for j in range(8)] + (share if name == SHARED[0] else []))
        pe_all, sr_all, kept = [], set(), []
        for i, _ in rows:
            pe, sr = names_of_call(got, off, i, names)
            print(name, "fast" if fast else "default", "call", i, "PE", len(pe), "different", len(set(pe)), "SR", len(sr))
            pe_all += pe
            sr_all |= set(sr)
            m = (o_clustered["group"] == o_cl[i]["group"]) & (o_clustered["cluster"] == o_cl[i]["id"])
            kept += [names[int(x)] for x in o_clustered["rec"][m]]
            if set(share) & (set(pe) | set(sr)):
                calls_of_share.add(i)
        assert all(in_scan[n] == 1 for n in pe_exp), (name, [n for n in pe_exp if in_scan[n] != 1])  # the scan found every designed pair, once
        assert set(pe_all) <= set(pe_exp), (name, pe_all)                                  # no read that was not designed for this locus
        assert sorted(pe_all) == sorted(kept), (name, pe_all, kept)                          # exactly the cluster's rows, by the CPU oracle
        assert (len(pe_all), len(set(pe_all))) == KEPT[fast][name], (name, len(pe_all), len(set(pe_all)))
        missing = [n for n in pe_exp if n not in pe_all]
        assert all(in_clustered[n] == 0 for n in missing), (name, missing)                   # a pair not listed is in no cluster at all
        assert all(in_clustered[n] == c for n, c in Counter(pe_all).items()), name           # a pair listed twice is in the table twice
        assert sorted(sr_all) == sr_exp, (name, sr_all)
        if name == cc.LOCI[0][0]:
            share_as_pair = set(pe_all) & set(share)
    assert len(calls_of_share) == 2 and share_as_pair  # a shared read is a member pair of one call and a split read of the other
    t.close()


# ---- 2b. the order of the calls: a reference list whose numeric and lexicographic group orders differ ---------------------------
ORDER_CONTIGS = [("chr1", 2_000_000), ("chr2", 2_000_000), ("chr10", 2_000_000)]
# One locus per chromosome pair, one on chr1 alone and one on chr2 alone.  A record on the third contig carries the id of "chr3" for
# its own side (the reference's chromID2ChrName of its tid), so the two tuples of a split read there never agree: the loci on chr10
# get clusters but no vote, on the CPU oracle too.  The locus on chr2 is there so that three groups hold a voted cluster.
ORDER_LOCI = [("x1_2", 0, 300_000, "L", 1, 700_000, "R"), ("x1_10", 0, 900_000, "L", 2, 500_000, "L"), ("x2_10", 1, 1_300_000, "R", 2, 1_200_000, "R"),
              ("s1", 0, 1_400_000, "L", 0, 1_800_000, "R"), ("s2", 1, 300_000, "R", 1, 1_000_000, "L")]
_ORDER = {}


def order_tumor():
    if "t" not in _ORDER:
        ds = cc.designed_tumor(mix=False, contigs=ORDER_CONTIGS, loci=ORDER_LOCI, n_proper=4000)
        _ORDER["t"] = (ds, ds.to_soa())
    return _ORDER["t"]


@pytest.mark.parametrize("fast", [True, False])
def test_per_call_outputs_where_group_orders_differ(fast):
    """Groups in numeric key order: chr1_chr1, chr1_chr2, chr1_chr10, chr2_chr2, chr2_chr10; in BK_STAGE_CLUSTERS order (the
    reference's std::map<string>): chr1_chr1, chr1_chr10, chr1_chr2, chr2_chr10, chr2_chr2.  Every row of the four per-call
    outputs must be the row of its definition over the fetched clusters, with a normal made of the tumour's own records."""
    ds, cols = order_tumor()
    names = [n for n, _ in ds.contigs]
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    cl, _ = t.fetch(abi.STAGE_CLUSTERS)
    # the fixture's own condition
    keys = sorted({(int(c["p1_tid"]), int(c["p2_tid"])) for c in cl})
    lexicographic = sorted(keys, key=lambda k: names[k[0]] + "_" + names[k[1]])
    voted_keys = {(int(c["p1_tid"]), int(c["p2_tid"])) for c in cl if c["flags"] & 2}
    assert len(voted_keys) >= 3, voted_keys
    assert keys != lexicographic, keys
    assert any(keys.index(k) != lexicographic.index(k) for k in voted_keys)  # a voted call moves between the two orders
    row_keys = [(int(c["p1_tid"]), int(c["p2_tid"])) for c in cl]
    assert row_keys == sorted(row_keys, key=lexicographic.index)
    # the four outputs, every row
    n = capi.Context(ds.contigs)
    n.upload(cols)
    n.isize_stats()
    n.discordant_pairs(QUAL, w)
    n.split_evidence()
    got = t.normal_support(n, w)
    exp = cc.expected_support(cl, n.fetch(abi.STAGE_SCAN)[0], n.fetch(abi.STAGE_SPLITS)[0], cols, w)
    assert got.dtype == abi.NORMAL_SUPPORT and len(got) == len(cl)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, [(cl[i], got[i], exp[i]) for i in bad[:5]]
    assert got["n_sr"].any() and got["n_drp"].all()  # (the normal is the tumour: every call finds its own pairs)
    for records, anchor in ((t, 0), (t, 10), (n, 10)):
        ref = t.ref_support(records, QUAL, anchor, w)
        exp = cc.expected_ref_support(cl, cols, QUAL, anchor, w)
        assert ref.dtype == abi.REF_SUPPORT and len(ref) == len(cl)
        bad = np.nonzero(ref != exp)[0]
        assert len(bad) == 0, [(cl[i], ref[i], exp[i]) for i in bad[:5]]
    junc = t.junctions()
    exp = cc.expected_junctions(cl, t.fetch(abi.STAGE_CLUSTERED)[0], t.fetch(abi.STAGE_SPLITS)[0])
    assert junc.dtype == abi.JUNCTION and len(junc) == len(cl)
    bad = [i for i in range(len(cl)) if junc[i].tobytes() != exp[i].tobytes()]
    assert not bad, [(cl[i], junc[i], exp[i]) for i in bad[:5]]
    assert np.array_equal(junc["splits"].astype(np.int64).sum(1), got["n_sr"].astype(np.int64))  # (the normal is the tumour)
    rows, off, _ = check_context(t, *columns(cols))  # bk_evidence against expected_evidence, call_off against the rows
    assert junc["splits"].any() and (rows["kind"] == abi.EV_SPLIT).any()
    assert np.array_equal(t.fetch(abi.STAGE_CLUSTERS)[0], cl)
    t.close()
    n.close()


# ---- 3. table forms, call order, errors -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "host_no_qcheck", "device", "device_side", "exclude_host", "exclude_device", "decode_ctx"])
def test_evidence_table_forms(form):
    import torch
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
        cols = {"qhash": dcols["qhash"].cpu().numpy().view(np.uint64), "mapq": dcols["mapq"].cpu().numpy().view(np.uint8)}
        if "qcheck" in dcols:
            cols["qcheck"] = dcols["qcheck"].cpu().numpy().view(np.uint32)
    elif form == "decode_ctx":
        ds, cols = shared()
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        ds, cols = shared()
        t, hold = cc.make_ctx(ds.contigs, cols, "device" if form.endswith("device") else "host", qcheck=form != "host_no_qcheck")
        if form == "host_no_qcheck":
            cols = {k: v for k, v in cols.items() if k != "qcheck"}
        if form.startswith("exclude"):
            assert t.exclude_regions(*cc.EXCLUDE) > 0
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, *cc.EXCLUDE))  # `rec` numbers the kept records
    w, n_valid = t.run(qual=QUAL, fast=True)
    assert n_valid > 0
    got, off, cl = check_context(t, *columns(cols))
    assert (got["kind"] == abi.EV_SPLIT).any()
    if form == "host_no_qcheck":
        assert not got["qcheck"].any()
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


def test_evidence_call_order_and_errors():
    ds, cols = shared()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.evidence()
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    t.mask_and_cluster(w, True)
    t.split_evidence()
    t.cluster_summary(w)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints") as e:
        t.evidence()
    assert e.value.code == abi.BK_ERR_ARG
    t.split_breakpoints(w)
    check_context(t, *columns(cols))
    C = capi.C
    data, n, off = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
    assert t.L.bk_evidence(t.h, None, C.byref(n), C.byref(off)) == abi.BK_ERR_ARG and b"null output" in t.L.bk_last_error(t.h)
    assert t.L.bk_evidence(t.h, C.byref(data), None, C.byref(off)) == abi.BK_ERR_ARG
    assert t.L.bk_evidence(t.h, C.byref(data), C.byref(n), None) == abi.BK_ERR_ARG
    assert t.L.bk_evidence(None, C.byref(data), C.byref(n), C.byref(off)) == abi.BK_ERR_ARG
    # the other mode on the same context: the rows follow the new clusters once the stages have run again
    t.mask_and_cluster(w, False)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.evidence()
    t.cluster_summary(w)
    t.split_breakpoints(w)
    check_context(t, *columns(cols))
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.evidence()
    assert e.value.code == abi.BK_ERR_ARG
    t.close()
    s.close()


def test_evidence_of_a_context_without_clusters():
    tum = cc.quiet_tumor()
    t = capi.Context(tum.contigs)
    t.upload(tum.to_soa())
    t.run(qual=QUAL, fast=True)
    assert len(t.fetch(abi.STAGE_CLUSTERS)[0]) == 0
    got, off = t.evidence()
    assert got.dtype == abi.EVIDENCE and len(got) == 0 and off.tolist() == [0]
    t.close()


def test_evidence_is_timed():
    ds, cols = shared()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.timing_enable(True)
    t.run(qual=QUAL, fast=True)
    t.junctions()
    got, off = t.evidence()
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "evidence" in tm and "junctions" in tm and tm["evidence"][0] > 0 and tm["evidence"][1] > 0
    assert touched["evidence"] >= len(got) * abi.EVIDENCE.itemsize
    t.close()


# ---- 4. command line ----------------------------------------------------------------------------------------------------------
HEADER = "Call\tKind\tRead\tChr1\tPos1\tChr2\tPos2\tSides\tFlag1\tFlag2\tMapq1\tMapq2\tRecord"


def assert_other_files_identical(a, b, tmp):
    """every file of run `a` is in run `b`, byte-identical but for the prefix in _params.txt, its new last line and the timings of
    _performance.txt; run `b` has two more files"""
    fa = sorted(f[len("a"):] for f in os.listdir(tmp) if f.startswith("a_"))
    fb = sorted(f[len("b"):] for f in os.listdir(tmp) if f.startswith("b_"))
    assert fb == sorted(fa + ["_evidence.txt", "_evidence.bam"]) and "_fusion.txt" in fa and "_params.txt" in fa, (fa, fb)
    for suffix in fa:
        if suffix == "_params.txt":
            pa, pb = open(a + suffix).read(), open(b + suffix).read()
            assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "evidence\t1\n", (pa, pb)
        elif suffix == "_performance.txt":
            xa, xb = open(a + suffix).read().split("\n"), open(b + suffix).read().split("\n")
            assert xa[0] == xb[0] and xa[1].split("\t")[:5] == xb[1].split("\t")[:5]
        else:
            assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix


def written_calls(cl, fusion_path):
    """rows of BK_STAGE_CLUSTERS that the fusion table of the run holds (as test_gpu_vcf matches them)"""
    table = set((f[1], f[2], f[7], f[8]) for f in cc.fusion_rows(fusion_path))
    out = [i for i, c in enumerate(cl) if c["flags"] & 2 and
           (cc.NAMES[c["p1_tid"]] + ":%d" % c["p1_exact"], cc.NAMES[c["p2_tid"]] + ":%d" % c["p2_exact"], str(c["n_drp"]), str(c["n_sr"])) in table]
    assert len(set((cc.NAMES[cl[i]["p1_tid"]], int(cl[i]["p1_exact"]), cc.NAMES[cl[i]["p2_tid"]], int(cl[i]["p2_exact"]), int(cl[i]["n_drp"]), int(cl[i]["n_sr"]))
                   for i in out)) == len(table)
    return out


def check_cli_outputs(prefix, bam_path, ds, cols, fast, with_x, fusion_path):
    """the txt against bk_evidence on the same table with the test's own names; the BAM against the extraction rule on the input"""
    names = [r.qname for r in ds.recs]
    t = capi.Context(ds.contigs)
    t.upload(cols)
    kept_names = names
    if with_x:
        keep = ~cc.excluded_mask(cols, *cc.EXCLUDE)
        t.exclude_regions(*cc.EXCLUDE)
        kept_names = [n for n, k in zip(names, keep) if k]
    t.run(qual=QUAL, fast=fast)
    got, off = t.evidence()
    cl = t.fetch(abi.STAGE_CLUSTERS)[0]
    t.close()
    calls = written_calls(cl, fusion_path)
    chrom = lambda tid: "*" if tid < 0 else cc.NAMES[tid]
    exp, tags = [HEADER], {}
    for c in calls:
        for r in got[int(off[c]):int(off[c + 1])]:
            name = kept_names[int(r["rec"])]
            sides = "LR"[int(r["sides"]) >> 1] + "LR"[int(r["sides"]) & 1]
            exp.append("\t".join(["bk%d" % c, "PE" if r["kind"] == abi.EV_PAIR else "SR", name, chrom(int(r["tid1"])), str(r["pos1"]), chrom(int(r["tid2"])), str(r["pos2"]),
                                  sides, str(r["flag1"]), str(r["flag2"]), str(r["mapq1"]), str(r["mapq2"]), str(r["rec"])]))
            ids = tags.setdefault(name, [])
            if c not in ids:
                ids.append(c)
    text = open(prefix + "_evidence.txt").read()
    assert text == "\n".join(exp) + "\n", (text[:600], exp[:4])
    # the BAM: every alignment of every listed read (also inside an excluded interval), in file order, tagged with the read's calls
    sel = [i for i, n in enumerate(names) if n in tags]
    h_in, r_in = split_stream(bam_path)
    h_out, r_out = split_stream(prefix + "_evidence.bam")
    assert h_out == h_in and len(r_out) == len(sel)
    for j, i in enumerate(sel):
        tail = b"bkZ" + ",".join("bk%d" % c for c in sorted(tags[names[i]])).encode() + b"\0"
        assert r_out[j] == r_in[i] + tail, (j, i)
    assert open(prefix + "_evidence.bam", "rb").read()[-28:] == bamio._BGZF_EOF
    idx = np.asarray(sel, np.int64)
    host = capi.decode_bam(prefix + "_evidence.bam")[1]
    table = capi.decode_bam_device(prefix + "_evidence.bam")  # the GPU feed reads the file too
    dev = cc.device_cols(table)
    table.close()
    for k in cc.FIXED:
        assert np.array_equal(host[k], cols[k][idx]) and np.array_equal(dev[k], cols[k][idx]), k
    for k in ("cigar", "aux", "cigar_off", "aux_off"):
        assert np.array_equal(host[k], dev[k]), k
    return calls, tags


def split_stream(path):
    import gzip
    import struct
    d = gzip.decompress(open(path, "rb").read())
    assert d[:4] == b"BAM\1"
    p = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<i", d, p)[0] + 4
    header, recs = d[:p], []
    while p < len(d):
        bs, = struct.unpack_from("<i", d, p)
        assert bs >= 32 and p + 4 + bs <= len(d)
        recs.append(d[p + 4:p + 4 + bs])
        p += 4 + bs
    return header, recs


@pytest.mark.parametrize("variant", ["plain", "all", "across_blocks", "exclude", "normal_genotype_vcf"])
@pytest.mark.parametrize("mode", ["fast", "default"])
def test_cli_evidence(mode, variant):
    ds, cols = shared()
    with_x = variant == "exclude"
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb, bed = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "x.bed")
        cc.write_indexed(ds, tb, aligned=variant != "across_blocks")
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        extra = ["-fast"] if mode == "fast" else []
        if variant != "plain":
            extra += ["-all"]
        if variant == "normal_genotype_vcf":
            cc.designed_normal().write_bam(nb, aligned=True)
            extra += ["-normal", nb, "-genotype", "-vcf"]
        if with_x:
            with open(bed, "w") as f:
                for t, s, e in zip(*cc.EXCLUDE):
                    f.write("%s\t%d\t%d\n" % (cc.NAMES[t], s, e))
            extra += ["-x", bed]
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        r = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-o", b, "-evidence"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert_other_files_identical(a, b, tmp)
        fusion = b + ("_fusion.txt" if variant == "plain" else "_fusion_all.txt")
        calls, tags = check_cli_outputs(b, tb, ds, cols, mode == "fast", with_x, fusion)
        assert len(calls) >= (4 if variant == "plain" else 9)
        if variant != "plain":
            assert any(len(v) == 2 for v in tags.values())  # the shared reads carry two call ids
        if variant == "all":
            c = os.path.join(tmp, "c")  # two runs give the same bytes
            r = subprocess.run(base + ["-o", c, "-evidence"], env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            for suffix in ("_evidence.txt", "_evidence.bam"):
                assert open(c + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix


def test_cli_evidence_of_a_sample_without_calls_and_errors():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        r = subprocess.run(base + ["-evidence", "-gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-evidence cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-evidence"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(prefix + "_evidence.txt").read() == HEADER + "\n"
        h_in, _ = split_stream(tb)
        assert split_stream(prefix + "_evidence.bam") == (h_in, [])
        assert open(prefix + "_params.txt").read().endswith("evidence\t1\n")
        assert capi.decode_bam(prefix + "_evidence.bam")[0] == tum.contigs

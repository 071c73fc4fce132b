"""Unique support (`bk_unique_support`, `-dedup`): the counts and `first` against the numpy definition (tests/dedupcases.py) over the
fetched stage tables, byte for byte, on the seeded datasets, on designed duplicates, on fragments whose keys differ in one field
alone and on a call deeper than the implementation's tiles; every table form; call order and errors; and the command line's files
against the C ABI."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import callcases as cc
from tests import dedupcases as dc
from tests.test_gpu_evidence import written_calls

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
STAGES = (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)


def check_context(t, cols):
    """bk_unique_support of a context that has run, against the definition over its own fetched tables"""
    ev, off = t.evidence()
    C = capi.C
    data, n, coff = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
    t._check(t.L.bk_evidence(t.h, C.byref(data), C.byref(n), C.byref(coff)))  # the library's own buffers, looked at again below
    before = [t.fetch(st)[0] for st in STAGES]
    rows, first = t.unique_support()
    clustered, splits, cl = [t.fetch(st)[0] for st in STAGES]
    for a, b in zip(before, (clustered, splits, cl)):
        assert np.array_equal(a, b)  # the call changes nothing a fetch returns
    if n.value:  # bk_evidence's buffers are still there and unchanged
        buf = (C.c_char * (n.value * abi.EVIDENCE.itemsize)).from_address(data.value)
        assert np.frombuffer(buf, dtype=abi.EVIDENCE, count=n.value).tobytes() == ev.tobytes()
    assert np.ctypeslib.as_array(coff, shape=(len(cl) + 1,)).tobytes() == off.tobytes()
    exp, exp_first = dc.expected_unique_support(cl, clustered, splits, cols)
    assert rows.dtype == abi.UNIQUE_SUPPORT and first.dtype == np.uint64 and len(first) == len(ev)
    bad = [i for i in range(min(len(rows), len(exp))) if rows[i].tobytes() != exp[i].tobytes()]
    assert len(rows) == len(exp) and not bad, (len(rows), len(exp), [(cl[i], rows[i], exp[i]) for i in bad[:5]])
    assert first.tobytes() == exp_first.tobytes(), np.flatnonzero(first != exp_first)[:10]
    dc.check_invariants(ev, off, rows, first)
    again, first2 = t.unique_support()  # two calls in one process: the same bytes
    assert again.tobytes() == rows.tobytes() and first2.tobytes() == first.tobytes()
    only = t.unique_support(listing=False)  # the counts alone
    assert only.tobytes() == rows.tobytes()
    return rows, first, ev, off, cl


def run_context(ds, cols, fast):
    t = capi.Context(ds.contigs)
    t.upload(cols)
    w, n_valid = t.run(qual=QUAL, fast=fast)
    return t, n_valid


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["genotype", "edge", "cfg"])
@pytest.mark.parametrize("fast", [True, False])
def test_unique_support_equals_its_definition(fast, name):
    ds, cols = cc.call_dataset(name)
    t, n_valid = run_context(ds, cols, fast)
    rows, first, ev, off, cl = check_context(t, cols)
    if name != "edge":
        assert n_valid >= (5 if name == "genotype" else 100) and rows["uniq_splits"].any()
    if name == "cfg":
        assert (first != np.arange(len(first))).any()  # the stages keep some pairs twice, a read gives two tuples
    t.close()


@pytest.mark.parametrize("fast", [True, False])
def test_designed_duplicates(fast):
    """every locus of dedup_tumor is voted at its designed breakpoints with 16 tuples of 5 split-read fragments, the largest of 6
    tuples (3 copies of a read, two tuples each); the pair rows are what isolation and clustering keep: through the definition"""
    ds, cols = dc.dedup_tumor()
    t, n_valid = run_context(ds, cols, fast)
    rows, first, ev, off, cl = check_context(t, cols)
    for name, ta, bpa, da, tb, bpb, db in cc.LOCI:
        at = cc.rows_of(cl, ta, bpa, tb, bpb)
        assert len(at) == 1, name
        r = rows[at[0][0]]
        n_split_rows = int((ev["kind"][int(off[at[0][0]]):int(off[at[0][0] + 1])] == abi.EV_SPLIT).sum())
        assert (n_split_rows, int(r["uniq_splits"]), int(r["top_splits"])) == (16, 5, 6), (name, r)
        assert r["uniq_pairs"] < cl[at[0][0]]["n_drp"] and r["top_pairs"] >= 2, (name, r)
    t.close()


@pytest.mark.parametrize("fast", [True, False])
def test_near_keys_stay_apart(fast):
    ds, cols = dc.near_key_tumor()
    t, n_valid = run_context(ds, cols, fast)
    rows, first, ev, off, cl = check_context(t, cols)
    assert n_valid == 1 and dc.NEAR_REQUIRED <= dc.fields_differing_alone(cl, *[t.fetch(st)[0] for st in STAGES[:2]], cols)
    assert int(rows[0]["uniq_splits"]) == 5 and int(rows[0]["top_splits"]) == 4
    t.close()


def test_deep_call():
    ds, cols = dc.deep_tumor()
    t, n_valid = run_context(ds, cols, True)
    rows, first, ev, off, cl = check_context(t, cols)
    dc.deep_rows_expected(rows)
    t.close()


# ---- 2. table forms, call order, errors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device", "device_side", "exclude_host", "decode_ctx"])
def test_unique_support_table_forms(form):
    import torch
    hold = None
    if form == "device_side":
        from breakid_amd import synth_gpu
        contigs, dcols = synth_gpu.make_wgs(1_500_000, 4242, torch.device("cuda", 0))
        assert "side" in dcols
        t = capi.Context(contigs)
        t.attach_device(abi.device_ptrs(dcols), dcols["n"], dcols["n_cigar_words"], dcols["n_aux_bytes"])
        hold = dcols
        cols = {k: dcols[k].cpu().numpy().view(dt) for k, dt in (("qhash", np.uint64), ("mapq", np.uint8), ("mtid", np.int32), ("mpos", np.int32))}
        if "qcheck" in dcols:
            cols["qcheck"] = dcols["qcheck"].cpu().numpy().view(np.uint32)
    elif form == "decode_ctx":
        ds, cols = dc.dedup_tumor()
        with tempfile.TemporaryDirectory() as tmp:
            p = os.path.join(tmp, "a.bam")
            ds.write_bam(p, aligned=True)
            t, hold = capi.decode_bam_device_ctx(p, qual=QUAL)
    else:
        ds, cols = dc.dedup_tumor()
        t, hold = cc.make_ctx(ds.contigs, cols, "device" if form.endswith("device") else "host")
        if form.startswith("exclude"):
            assert t.exclude_regions(*cc.EXCLUDE) > 0
            cols = cc.filtered(cols, ~cc.excluded_mask(cols, *cc.EXCLUDE))  # `rec` numbers the kept records
    w, n_valid = t.run(qual=QUAL, fast=True)
    assert n_valid > 0
    rows, first, ev, off, cl = check_context(t, cols)
    assert rows["uniq_splits"].any()
    t.close()
    if form == "decode_ctx":
        hold.close()
    del hold


def test_unique_support_call_order_and_errors():
    ds, cols = dc.dedup_tumor()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.unique_support()
    mean, sd = t.isize_stats()
    w = capi.w_from(mean, sd)
    t.discordant_pairs(QUAL, w)
    t.mask_and_cluster(w, True)
    t.split_evidence()
    t.cluster_summary(w)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints") as e:
        t.unique_support(listing=False)
    assert e.value.code == abi.BK_ERR_ARG
    t.split_breakpoints(w)
    rows, first = t.unique_support()  # it needs no earlier bk_evidence call
    exp, exp_first = dc.expected_unique_support(*[t.fetch(st)[0] for st in (abi.STAGE_CLUSTERS, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS)], cols)
    assert rows.tobytes() == exp.tobytes() and first.tobytes() == exp_first.tobytes()
    C = capi.C
    data, n, fp, nr = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)(), C.c_uint64()
    f = t.L.bk_unique_support
    assert f(t.h, None, C.byref(n), C.byref(fp), C.byref(nr)) == abi.BK_ERR_ARG and b"null output" in t.L.bk_last_error(t.h)
    assert f(t.h, C.byref(data), None, C.byref(fp), C.byref(nr)) == abi.BK_ERR_ARG
    assert f(t.h, C.byref(data), C.byref(n), C.byref(fp), None) == abi.BK_ERR_ARG and b"go together" in t.L.bk_last_error(t.h)
    assert f(t.h, C.byref(data), C.byref(n), None, C.byref(nr)) == abi.BK_ERR_ARG
    assert f(None, C.byref(data), C.byref(n), C.byref(fp), C.byref(nr)) == abi.BK_ERR_ARG
    assert f(t.h, C.byref(data), C.byref(n), None, None) == abi.BK_OK and n.value == len(rows)
    # the other mode on the same context: the rows follow the new clusters once the stages have run again
    t.mask_and_cluster(w, False)
    with pytest.raises(capi.BreakIDError, match="bk_split_breakpoints"):
        t.unique_support()
    t.cluster_summary(w)
    t.split_breakpoints(w)
    check_context(t, cols)
    s = capi.Context(ds.contigs)
    s.upload(cols)
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.unique_support()
    assert e.value.code == abi.BK_ERR_ARG
    t.close()
    s.close()


def test_unique_support_of_a_context_without_clusters():
    tum = cc.quiet_tumor()
    t = capi.Context(tum.contigs)
    t.upload(tum.to_soa())
    t.run(qual=QUAL, fast=True)
    assert len(t.fetch(abi.STAGE_CLUSTERS)[0]) == 0
    rows, first = t.unique_support()
    assert rows.dtype == abi.UNIQUE_SUPPORT and len(rows) == 0 and len(first) == 0
    assert len(t.unique_support(listing=False)) == 0
    t.close()


def test_unique_support_is_timed():
    ds, cols = dc.dedup_tumor()
    t = capi.Context(ds.contigs)
    t.upload(cols)
    t.timing_enable(True)
    t.run(qual=QUAL, fast=True)
    rows, first = t.unique_support()
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip([name for name, _, _ in t.timing()], t.timing_touched()))
    assert "unique" in tm and tm["unique"][0] > 0 and tm["unique"][1] > 0
    assert touched["unique"] >= len(first) * 8 + len(rows) * abi.UNIQUE_SUPPORT.itemsize
    t.close()


# ---- 3. command line --------------------------------------------------------------------------------------------------------------
DEDUP_COLUMNS = ["Uniq_DRP", "Uniq_SR", "Top_DRP", "Top_SR"]
INFO_LINES = ("##INFO=<ID=UPE,Number=1,Type=Integer,", "##INFO=<ID=USR,Number=1,Type=Integer,")


def outputs(tmp, prefix):
    return sorted(f[len(prefix):] for f in os.listdir(tmp) if f.startswith(prefix + "_"))


@pytest.mark.parametrize("variant", ["plain", "all_vcf_evidence", "everything"])
@pytest.mark.parametrize("mode", ["fast", "default"])
def test_cli_dedup(mode, variant):
    ds, cols = dc.dedup_tumor()
    names = [r.qname for r in ds.recs]
    everything = variant == "everything"
    with tempfile.TemporaryDirectory() as tmp:
        tb, nb = os.path.join(tmp, "t.bam"), os.path.join(tmp, "n.bam")
        cc.write_indexed(ds, tb)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        extra = ["-fast"] if mode == "fast" else []
        if variant != "plain":
            extra += ["-all", "-vcf", "-evidence"]
        if everything:
            cc.designed_normal().write_bam(nb, aligned=True)
            extra += ["-normal", nb, "-genotype", "-clip"]
        base = [BIN, "-i", tb, "-n", side["nib"]] + extra
        a, b = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        r = subprocess.run(base + ["-o", a], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run(base + ["-o", b, "-dedup"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        # the API on the same table
        t, _ = run_context(ds, cols, mode == "fast")
        rows, first = t.unique_support()
        ev, off = t.evidence()
        cl = t.fetch(abi.STAGE_CLUSTERS)[0]
        t.close()
        # 1. the files: the twins are new, three files change, every other file is byte-identical
        twins = ["_fusion_dedup.txt"] + (["_fusion_all_dedup.txt"] if variant != "plain" else [])
        fa, fb = outputs(tmp, "a"), outputs(tmp, "b")
        assert fb == sorted(fa + twins), (fa, fb)
        changed = {"_params.txt", "_performance.txt"} | ({"_fusion.vcf", "_evidence.txt"} if variant != "plain" else set())
        for suffix in fa:
            if suffix not in changed:
                assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix
        if everything:
            assert {"_fusion_rescued.txt", "_fusion_rescued.vcf", "_evidence_rescued.txt", "_evidence.bam", "_fusion_all_genotype.txt", "_fusion_all_clip.txt"} <= set(fa) - changed
        pa, pb = open(a + "_params.txt").read(), open(b + "_params.txt").read()
        assert pb == pa.replace("out_file\t" + a, "out_file\t" + b) + "dedup\t1\n", (pa, pb)
        # 2. the twins: the rows of their fusion table in its order, and the four numbers of the call's API row
        for twin in twins:
            plain = twin.replace("_dedup", "")
            lines, src = open(b + twin).read().split("\n"), open(b + plain).read().split("\n")
            assert len(lines) == len(src) and lines[-1] == "" and lines[0] == src[0] + "\t" + "\t".join(DEDUP_COLUMNS)
            calls = written_calls(cl, b + plain)
            assert len(calls) == len(lines) - 2 and len(calls) >= (4 if plain == "_fusion.txt" else 8)
            by_key = {(cc.NAMES[cl[i]["p1_tid"]] + ":%d" % cl[i]["p1_exact"], cc.NAMES[cl[i]["p2_tid"]] + ":%d" % cl[i]["p2_exact"]): i for i in calls}
            assert len(by_key) == len(calls)
            for line, s in zip(lines[1:-1], src[1:-1]):
                f = line.split("\t")
                u = rows[by_key[(f[1], f[2])]]
                assert line == s + "\t%d\t%d\t%d\t%d" % (u["uniq_pairs"], u["uniq_splits"], u["top_pairs"], u["top_splits"]), line
        if variant == "plain":
            return
        # 3. the VCF: UPE / USR last in INFO on both breakends of a call, their header lines, nothing else touched
        va, vb = open(a + "_fusion.vcf").read().split("\n"), open(b + "_fusion.vcf").read().split("\n")
        assert [l for l in vb if not l.startswith(INFO_LINES)] != vb and len(vb) == len(va) + 2
        assert sum(l.startswith(INFO_LINES[0]) for l in vb) == 1 and sum(l.startswith(INFO_LINES[1]) for l in vb) == 1
        body_a = [l for l in va if l and not l.startswith("#")]
        body_b = [l for l in vb if l and not l.startswith("#")]
        assert [l for l in va if l.startswith("#")] == [l for l in vb if l.startswith("#") and not l.startswith(INFO_LINES)]
        assert len(body_a) == len(body_b) == 2 * len(written_calls(cl, b + "_fusion_all.txt"))
        for la, lb in zip(body_a, body_b):
            x, y = la.split("\t"), lb.split("\t")
            u = rows[int(y[2][2:].split("_")[0])]
            assert y[:7] == x[:7] and y[8:] == x[8:] and y[7] == x[7] + ";UPE=%d;USR=%d" % (u["uniq_pairs"], u["uniq_splits"]), lb
        # 4. the evidence table: a last column Dup, 0 on a fragment's first line
        ea, eb = open(a + "_evidence.txt").read().split("\n"), open(b + "_evidence.txt").read().split("\n")
        assert len(ea) == len(eb) and eb[0] == ea[0] + "\tDup" and eb[-1] == ""
        k = 0
        for c in sorted(written_calls(cl, b + "_fusion_all.txt")):
            for r_ in range(int(off[c]), int(off[c + 1])):
                k += 1
                assert eb[k] == ea[k] + "\t%d" % (0 if int(first[r_]) == r_ else 1) and eb[k].startswith("bk%d\t" % c), (k, eb[k])
                assert eb[k].split("\t")[2] == names[int(ev["rec"][r_])]
        assert k == len(eb) - 2 and any(l.endswith("\t1") for l in eb[1:-1])


def test_cli_dedup_of_a_sample_without_calls_and_errors():
    tum = cc.quiet_tumor()
    with tempfile.TemporaryDirectory() as tmp:
        tb = os.path.join(tmp, "t.bam")
        cc.write_indexed(tum, tb)
        side = synth.write_side_files(tum, tmp)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        prefix = os.path.join(tmp, "z")
        base = [BIN, "-i", tb, "-o", prefix, "-n", side["nib"], "-all", "-fast"]
        r = subprocess.run(base + ["-dedup", "-gpus", "2"], env=env, capture_output=True, text=True)
        assert r.returncode == 1 and "-dedup cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
        assert not any(f.startswith("z_") for f in os.listdir(tmp))
        r = subprocess.run(base + ["-dedup", "-evidence", "-vcf"], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        header = open(prefix + "_fusion.txt").read()
        assert header.count("\n") == 1
        for twin in ("_fusion_dedup.txt", "_fusion_all_dedup.txt"):
            assert open(prefix + twin).read() == header[:-1] + "\t" + "\t".join(DEDUP_COLUMNS) + "\n"
        assert open(prefix + "_evidence.txt").read().split("\n")[0].endswith("\tRecord\tDup")
        assert all(any(l.startswith(i) for l in open(prefix + "_fusion.vcf").read().split("\n")) for i in INFO_LINES)
        assert open(prefix + "_params.txt").read().endswith("dedup\t1\n")

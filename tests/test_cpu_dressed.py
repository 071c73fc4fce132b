"""CPU: the host BAM decoder, bk_bam_extract and the CPU build of the command line on records shaped like aligner output
(breakid_amd/dress.py: bases, qualities, typed aux fields around SA / OC, hand-written aux LAYOUTS), and what the REAL
reference made of such files (tests/golden/edge_dressed.*, g1_dressed.*)."""
import json
import os
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from oracle import pyoracle
from tests import dresscases, refdump
from tests.test_cpu_cli import binaries  # noqa: F401  (fixture: make -C oracle san)

SUFFIXES = [".ahc.stages.txt", ".fast.stages.txt", ".regions.json", ".soa.npz"] + [
    ".%s%s" % (m, s) for m in ("ahc", "fast") for s in ("_fusion.txt", "_fusion_all.txt", "_perf5.txt", "_params.txt")]


def test_the_reference_ignores_bases_qualities_and_foreign_fields(golden_dir):
    """the premise of the dresser, established by the reference itself: every golden of the dressed g1 file is the golden of
    the bare one, byte for byte (the params file names its input)"""
    for s in SUFFIXES:
        a = open(os.path.join(golden_dir, "g1_dressed" + s), "rb").read()
        b = open(os.path.join(golden_dir, "g1" + s), "rb").read()
        if s.endswith("_params.txt"):
            a = a.replace(b"g1_dressed.bam", b"g1.bam")
        assert a == b, s


def test_the_reference_read_the_layouts_as_stated(golden_dir):
    """split tuples the reference printed for the region of the layout reads: one per layout whose blob is not empty, with
    the partner of the FIRST field named SA and the cigar of the first OC; none for the others"""
    reg = json.load(open(os.path.join(golden_dir, "edge_dressed.regions.json")))[0]
    assert (reg["chr"], reg["start"], reg["end"]) == dresscases.LAYOUT_REGION
    seen = {}
    for ln in reg["sa"].strip().split("\n")[1:]:
        f = ln.split()
        if f[2] == "0":
            seen.setdefault(f[0], []).append(f)
    for lay in dresscases.LAYOUTS:
        rows = seen.get(lay.qname, [])
        assert len(rows) == (1 if lay.sa else 0), (lay.name, rows)
        if lay.sa:
            chrom, pos, _, cigar = lay.sa.split(";")[0].split(",")[:4]
            f = rows[0]
            assert (f[6], f[8], f[9], f[11]) == (lay.oc or "60M40S", chrom, pos, cigar), (lay.name, f)
    # the pair whose read name fills l_read_name = 255 is a discordant pair for the reference
    dump = refdump.parse_stages(os.path.join(golden_dir, "edge_dressed.fast.stages.txt"))
    assert sum(r["qname"] == dresscases.LONG_NAME for g in dump["groups"].values() for r in g.get("scan", [])) == 1


@pytest.fixture(scope="module")
def files():
    """the dressed files, written once: name -> (Dataset, expected table, {aligned: path})"""
    with tempfile.TemporaryDirectory() as t:
        out = {}
        lay = synth.Dataset([("chr%d" % i, 400_000) for i in range(1, 5)], dresscases.layout_recs())
        lay.sort()
        for name, ds in (("edge", dresscases.edge_dressed()), ("g1", synth.make_g1()), ("layouts", lay)):
            paths = {}
            for aligned in (True, False):
                paths[aligned] = os.path.join(t, "%s.%d.bam" % (name, aligned))
                dresscases.write_dressed(ds, paths[aligned], aligned=aligned)
            out[name] = (ds, ds.to_soa(), paths)
        yield out


@pytest.mark.parametrize("threads", ["1", "5"])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "across_blocks"])
@pytest.mark.parametrize("name", ["edge", "g1", "layouts"])
def test_host_decoder_on_dressed_records(files, monkeypatch, name, aligned, threads):
    ds, ref, paths = files[name]
    monkeypatch.setenv("BREAKID_THREADS", threads)
    contigs, cols = capi.decode_bam(paths[aligned])
    assert contigs == ds.contigs
    dresscases.assert_table(ds, cols, ref)


def test_host_decoder_dressed_records_across_decode_chunks(monkeypatch):
    """more than 2 x 65536 dressed records: the decoder's record chunks begin and end inside dressed records' neighbourhoods"""
    contigs = [("chr1", 3_000_000), ("chr2", 2_000_000)]
    ds = synth.make_cfg(5, contigs, 150_000, 40, 30, 200, jitter=200, read_len=100)
    for i in range(0, len(ds.recs), 977):
        ds.recs[i].sa = "chr2,%d,+,40S60M,60,0;" % (100 + i)
        if i % 2:
            ds.recs[i].oc = "60M40S"
    ref = ds.to_soa()
    assert len(ref["tid"]) > 2 * 65536
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "a.bam")
        dresscases.write_dressed(ds, p)
        for th in ("1", "5"):
            monkeypatch.setenv("BREAKID_THREADS", th)
            dresscases.assert_table(ds, capi.decode_bam(p)[1], ref)


@pytest.mark.parametrize("ends_with_record", [False, True])
def test_host_decoder_walks_past_records_spelled_inside_a_payload(ends_with_record):
    """the files of test_gpu_dressed's decoy test are legal BAM: the host decoder, which follows the length chain from the
    first record, gives the exact table"""
    ds = synth.make_g1()
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "d.bam")
        dresscases.write_decoy_chain_file(ds, p, ends_with_record)
        dresscases.assert_table(ds, capi.decode_bam(p)[1])


def test_extract_appends_its_tag_behind_the_aux_of_dressed_records(files):
    ds, _, paths = files["edge"]
    names = sorted({r.qname for r in ds.recs})
    chosen = [lay.qname for lay in dresscases.LAYOUTS] + [dresscases.LONG_NAME] + names[::97]
    chosen = list(dict.fromkeys(chosen))
    tags = ["1", "2,5", "17"]
    keys = np.zeros(len(chosen), abi.READ_KEY)
    for i, q in enumerate(chosen):
        keys[i] = (synth.fnv1a64(q.encode()), synth.qname_check(q.encode()), i % 3)
    for aligned in (True, False):
        with tempfile.TemporaryDirectory() as t:
            out = os.path.join(t, "ev.bam")
            got_names, n = capi.bam_extract(paths[aligned], out, keys, tags)
            assert got_names == chosen
            m = dresscases.check_extract(paths[aligned], out, {q.encode(): tags[i % 3] for i, q in enumerate(chosen)})
            assert m == n and m >= 3 * len(dresscases.LAYOUTS) + 2


def test_the_generator_puts_every_type_in_front_of_a_split_read(golden_dir):
    """non-vacuity, asserted on the generator: each scalar / string type and each B sub-type stands in front of the SA:Z of
    at least three records that own a tuple of the oracle's STAGE_SPLITS on the dressed edge table"""
    ds = dresscases.edge_dressed()
    cols = ds.to_soa()
    o = pyoracle.Oracle(ds.contigs, cols)
    _, rc = o.run(20, fast=True)
    assert rc == 0
    sp, _ = o.fetch(abi.STAGE_SPLITS)
    o.close()
    owners = set(int(v) for v in sp["rec"])
    count = {k: 0 for k in dresscases.KINDS}
    for i, (r, _, _, aux) in enumerate(dresscases.dress_plan(ds)):
        if i in owners:
            for k in set(dresscases.kinds_in_front_of_sa(aux)):
                count[k] += 1
    assert len(count) == 18 and min(count.values()) >= 3, count
    # and the rest of what the dresser promises is in the file: every l_seq, qualities of 0xFF, long arrays, decoys, a second SA
    plan = dresscases.dress_plan(ds)
    assert {len(q) for _, _, q, _ in plan} == set(dresscases.L_SEQS)
    assert sum(1 for _, _, q, _ in plan if len(q) > 1 and q == b"\xff" * len(q)) >= 10
    items = [it for _, _, _, aux in plan for it in aux if not isinstance(it, bytes)]
    assert sum(1 for it in items if len(it) == 3 and it[1] == "B" and len(it[2][1]) >= 3000) >= 5
    assert sum(1 for it in items if len(it) == 3 and it[1] in "ZH" and dresscases.DECOY_SA in bamio.encode_aux_item(it)) >= 5
    assert sum(1 for it in items if len(it) == 3 and it[1] == "B" and it[2][0] == "C" and dresscases.DECOY_BYTES in it[2][1]) >= 1
    assert sum(1 for _, _, _, aux in plan if sum(1 for it in aux if not isinstance(it, bytes) and it[0] == "SA") == 2) >= 5
    assert sum(1 for r, _, _, aux in plan if not r.sa and any(not isinstance(it, bytes) and it[0] == "OC" for it in aux)) >= 5


@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_host_code_reproduces_reference_txt_on_the_dressed_file(binaries, golden_dir, mode):  # noqa: F811
    dresscases.check_cli_reproduces_reference_txt(binaries["plain"], golden_dir, mode, aligned=(mode == "fast"))


@pytest.mark.parametrize("san", ["asan", "ubsan"])
@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_host_code_clean_under_sanitizers_on_the_dressed_file(binaries, golden_dir, san, mode):  # noqa: F811
    dresscases.check_cli_reproduces_reference_txt(binaries[san], golden_dir, mode, aligned=(mode == "ahc"))

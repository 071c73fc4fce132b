"""Junction fit without a GPU: the row layouts and the exports, the Python definition (tests/homologycases.py) on the designed truth
of the consensus BAM, on the insertion and microhomology loci and on its own reference packer, and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import callcases as cc
from tests import homologycases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
RADIUS = 64 + hc.MAX_SHIFT + 33


def test_row_layouts_and_exports():
    assert abi.JUNCTION_PROBE.itemsize == 32 and abi.JUNCTION_FIT.itemsize == 32
    assert list(abi.JUNCTION_PROBE.names) == ["tid_own", "pos_own", "dir_own", "tid_mate", "pos_mate", "dir_mate", "qlen", "reserved"]
    assert list(abi.JUNCTION_FIT.names) == ["shift", "ins", "aligned", "mism", "hom_fwd", "hom_back", "score", "placed"]
    assert [abi.JUNCTION_FIT.fields[f][1] for f in abi.JUNCTION_FIT.names] == list(range(0, 32, 4))
    assert [abi.JUNCTION_PROBE.fields[f][1] for f in abi.JUNCTION_PROBE.names] == list(range(0, 32, 4))
    assert abi.JUNCTION_FIT.fields["shift"][0] == np.dtype("<i4") and abi.JUNCTION_FIT.fields["score"][0] == np.dtype("<i4")
    assert abi.JUNCTION_PROBE.fields["tid_own"][0] == np.dtype("<i4") and abi.JUNCTION_PROBE.fields["tid_mate"][0] == np.dtype("<i4")
    assert [n for n, _ in abi.REFSEQ_COLS] == ["tid", "start", "len", "off", "bases"] and capi.C.sizeof(abi.RefSeq) == 8 * 6
    assert "bk_junction_fit" in capi.EXPORTS and hasattr(capi.lib(), "bk_junction_fit") and hasattr(capi.Context, "junction_fit")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_junction_fit { int32_t shift; uint32_t ins, aligned, mism, hom_fwd, hom_back; int32_t score; uint32_t placed; };" in header
    assert "struct bk_junction_probe { int32_t tid_own; uint32_t pos_own, dir_own; int32_t tid_mate; uint32_t pos_mate, dir_mate; uint32_t qlen, reserved; };" in header
    assert "typedef struct bk_refseq {" in header


def test_reference_packer_and_nib_writer(tmp_path):
    """a window table, a whole nib payload and the genome itself give the same bases; gaps and the contig's ends are N"""
    g = hc.Genome([1001, 40], {(0, 7): "N", (0, 8): "G"})
    path = str(tmp_path / "c.nib")
    g.write_nib(path, 0)
    n, payload = hc.read_nib(path)
    assert n == 1001 and len(payload) == 501
    whole = {"tid": np.zeros(1, np.int32), "start": np.zeros(1, np.uint32), "len": np.asarray([n], np.uint32), "off": np.asarray([0, len(payload)], np.uint64), "bases": payload}
    pos = np.arange(-3, 1010)
    assert np.array_equal(hc.ref_codes(whole, 0, pos), g.codes(0, pos))
    assert g.text(0, 6, 9)[1:3] == "NG" and list(hc.ref_codes(whole, 0, [0, 1002])) == [4, 4] and list(hc.ref_codes(whole, 1, [5])) == [4]
    parts = g.refseq([(0, 3, 10), (0, 13, 7), (0, 500, 501), (1, 0, 40)])  # abutting, a gap, an odd length at the contig's end
    got = hc.ref_codes(parts, 0, pos)
    inside = ((pos >= 4) & (pos <= 20)) | ((pos >= 501) & (pos <= 1001))
    assert np.array_equal(got, np.where(inside, g.codes(0, pos), 4))
    assert np.array_equal(hc.ref_codes(parts, 1, np.arange(0, 45)), g.codes(1, np.arange(0, 45)))
    soft = dict(parts)
    soft["bases"] = parts["bases"] | 0x88  # the soft-mask bit changes nothing
    assert np.array_equal(hc.ref_codes(soft, 0, pos), got)
    probes = hc.as_probes([(0, 100, 0, 0, 600, 1, 5), (0, 5, 1, 1, 39, 0, 5), (3, 5, 0, 0, 5, 0, 5)])
    assert hc.merged_windows(probes, 10, g.lengths) == [(0, 0, 15), (0, 89, 21), (0, 589, 21), (1, 28, 12)]


def fit_one(ref, row, text, max_len=64, **kw):
    return hc.expected_fit(ref, hc.as_probes([row]), hc.as_query([text], max_len), max_len, **kw)[0]


@pytest.fixture(scope="module")
def designed():
    g = hc.genome()
    probes, texts = hc.designed_table()
    extra = hc.as_probes([hc.locus_probe(hc.HOM_LOCUS, True, 40), hc.locus_probe(hc.HOM_LOCUS, False, 60)])
    ref = g.refseq(hc.merged_windows(np.concatenate([probes, extra]), RADIUS, hc.LENGTHS))
    return g, ref, probes, texts


def test_definition_on_the_designed_truth(designed):
    g, ref, probes, texts = designed
    rows = hc.expected_fit(ref, probes, hc.as_query(texts, 64), 64)
    assert len(rows) == 18 and (rows["placed"] == 1).all()
    assert (rows["shift"] == 0).all() and (rows["ins"] == 0).all() and (rows["aligned"] == probes["qlen"]).all()
    ll_a = [k for k, p in enumerate(probes) if (int(p["tid_own"]), int(p["pos_own"])) == cc.LOCI[1][1:3]]
    assert len(ll_a) == 1 and int(rows[ll_a[0]]["mism"]) == 1  # the designed 4 : 4 tie in column 7 or 9 of LL_x, side A
    assert int(rows["mism"].sum()) == 1 and (rows["score"] == rows["aligned"].astype(np.int64) - 2 * rows["mism"]).all()
    hom = rows["hom_fwd"].astype(np.int64) + rows["hom_back"]
    assert int((hom > 0).sum()) == 10 and hom.max() == 1  # chance homology: one base, back on one side and forward on the other
    for k in range(0, 18, 2):
        if rows[k]["mism"] == 0 and rows[k + 1]["mism"] == 0:
            assert hom[k] == hom[k + 1] and int(rows[k]["hom_back"]) == int(rows[k + 1]["hom_fwd"]) and int(rows[k]["hom_fwd"]) == int(rows[k + 1]["hom_back"])
    # the same from a table of whole contigs: the windows hold all a walk reads
    whole = g.refseq([(t, 0, n) for t, n in enumerate(hc.LENGTHS)])
    assert hc.expected_fit(whole, probes, hc.as_query(texts, 64), 64).tobytes() == rows.tobytes()


def test_insertions_and_single_mismatches(designed):
    g, ref, probes, texts = designed
    row, text = hc.insertion_query(g)
    assert text.startswith(hc.INSERTED) and len(text) == 40
    r = fit_one(ref, row, text)
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"]), int(r["aligned"]), int(r["score"])) == (7, 3, 0, 33, 33) and r["hom_fwd"] == 0 and r["hom_back"] == 0
    # GATTACA: its last base continues the partner by chance, so a shorter insertion with one mismatch ties the score and wins
    row, text = hc.insertion_query(g, last="A")
    r = fit_one(ref, row, text)
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"]), int(r["score"])) == (4, 0, 1, 34)
    # with max_ins 0 the inserted bases can only be mismatches; with max_shift 0 the continuation is not found behind them
    r = fit_one(ref, row, text, max_ins=0)
    assert int(r["ins"]) == 0 and int(r["aligned"]) == 40
    # a complemented base in column 0 is a non-templated base, in column 1 or 5 a mismatch
    row, text = tuple(probes[0])[:7], texts[0]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for col, want in ((0, (1, 1, 0)), (1, (0, 0, 1)), (5, (0, 0, 1))):
        t = text[:col] + comp[text[col]] + text[col + 1:]
        r = fit_one(ref, row, t)
        assert (int(r["ins"]), int(r["shift"]), int(r["mism"])) == want, (col, r)
    r = fit_one(ref, row, text[:5] + "N" + text[6:])
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"])) == (0, 0, 1)  # N matches nothing


def test_microhomology_locus(designed):
    g, ref, _, _ = designed
    _, ta, bpa, _, tb, bpb, _ = hc.HOM_LOCUS
    a, b = hc.locus_probe(hc.HOM_LOCUS, True, 40), hc.locus_probe(hc.HOM_LOCUS, False, 60)
    qa, qb = hc.mate_text(g, a[2], a[3], a[4], a[5], 0, 40), hc.mate_text(g, b[2], b[3], b[4], b[5], 0, 60)
    assert g.text(ta, bpa + 1, bpa + hc.HOM_PATCHED) == qa[:hc.HOM_PATCHED]  # the patch: the own contig goes on as the partner does
    ra, rb = fit_one(ref, a, qa), fit_one(ref, b, qb)
    assert int(ra["hom_fwd"]) >= hc.HOM_PATCHED and int(ra["hom_fwd"]) + int(ra["hom_back"]) == 6 and ra["mism"] == 0 and ra["shift"] == 0
    assert int(rb["hom_back"]) == int(ra["hom_fwd"]) and int(rb["hom_fwd"]) == int(ra["hom_back"])
    # both sides name the same bases: side A's stretch on its own contig, side B's on its own
    sa = hc.hom_seq(g, ta, bpa, hc.LEFT, int(ra["hom_fwd"]), int(ra["hom_back"]))
    sb = hc.hom_seq(g, tb, bpb, hc.RIGHT, int(rb["hom_fwd"]), int(rb["hom_back"]))
    assert sa == sb and len(sa) == 6
    # max_hom caps the backward count, qlen the forward one
    assert int(fit_one(ref, a, qa, max_hom=0)["hom_back"]) == 0 and int(fit_one(ref, a[:6] + (3,), qa[:3])["hom_fwd"]) == 3
    # an unplaced probe is all zeros
    assert not fit_one(ref, a[:3] + (-1,) + a[4:], qa).tobytes().strip(b"\0") and not fit_one(ref, a[:6] + (0,), "").tobytes().strip(b"\0")


def test_tie_rules_on_repeats():
    poly, _ = hc.repeat_ref("A")
    r = fit_one(poly, (0, 300, hc.LEFT, 0, 400, hc.RIGHT, 30), "A" * 30)
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"])) == (0, 0, 0) and int(r["hom_fwd"]) == 30 and int(r["hom_back"]) == 32
    di, text = hc.repeat_ref("AC")
    q = text[402:432]  # M[3 ..] of a probe at 400 (1-based): the period makes shifts 3, 1, -1, -3, .. equal; |1| ties, +1 wins
    r = fit_one(di, (0, 300, hc.LEFT, 0, 400, hc.RIGHT, 30), q)
    assert (int(r["ins"]), int(r["shift"]), int(r["mism"])) == (0, 1, 0)
    r = fit_one(di, (0, 300, hc.LEFT, 0, 400, hc.RIGHT, 30), "G" + q[1:])  # column 0 off: ins 1 on the nearest diagonal that fits
    assert (int(r["ins"]), int(r["mism"]), abs(int(r["shift"]))) == (1, 0, 0)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_homology(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-consensus", "-homology"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -homology needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-consensus", "-homology", "-homshift", "10", "-homins", "0", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -homology needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-homology"], capture_output=True, text=True)
    assert r.returncode == 1 and "-homology needs -consensus" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-consensus", "-homshift", "10"], capture_output=True, text=True)
    assert r.returncode == 1 and "-homshift and -homins need -homology" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-consensus", "-homology", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-homology cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-homology" in r.stderr and "-homshift" in r.stderr and "-homins" in r.stderr


def test_definition_on_the_edge_table():
    ref, probes, query = hc.edge_table()
    rows = hc.expected_fit(ref, probes, query, 100)
    assert list(rows["placed"][-5:]) == [0, 0, 0, 1, 1] and not rows[-5:-2].tobytes().strip(b"\0")
    on_two = probes["tid_own"] == 2  # a contig without a segment: no own walk, so no homology
    assert on_two.sum() > 10 and not rows["hom_fwd"][on_two].any() and not rows["hom_back"][on_two].any()
    none = hc.expected_fit(hc.make_refseq([]), probes, query, 100)
    live = none["placed"] == 1  # no reference at all: every column a mismatch, so the longest insertion on the nearest diagonal
    assert (none["shift"][live] == 0).all() and (none["ins"][live] == np.minimum(32, probes["qlen"][live] - 1)).all() and (none["mism"] == none["aligned"]).all()
    assert set(np.unique(ref["bases"] >> 4)) >= set(range(16))  # soft-masked nibbles and every N code are in the table

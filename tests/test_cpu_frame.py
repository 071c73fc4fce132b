"""Fusion frame without a GPU: the row layouts, the exports and the header's text; the two statements of the definition in
tests/framecases.py (coordinates of the parts against one entry per base) on seeded small cases that reach every class; the hand
example of the header in both variants; the model the Python helper builds from refGene rows; and the command line's refusals."""
import os
import subprocess
from functools import partial

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import framecases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layouts_and_exports():
    assert abi.FRAME_SITE.itemsize == 24 and abi.FRAME_CALL.itemsize == 48
    assert list(abi.FRAME_SITE.names) == ["tid1", "pos1", "tid2", "pos2", "right1", "right2", "reserved"]
    assert [abi.FRAME_SITE.fields[f][1] for f in abi.FRAME_SITE.names] == [0, 4, 8, 12, 16, 17, 18]
    assert list(abi.FRAME_CALL.names) == ["cls", "order", "loc", "role", "exon", "reserved", "tx", "cod", "n_tx", "n_inframe", "n_compatible", "reserved2"]
    assert [abi.FRAME_CALL.fields[f][1] for f in abi.FRAME_CALL.names] == [0, 1, 2, 4, 6, 10, 12, 20, 28, 36, 40, 44]
    assert abi.FRAME_CALL.fields["tx"][0] == np.dtype(("<i4", (2,))) and abi.FRAME_CALL.fields["exon"][0] == np.dtype(("<u2", (2,)))
    assert abi.FRAME_CLASSES == ["none", "antisense", "truncating", "promoter", "outframe", "inframe"]
    C = capi.C
    assert C.sizeof(abi.TxModel) == 16 + 7 * 8 and [f[0] for f in abi.TxModel._fields_] == ["n_tx", "n_parts", "tid", "tx_start", "tx_end", "strand", "ex_off", "ex_start", "ex_end"]
    assert "bk_fusion_frame" in capi.EXPORTS and hasattr(capi.lib(), "bk_fusion_frame")
    assert hasattr(capi.Context, "fusion_frame") and hasattr(capi, "TxModel")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_frame_site { int32_t tid1; uint32_t pos1; int32_t tid2; uint32_t pos2; uint8_t right1, right2; uint8_t reserved[6]; };" in header
    assert ("struct bk_frame_call { uint8_t cls, order, loc[2], role[2]; uint16_t exon[2]; uint16_t reserved; int32_t tx[2]; uint32_t cod[2], n_tx[2], n_inframe, n_compatible; "
            "uint32_t reserved2; };") in header
    assert "int bk_fusion_frame(bk_ctx *ctx, const bk_txmodel *model, const struct bk_frame_site *sites, uint64_t n, const struct bk_frame_call **out);" in header
    for k, name in enumerate(abi.FRAME_CLASSES):
        assert "#define BK_FRAME_%s %d\n" % (name.upper(), k) in header
    for k, name in enumerate(["NONCODING", "5UTR", "CDS", "INTRON", "3UTR"]):
        assert "#define BK_LOC_%s %d" % (name, k + 1) in header
    assert "constexpr uint32_t FRAME_CHUNK = %d;" % abi.FRAME_CHUNK in open(os.path.join(ROOT, "breakid_amd", "csrc", "frame.h")).read()
    assert "T.tx_start < P && P <= T.tx_end" in header and "scope `fusion_frame`" in header and "2^24 transcripts or 2^28 parts" in header


def test_the_two_statements_agree_and_reach_every_class():
    """1000 seeded cases (a model of up to seven transcripts with up to four coding parts on a 160-base contig, one site each): both
    statements give the same bytes, every class is the reported one at least 20 times, and so is a pair of one transcript with itself"""
    rng = np.random.default_rng(28)
    per_base = partial(fc.per_base, length=160)
    seen, same, pairs = [0] * 6, 0, 0
    for case in range(1000):
        cols, sites = fc.random_case(rng)
        a = fc.expected(cols, sites)
        b = fc.expected(cols, sites, info=per_base)
        assert a.tobytes() == b.tobytes(), (case, a, b)
        seen[int(a[0]["cls"])] += 1
        same += int(a[0]["tx"][0]) >= 0 and int(a[0]["tx"][0]) == int(a[0]["tx"][1])
        pairs += int(a[0]["n_tx"][0]) * int(a[0]["n_tx"][1])
        assert int(a[0]["n_inframe"]) <= int(a[0]["n_compatible"]) <= int(a[0]["n_tx"][0]) * int(a[0]["n_tx"][1])
    assert min(seen) >= 20 and same >= 20 and pairs >= 1000, (seen, same, pairs)  # (a pair per case on average)


def g1_model(geneb_strand="-"):
    lines = list(synth.G1_REFGENE)
    lines[1] = lines[1].replace("\tchr2\t-\t", "\tchr2\t%s\t" % geneb_strand)
    names = ["chr%d" % i for i in range(1, 23)] + ["chrX", "chrY"]
    model, dropped = capi.TxModel.from_refgene(lines + ["0\tNR_000009\tchr1\t+\t1\t9\t9\t9\t1\t1,\t9,\t0\tNC\tunk\tunk\t-1,", lines[0].replace("chr1", "chrUn")], names)
    assert dropped == 1 and len(model) == 2 and model.genes == ["GENEA", "GENEB"] and model.names == ["NM_000001", "NM_000002"]
    return model


def test_hand_example():
    """the G1 call: side 1 chr1:50099 LEFT, side 2 chr2:80200 RIGHT"""
    site = fc.as_sites([(0, 50099, 0, 1, 80200, 1)])
    m = g1_model()
    assert fc.parts_of(m.cols, 0) == [(40500, 41000), (50000, 51000), (58000, 59500)] and fc.parts_of(m.cols, 1) == [(70500, 71000), (80100, 89500)]
    assert fc.side_info(m.cols, 0, 50099, 0) == (3000, 599, fc.HEAD, 2, fc.CDS)
    assert fc.side_info(m.cols, 1, 80200, 1) == (9900, 9301, fc.HEAD, 1, fc.CDS)
    c = fc.expected(m.cols, site)[0]
    assert (int(c["cls"]), int(c["order"]), list(c["tx"]), list(c["cod"]), list(c["role"]), list(c["n_tx"])) == (fc.ANTISENSE, 0, [0, 1], [599, 9301], [1, 1], [1, 1])
    assert int(c["n_inframe"]) == 0 and int(c["n_compatible"]) == 0
    assert fc.call_fields(c, m.names, m.genes) == ["antisense", ".", "GENEA", "NM_000001", "CDS", "2", "599", ".", "GENEB", "NM_000002", "CDS", "1", "9301", ".", "1", "0", "0"]
    assert fc.info_fields(c, m.genes) == ";FRCLASS=antisense"
    p = g1_model("+")
    assert fc.side_info(p.cols, 1, 80200, 1) == (9900, 599, fc.TAIL, 2, fc.CDS)
    c = fc.expected(p.cols, site)[0]
    assert (int(c["cls"]), int(c["order"]), list(c["cod"]), list(c["exon"]), list(c["loc"])) == (fc.INFRAME, 1, [599, 599], [2, 2], [fc.CDS, fc.CDS])
    assert int(c["n_inframe"]) == 1 and int(c["n_compatible"]) == 1
    assert fc.call_fields(c, p.names, p.genes) == ["inframe", "5-3", "GENEA", "NM_000001", "CDS", "2", "599", "2", "GENEB", "NM_000002", "CDS", "2", "599", "2", "1", "1", "1"]
    assert fc.info_fields(c, p.genes) == ";FRCLASS=inframe;FR5P=GENEA;FR3P=GENEB"
    # the sides the other way round: the same pair, side 2 is the 5' partner
    c = fc.expected(p.cols, fc.as_sites([(1, 80200, 1, 0, 50099, 0)]))[0]
    assert (int(c["cls"]), int(c["order"]), list(c["tx"])) == (fc.INFRAME, 2, [1, 0])
    assert fc.info_fields(c, p.genes) == ";FRCLASS=inframe;FR5P=GENEA;FR3P=GENEB"
    # a side without a transcript: none, and the other side still reports its transcript
    c = fc.expected(p.cols, fc.as_sites([(0, 50099, 0, 5, 80200, 1)]))[0]
    assert (int(c["cls"]), int(c["order"]), list(c["tx"]), list(c["n_tx"])) == (fc.NONE, 0, [0, -1], [1, 0])
    assert fc.call_fields(c, p.names, p.genes) == ["none", ".", "GENEA", "NM_000001", "CDS", "2", "599", "."] + ["."] * 6 + ["0", "0", "0"]
    assert fc.info_fields(c, p.genes) == ""


def test_overlap_rule_and_an_intragenic_deletion():
    # the half-open rule: a transcript [100, 200) overlaps P = 101 .. 200, not 100 (its first base is b = 100, P = 101) and not 201
    cols = fc.make_cols([(0, 100, 200, 0, [(110, 150), (160, 190)])])
    assert [len(fc.overlapping(cols, 0, P)) for P in (100, 101, 200, 201)] == [0, 1, 1, 0]
    # a deletion inside one '+' transcript, LEFT at P1 and RIGHT at P2: in frame exactly when the coding bases between are a multiple of 3
    for P1, P2 in ((120, 124), (120, 125), (120, 126), (140, 165), (140, 166), (140, 167), (105, 120), (120, 195)):
        removed = sum(1 for b in range(P1, P2 - 1) if 110 <= b < 150 or 160 <= b < 190)
        c = fc.expected(cols, fc.as_sites([(0, P1, 0, 0, P2, 1)]))[0]
        bounds = 110 < P1 and P2 - 1 < 190
        assert int(c["cls"]) == ((fc.INFRAME if removed % 3 == 0 else fc.OUTFRAME) if bounds else fc.TRUNCATING), (P1, P2, removed, c)
        assert list(c["tx"]) == [0, 0] and int(c["order"]) == 1


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_frame(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-frame"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -frame needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-frame", "-all", "-fast", "-coverage"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -coverage needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    # -f alone completed to -fast while that was the only option with an f, and still means it
    r = subprocess.run(base + ["-f", "-frame"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -frame needs the GPU library" in r.stderr and "ambiguous" not in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    # the usage refusals stand behind the help text, in the order of the table: -frame's own behind every older row
    for args, word in ((["-frame", "-gpus", "2"], "Error: -frame cannot be combined with -gpus."), (["-frame", "-covflank", "100"], "Error: -covflank needs -coverage."),
                       (["-frame", "-gpus", "2", "-simflank", "9"], "Error: -simflank needs -similar."), (["-frame", "-gpus", "2", "-coverage"], "Error: -coverage cannot be combined with -gpus.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-frame" in r.stderr and "FRCLASS" in r.stderr and "Error" not in r.stderr

"""`-lociseq` and `-panel` of the command line: the bytes of <prefix>_cliploci_seq.txt against cliplocicases + consensuscases + the
brute force of tests/seqmatchcases.py on a designed BAM with bases; every other file unchanged; stdout, the params lines, a run
without a written locus, refusals and FASTA errors."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import callcases as cc
from tests import cliplocicases as lc
from tests import consensuscases as kc
from tests import seqmatchcases as sm

pytestmark = pytest.mark.gpu
BIN = cc.BIN
QUAL = cc.QUAL
CONTIGS = cc.CONTIGS
NAMES = cc.NAMES
TLEN = [l for _, l in CONTIGS]
LOCI = [("a", 0, 300_000, "L", 1, 700_000, "R"), ("b", 1, 700_090, "R", 3, 900_000, "R")]
SEQ_COLUMNS = ["Seq_N", "Seq_Len", "Seq_Agree", "Seq", "Seq_Tail"]
PANEL_COLUMNS = ["Pn_Name", "Pn_Strand", "Pn_Score", "Pn_Len", "Pn_Mism", "Pn_Run", "Pn_QStart", "Pn_Start", "Pn_End", "Pn_Seeds", "Pn_Second", "Pn_Score2", "Pn_PairSpan"]


def elements():
    """the three panel sequences: B ends in 20 A; C; D holds 30 bases of B's head with one substitution in their middle (runs of 15
    and 14: a runner-up at seed 12, nothing at seed 16)"""
    rng = np.random.default_rng(21)
    B = sm.draw(rng, 190) + "A" * 20
    C = sm.draw(rng, 150)
    piece = B[5:35]
    D = sm.draw(rng, 40) + piece[:15] + ("A" if piece[15] != "A" else "C") + piece[16:] + sm.draw(rng, 40)
    return B, C, D


def fasta_text(B, C, D):
    """lower case, IUPAC letters, blank lines, a description behind the name, a line with CR LF"""
    return ("\n>ELEM_B an element with a tail\n" + B[:70].lower() + "\n\n" + B[70:140] + "\r\n" + B[140:] + "\n>ELEM_C\n" + C[:80] + "\n" + C[80:] + "RYKM\n\n>ELEM_D third\n" +
            D.lower() + "\n")


def text_codes(t):
    return np.asarray([kc.CODE[c] for c in t], np.uint8)


def clip_reads(B, C):
    """chr3 1 200 000 / 1 199 991: a mutual pair whose LEFT clips read into B's head and whose RIGHT clips come out of its poly-A end;
    chr3 1 300 000 / 1 299 991: the same with C reverse-complemented; chr3 1 500 000: a RIGHT locus of drawn bases; chr3 1 600 000: two
    reads, below -locisupport.  Returns [(record, lead, trail)], the clips in read order."""
    rng = np.random.default_rng(22)
    rc = sm.revcomp(C)
    out = [(lc.left_clip("bl%d" % k, 2, 1_200_000), None, B[:40]) for k in range(4)] + [(lc.right_clip("br%d" % k, 2, 1_199_991), B[-40:], None) for k in range(3)]
    out += [(lc.left_clip("cl%d" % k, 2, 1_300_000), None, rc[:40]) for k in range(3)] + [(lc.right_clip("cr%d" % k, 2, 1_299_991), rc[-40:], None) for k in range(4)]
    lone = sm.draw(rng, 40)
    out += [(lc.right_clip("or%d" % k, 2, 1_500_000), lone, None) for k in range(3)]
    out += [(lc.left_clip("lo%d" % k, 2, 1_600_000), None, B[:40]) for k in range(2)]
    return out


@pytest.fixture(scope="module")
def cli():
    B, C, D = elements()
    ds = cc.designed_tumor(mix=False, n_proper=3000, loci=LOCI)
    designed = clip_reads(B, C)
    codes = {id(r): kc.record_codes(r, lead=None if lead is None else text_codes(lead), trail=None if trail is None else text_codes(trail)) for r, lead, trail in designed}
    ds.recs += [r for r, _, _ in designed]
    ds.sort()
    for r in ds.recs:
        if id(r) not in codes:
            codes[id(r)] = kc.record_codes(r)
    cols = ds.to_soa()
    t = capi.Context(CONTIGS)
    t.upload(cols)
    t.run(qual=QUAL, fast=True)
    clusters = t.fetch(abi.STAGE_CLUSTERS)[0].copy()
    t.close()
    clipped = [r for r in ds.recs if "S" in r.cigar and not r.sa]
    reads = kc.make_reads([(r.tid, r.pos, r.flag, r.mapq, r.cigar, codes[id(r)]) for r in clipped])
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "t.bam")

        def gen():
            for r in ds.recs:
                aux = ([("SA", r.sa)] if r.sa else []) + ([("OC", r.oc)] if r.oc else [])
                c = codes[id(r)]
                yield bamio.encode_record(r.qname, r.flag, r.tid, r.pos, r.mapq, bamio.parse_cigar(r.cigar), r.mtid, r.mpos, r.isize, aux, seq=bytes(kc.pack_codes(c)), qual=b"\x1e" * len(c))
        bamio.write_bam(bam, ds.contigs, gen(), aligned=True)
        bamio.write_bai(bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=cc.designed_refgene())
        fa = os.path.join(tmp, "panel.fa")
        with open(fa, "wb") as f:
            f.write(fasta_text(B, C, D).encode())
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        base = [BIN, "-i", bam, "-n", side["nib"], "-fast"]
        runs = {}
        for name, extra in (("a", ["-all", "-cliploci"]), ("b", ["-all", "-cliploci", "-lociseq"]), ("c", ["-all", "-cliploci", "-lociseq", "-panel", fa]),
                            ("d", ["-cliploci", "-lociseq", "-conslen", "30", "-panel", fa, "-panelseed", "16"]),
                            ("e", ["-cliploci", "-locisupport", "1000", "-lociseq", "-panel", fa])):
            r = subprocess.run(base + ["-o", os.path.join(tmp, name)] + extra, env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            runs[name] = r
        yield dict(tmp=tmp, cols=cols, clusters=clusters, reads=reads, fa=fa, runs=runs, base=base, env=env, elements=(B, C, D))


def expected_seq_file(cli, conslen=64, seed=None, min_reads=3):
    """(the text of <prefix>_cliploci_seq.txt, the lociseq line, the panel line or None, the rows' fields)"""
    cols = cli["cols"]
    rows, _ = lc.both(cols, TLEN, QUAL, 10, 2, 50, min_reads, cli["clusters"])
    endpos = cc.rec_endpos(cols)
    written = list(lc.written(rows))
    sites = kc.as_sites([(int(rows[i]["tid"]), int(rows[i]["pos"]), 0, int(rows[i]["dir"])) for i in written])
    crow, cbases, _ = kc.expected_consensus(cli["reads"], sites, QUAL, 10, conslen, 2) if written else (np.zeros(0, abi.CONSENSUS), np.zeros((0, conslen), np.uint8), None)
    names, seqs = sm.read_fasta(cli["fa"])
    texts = [bytes(cbases[k, :int(crow[k]["len"])]).decode() for k in range(len(written))]
    hits = sm.expected_hits(seqs, texts, seed, reversed_=[int(s["dir"]) for s in sites]) if seed else None
    at = {i: k for k, i in enumerate(written)}
    lines, fields = ["\t".join(lc.COLUMNS + SEQ_COLUMNS + (PANEL_COLUMNS if seed else []))], []
    n_tail = n_hit = n_pairs = 0
    for k, i in enumerate(written):
        r = rows[i]
        tid, pos = int(r["tid"]), int(r["pos"])
        f = lc.row_fields(i, r, rows, NAMES, cc.single_base_depth(cols, endpos, tid, pos), "intergenic")
        f += kc.side_text(crow[k], cbases[k], int(r["dir"]))
        t = texts[k]
        lead = len(t) - len(t.lstrip(t[0])) if t else 0
        f.append(t[0] + str(lead) if t else ".")
        n_tail += lead >= 10
        if seed:
            h = hits[k]
            if int(h["found"]):
                n_hit += 1
                span = "."
                m = int(r["mate"])
                if int(r["flags"]) & 1 and m in at and int(hits[at[m]]["found"]) and int(hits[at[m]]["seq"]) == int(h["seq"]) and int(hits[at[m]]["orient"]) == int(h["orient"]):
                    left, right = (h, hits[at[m]]) if int(r["dir"]) == 0 else (hits[at[m]], h)
                    assert int(rows[m]["dir"]) != int(r["dir"])
                    if int(h["orient"]):
                        span = str(int(left["s_start"]) + int(left["len"]) - int(right["s_start"]))
                    else:
                        span = str(int(right["s_start"]) + int(right["len"]) - int(left["s_start"]))
                    n_pairs += int(r["dir"]) == 0
                f += [names[int(h["seq"])], "-" if int(h["orient"]) else "+", str(int(h["score"])), str(int(h["len"])), str(int(h["mism"])), str(int(h["run"])), str(int(h["q_start"]) + 1),
                      str(int(h["s_start"]) + 1), str(int(h["s_start"]) + int(h["len"])), str(int(h["n_seeds"])), names[int(h["seq2"])] if int(h["seq2"]) >= 0 else ".", str(int(h["score2"])), span]
            else:
                f += ["."] * 9 + ["0"] + ["."] * 3
        lines.append("\t".join(f))
        fields.append(f)
    lociseq = "lociseq: %d loci, %d with a sequence, %d with a tail of 10 or more" % (len(written), sum(1 for t in texts if t), n_tail)
    panel = "panel: %d sequences, %d bases, %d loci with a hit, %d pairs on one sequence" % (len(names), sum(len(s) for s in seqs), n_hit, n_pairs) if seed else None
    return "\n".join(lines) + "\n", lociseq, panel, fields


def test_lociseq_file(cli):
    text, lociseq, _, fields = expected_seq_file(cli)
    got = open(os.path.join(cli["tmp"], "b_cliploci_seq.txt")).read()
    assert got == text, (got, text)
    B, C, _ = cli["elements"]
    by = {(f[2], f[3]): f for f in fields}
    n = len(lc.COLUMNS)
    assert by[("1200000", "L")][n:n + 5] == ["4", "40", "1.000", B[:40], B[0] + "1"]
    assert by[("1199991", "R")][n:n + 5] == ["3", "40", "1.000", B[-40:], "A20"]  # the poly-A next to the junction
    assert by[("1300000", "L")][n + 3] == sm.revcomp(C)[:40] and by[("1299991", "R")][n + 3] == sm.revcomp(C)[-40:]
    assert ("1500000", "R") in by and ("1600000", "L") not in by and len(fields) == 5
    out = cli["runs"]["b"].stdout.split("\n")
    assert lociseq in out and lociseq.endswith("5 loci, 5 with a sequence, 1 with a tail of 10 or more") and not any(l.startswith("panel:") for l in out)
    # the table without the new columns is the other file, line for line
    plain = open(os.path.join(cli["tmp"], "b_cliploci.txt")).read().split("\n")
    assert ["\t".join(l.split("\t")[:n]) for l in got.split("\n")] == plain


def test_panel_columns(cli):
    text, lociseq, panel, fields = expected_seq_file(cli, seed=12)
    got = open(os.path.join(cli["tmp"], "c_cliploci_seq.txt")).read()
    assert got == text, (got, text)
    B, C, D = cli["elements"]
    by = {(f[2], f[3]): f for f in fields}
    n = len(lc.COLUMNS) + 5
    assert by[("1200000", "L")][n:] == ["ELEM_B", "+", "40", "40", "0", "40", "1", "1", "40", "3", "ELEM_D", "27", "210"]
    assert by[("1199991", "R")][n:] == ["ELEM_B", "+", "40", "40", "0", "40", "1", "171", "210", "17", ".", "0", "210"]
    assert by[("1300000", "L")][n:n + 2] == ["ELEM_C", "-"] and by[("1300000", "L")][n + 7:n + 9] == ["111", "150"] and by[("1300000", "L")][-1] == "150"
    assert by[("1299991", "R")][n:n + 2] == ["ELEM_C", "-"] and by[("1299991", "R")][n + 7:n + 9] == ["1", "40"] and by[("1299991", "R")][-1] == "150"
    assert by[("1500000", "R")][n:] == ["."] * 9 + ["0"] + ["."] * 3
    out = cli["runs"]["c"].stdout.split("\n")
    assert lociseq in out and panel in out and panel == "panel: 3 sequences, %d bases, 4 loci with a hit, 2 pairs on one sequence" % (len(B) + len(C) + 4 + len(D))
    # -panelseed 16 and -conslen 30, without -all: the runner-up of the first row is gone, the poly-A row has fewer seeds
    text, lociseq, panel, fields = expected_seq_file(cli, conslen=30, seed=16)
    got = open(os.path.join(cli["tmp"], "d_cliploci_seq.txt")).read()
    assert got == text, (got, text)
    by = {(f[2], f[3]): f for f in fields}
    assert by[("1200000", "L")][n:] == ["ELEM_B", "+", "30", "30", "0", "30", "1", "1", "30", "1", ".", "0", "210"]
    assert by[("1199991", "R")][n:n + 4] == ["ELEM_B", "+", "30", "30"] and by[("1199991", "R")][n + 9] == "9"
    assert lociseq in cli["runs"]["d"].stdout.split("\n") and panel in cli["runs"]["d"].stdout.split("\n")


def test_a_run_without_a_written_locus(cli):
    text, lociseq, panel, fields = expected_seq_file(cli, seed=12, min_reads=1000)
    assert not fields and text == "\t".join(lc.COLUMNS + SEQ_COLUMNS + PANEL_COLUMNS) + "\n"
    assert open(os.path.join(cli["tmp"], "e_cliploci_seq.txt")).read() == text
    out = cli["runs"]["e"].stdout.split("\n")
    assert "lociseq: 0 loci, 0 with a sequence, 0 with a tail of 10 or more" in out and panel in out and panel.endswith("0 loci with a hit, 0 pairs on one sequence")


def test_every_other_file_is_unchanged(cli):
    tmp = cli["tmp"]
    files = sorted(f[2:] for f in os.listdir(tmp) if f.startswith("a_"))
    assert "fusion.txt" in files and "fusion_all.txt" in files and "cliploci.txt" in files and "params.txt" in files
    a = os.path.join(tmp, "a")
    for name, tail, lines in (("b", "lociseq\t64\n", ("lociseq:",)), ("c", "lociseq\t64\npanel_file\t%s\npanel_seed\t12\n" % cli["fa"], ("lociseq:", "panel:"))):
        b = os.path.join(tmp, name)
        assert sorted(f[2:] for f in os.listdir(tmp) if f.startswith(name + "_")) == sorted(files + ["cliploci_seq.txt"])
        for f in files:
            ta, tb = open(os.path.join(tmp, "a_" + f), "rb").read(), open(os.path.join(tmp, name + "_" + f), "rb").read()
            if f == "params.txt":
                assert tb.decode() == ta.decode().replace("out_file\t" + a, "out_file\t" + b) + tail
            elif f == "performance.txt":  # (the last four columns are times)
                assert [l.split("\t")[:5] for l in ta.decode().split("\n")] == [l.split("\t")[:5] for l in tb.decode().split("\n")]
            else:
                assert ta.replace(a.encode(), b.encode()) == tb, f
        quiet = lambda out: [l for l in out.split("\n") if "costs time" not in l and not l.startswith(lines)]  # noqa: E731
        assert quiet(cli["runs"]["a"].stdout) == quiet(cli["runs"][name].stdout.replace(b, a))
        assert [l for l in cli["runs"][name].stdout.split("\n") if l.startswith(lines)] and not [l for l in cli["runs"]["a"].stdout.split("\n") if l.startswith(("lociseq:", "panel:"))]
    assert open(os.path.join(tmp, "d_params.txt")).read().endswith("lociseq\t30\npanel_file\t%s\npanel_seed\t16\n" % cli["fa"])


def test_refusals_and_fasta_errors(cli):
    tmp = cli["tmp"]
    base = cli["base"] + ["-o", os.path.join(tmp, "z")]
    fa = cli["fa"]
    for args, word in ((["-lociseq"], "-lociseq needs -cliploci."), (["-cliploci", "-panel", fa], "-panel and -panelseed need -lociseq."),
                       (["-cliploci", "-panelseed", "12"], "-panel and -panelseed need -lociseq."), (["-cliploci", "-lociseq", "-panelseed", "12"], "-panelseed needs -panel."),
                       (["-cliploci", "-lociseq", "-panel", fa, "-panelseed", "7"], "-panelseed must be a number from 8 to 16."),
                       (["-cliploci", "-lociseq", "-panel", fa, "-panelseed", "17"], "-panelseed must be a number from 8 to 16."),
                       (["-cliploci", "-lociseq", "-conslen", "257"], "-conslen must be a number from 1 to 256."), (["-cliploci", "-conslen", "30"], "-conslen needs -consensus."),
                       (["-cliploci", "-lociseq", "-gpus", "2"], "-cliploci cannot be combined with -gpus."), (["-lociseq", "-gpus", "2"], "-lociseq needs -cliploci.")):
        r = subprocess.run(base + args, env=cli["env"], capture_output=True, text=True)
        assert r.returncode == 1 and [l for l in r.stderr.split("\n") if "Error" in l] == [" Error: " + word], (args, r.stderr[-500:])
    r = subprocess.run(base + ["-cliploci", "-lociseq", "-panel", os.path.join(tmp, "none.fa")], env=cli["env"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: can not open panel file: " in r.stderr
    bad = os.path.join(tmp, "bad.fa")
    for text, line, what in ((b"ACGT\n>a\nAC\n", 1, "sequence data before the first header"), (b">a\nAC\n>b x\nAC\n\n>a y\nGG\n", 6, "duplicate sequence name a"),
                             (b">a\n>b\nAC\n", 1, "sequence a has no bases"), (b">a\nAC\n>b\n\n", 3, "sequence b has no bases")):
        with open(bad, "wb") as f:
            f.write(text)
        with pytest.raises(ValueError, match="line %d: " % line):
            sm.read_fasta(bad)
        r = subprocess.run(base + ["-cliploci", "-lociseq", "-panel", bad], env=cli["env"], capture_output=True, text=True)
        assert r.returncode == 1 and "Error: panel file %s line %d: %s" % (bad, line, what) in r.stderr, r.stderr[-500:]
    assert not any(f.startswith("z_") for f in os.listdir(tmp))

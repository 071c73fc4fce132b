"""The definition of bk_sequence_match (tests/seqmatchcases.py) against the hand examples of include/breakid_hip.h, its invariants
on drawn panels, and the FASTA rules of `-panel`.  No GPU."""
import numpy as np
import pytest

from breakid_amd import abi
from tests import seqmatchcases as sm

FIELDS = ("found", "seq", "orient", "score", "len", "mism", "run", "q_start", "s_start", "n_seeds", "seq2", "score2")


def row(r):
    return tuple(int(r[f]) for f in FIELDS)


def test_layouts():
    assert abi.SEQ_PROBE.itemsize == 8 and abi.SEQ_HIT.itemsize == 48
    assert abi.SEQ_HIT.names == FIELDS


def test_hand_examples():
    q = "TTTTTTTTTGGTGGCTCACGCCTGTAATCC"
    got = sm.expected_hits(sm.HAND_PANEL, [q, "GGTGGCTCACGC", "GGTGGCTCACG"], 12)
    assert row(got[0]) == (1, 1, 1, 30, 30, 0, 30, 0, 18, 2, 0, 21)
    # sequence 2 differs in one base that leaves two runs of 9: against it alone nothing is found
    assert row(sm.expected_hits(sm.HAND_PANEL[2:], [q], 12)[0])[:2] == (0, -1)
    r = got[1]
    assert (int(r["found"]), int(r["seq"]), int(r["s_start"]), int(r["score"]), int(r["n_seeds"]), int(r["seq2"]), int(r["score2"])) == (1, 0, 10, 12, 2, 1, 12)
    assert row(got[2]) == (0, -1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0)
    poly = sm.expected_hits(["C" + "A" * 20 + "G"], ["A" * 15], 12)[0]
    assert (int(poly["score"]), int(poly["s_start"]), int(poly["n_seeds"]), int(poly["len"]), int(poly["orient"])) == (15, 1, 12, 15, 0)


def test_the_model_reads_reversed_and_orientation_one():
    t = sm.draw(np.random.default_rng(3), 40)
    panel = ["ACGT" * 3 + t + "TTGA" * 3]
    fwd, rc = sm.expected_hits(panel, [t[5:35], sm.revcomp(t[5:35])], 12)
    assert row(fwd)[:9] == (1, 0, 0, 30, 30, 0, 30, 0, 17) and row(rc)[:9] == (1, 0, 1, 30, 30, 0, 30, 0, 17)
    # the same bytes read backwards are another string: reversed = 1 on the reversed bytes gives the forward answer
    back = sm.expected_hits(panel, [t[5:35][::-1]], 12, reversed_=[1])[0]
    assert back.tobytes() == fwd.tobytes()
    # q_start in orientation 1: five N, which match nothing, in front of the query move the segment in q, not on the panel
    shifted = sm.expected_hits(panel, ["NNNNN" + sm.revcomp(t[5:35])], 12)[0]
    assert (int(shifted["orient"]), int(shifted["q_start"]), int(shifted["s_start"]), int(shifted["len"])) == (1, 5, 17, 30)


@pytest.mark.parametrize("seed", [8, 12, 16])
def test_invariants(seed):
    rng = np.random.default_rng(seed)
    seqs = sm.drawn_panel(rng, 12, 6000)
    queries = sm.cut_queries(rng, seqs, 20, 48, 0.0) + sm.cut_queries(rng, seqs, 20, 48, 0.1) + [sm.draw(rng, 48) for _ in range(10)] + ["A" * 40, "ACGTN" * 8]
    got = sm.expected_hits(seqs, queries, seed)
    assert (got["found"] == (got["n_seeds"] > 0)).all()
    assert (got["score"] <= got["len"]).all() and (got["mism"] * 3 == got["len"] - got["score"]).all()
    for r in got:
        if int(r["seq2"]) >= 0 and int(r["seq2"]) < int(r["seq"]):
            assert int(r["score2"]) <= int(r["score"])
        if not int(r["found"]):
            assert row(r) == (0, -1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0)
        else:
            assert int(r["run"]) >= seed and int(r["score"]) >= seed and int(r["score2"]) <= int(r["score"])
    assert (got["found"][:20] == 1).all() and (got["score"][:20] == 48).all()  # the exact cuts are found whole
    assert got["found"][50] == 1  # the poly-A query meets the tails


def test_kmer_count_of_the_byte_model():
    p = sm.Panel(["ACGTACGTACGT", "ACGTNACGTACGTA", "ACG", ""])
    assert p.kmers(8) == 5 + 2 and p.kmers(12) == 1 and p.kmers(16) == 0
    off, bases = p.arrays()
    assert list(off) == [0, 12, 26, 29, 29] and bytes(bases[12:17]) == b"ACGTN"


def test_fasta_rules(tmp_path):
    f = tmp_path / "p.fa"
    f.write_bytes(b"\n>one first sequence\nacgtn\n\nRYACGT\r\n>two\nAC GT\n")
    names, seqs = sm.read_fasta(str(f))
    assert names == ["one", "two"] and seqs == ["ACGTNNNACGT", "ACNGT"]
    for text, line, what in ((b"ACGT\n>a\nAC\n", 1, "before the first header"), (b">a\nAC\n>b\nAC\n\n>a\nGG\n", 6, "duplicate"), (b">a\n>b\nAC\n", 1, "no bases"),
                             (b">a\nAC\n>b\n\n", 3, "no bases")):
        f.write_bytes(text)
        with pytest.raises(ValueError, match="line %d: .*%s" % (line, what)):
            sm.read_fasta(str(f))

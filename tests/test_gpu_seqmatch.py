"""Sequence match (`bk_sequence_match`): the index and the extension kernel against the brute force of tests/seqmatchcases.py, byte for
byte: the seed's range and its edges, the ends of a sequence and the join of two, N on either side, both orientations and `reversed`,
one designed case per level of the tie rule, seq2 / score2, a best segment off its seed, repeated k-mers, the sizes of the probe list
and a panel whose sort spans several tiles; two runs and a permuted probe list; a clip consensus fed in as it lies; errors, limits,
timing and an unchanged bk_fetch."""
import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import callcases as cc
from tests import consensuscases as kc
from tests import seqmatchcases as sm

pytestmark = pytest.mark.gpu
QUAL = cc.QUAL
FIELDS = abi.SEQ_HIT.names
NONE = (0, -1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0)


@pytest.fixture(scope="module")
def ctx():
    t = capi.Context(cc.CONTIGS)  # any live context: no table, no stage
    yield t
    t.close()


def row(r):
    return tuple(int(r[f]) for f in FIELDS)


def assert_rows(got, exp):
    assert got.dtype == abi.SEQ_HIT and len(got) == len(exp)
    bad = [k for k in range(len(exp)) if got[k].tobytes() != exp[k].tobytes()]
    assert not bad, [(k, got[k], exp[k]) for k in bad[:5]]


def check(ctx, seqs, queries, seed, reversed_=None, max_len=None):
    """the device's rows, after they were found equal to the definition's"""
    panel = seqs if isinstance(seqs, sm.Panel) else sm.Panel(seqs)
    probes, query = sm.pack(queries, max_len, reversed_)
    got = ctx.sequence_match(panel.arrays(), probes, query, seed)
    assert_rows(got, sm.expected_hits(panel, queries, seed, reversed_))
    return got


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


# ---- 1. the header's examples ---------------------------------------------------------------------------------------------------------
def test_hand_examples(ctx):
    got = check(ctx, sm.HAND_PANEL, ["TTTTTTTTTGGTGGCTCACGCCTGTAATCC", "GGTGGCTCACGC", "GGTGGCTCACG"], 12)
    assert row(got[0]) == (1, 1, 1, 30, 30, 0, 30, 0, 18, 2, 0, 21)
    assert row(got[1]) == (1, 0, 0, 12, 12, 0, 12, 0, 10, 2, 1, 12)
    assert row(got[2]) == NONE
    poly = check(ctx, ["C" + "A" * 20 + "G"], ["A" * 15], 12)[0]
    assert (int(poly["score"]), int(poly["s_start"]), int(poly["n_seeds"])) == (15, 1, 12)


# ---- 2. the seed ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [8, 12, 16])
def test_seed_edges(ctx, seed):
    rng = np.random.default_rng(100 + seed)
    P = sm.draw(rng, 400)
    a = 150
    # a copy of `seed` bases between two bases that differ from the panel's, and the same with its last base changed too
    exact = other(P[a - 1]) + P[a:a + seed] + other(P[a + seed])
    short = other(P[a - 1]) + P[a:a + seed - 1] + other(P[a + seed - 1]) + other(P[a + seed])
    got = check(ctx, [P], [exact, short, P[a:a + seed - 1], P[a:a + seed], sm.revcomp(exact)], seed)
    assert row(got[0])[:9] == (1, 0, 0, seed, seed, 0, seed, 1, a) and int(got[0]["n_seeds"]) == 1
    assert row(got[1]) == NONE and row(got[2]) == NONE  # a run of seed - 1; qlen = seed - 1
    assert row(got[3])[:9] == (1, 0, 0, seed, seed, 0, seed, 0, a)  # qlen = seed
    assert row(got[4])[:9] == (1, 0, 1, seed, seed, 0, seed, 1, a)
    # qlen = max_len = 256: the whole of it, and with a substitution every 15 bases (runs of 14: seeded at 8 and 12 only)
    long_q = P[100:356]
    dotted = "".join(other(c) if i % 15 == 14 else c for i, c in enumerate(long_q))
    got = check(ctx, [P], [long_q, dotted, sm.revcomp(dotted)], seed, max_len=256)
    assert row(got[0])[:9] == (1, 0, 0, 256, 256, 0, 256, 0, 100)
    assert (int(got[1]["n_seeds"]) >= 17 if seed <= 14 else int(got[1]["n_seeds"]) == 0) and int(got[2]["n_seeds"]) == int(got[1]["n_seeds"])
    # max_len 1: nothing can be found, and nothing is read behind the one byte
    assert all(row(r) == NONE for r in check(ctx, [P], ["A", "C", "", "N"], seed, max_len=1))


# ---- 3. the ends of a sequence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [8, 12, 16])
def test_sequence_edges(ctx, seed):
    rng = np.random.default_rng(200 + seed)
    A, B = sm.draw(rng, 90), sm.draw(rng, 70)
    h = seed // 2
    seqs = [A, B, "ACGTACG", "", sm.draw(rng, seed - 1), A[:seed - 1]]
    queries = [A[-h:] + B[:seed - h],                    # exists only across the join: not found
               A[:seed], A[-seed:], B[:seed], B[-seed:],  # a seed in a sequence's first and last bases
               sm.draw(rng, 7) + A[:30],                 # overhangs the start: d < 0
               B[-30:] + sm.draw(rng, 9),                # overhangs the end: d > len_s - qlen
               "N" * 5 + B[:20] + "N" * 5, A + B]
    got = check(ctx, seqs, queries, seed)
    assert row(got[0]) == NONE
    assert [(int(r["seq"]), int(r["s_start"]), int(r["score"])) for r in got[1:5]] == [(0, 0, seed), (0, 90 - seed, seed), (1, 0, seed), (1, 70 - seed, seed)]
    assert (int(got[5]["seq"]), int(got[5]["q_start"]), int(got[5]["s_start"]), int(got[5]["score"])) == (0, 7, 0, 30)
    assert (int(got[6]["seq"]), int(got[6]["q_start"]), int(got[6]["s_start"]), int(got[6]["score"])) == (1, 0, 40, 30)
    assert (int(got[8]["seq"]), int(got[8]["score"]), int(got[8]["seq2"]), int(got[8]["score2"])) == (0, 90, 1, 70)
    # nothing but short and empty sequences; no sequence at all
    assert all(row(r) == NONE for r in check(ctx, ["ACGTACG", "", A[:seed - 1]], queries, seed))
    probes, query = sm.pack(queries)
    none = ctx.sequence_match((np.zeros(1, np.uint64), np.zeros(0, np.uint8)), probes, query, seed)
    assert all(row(r) == NONE for r in none)


def test_n_never_matches(ctx):
    rng = np.random.default_rng(5)
    P = sm.draw(rng, 200)
    holed = P[:60] + "N" + P[61:]  # an N inside every k-mer that would seed the first query
    q = P[50:72]
    got = check(ctx, [holed, "N" * 40], [q, q[:10] + "N" + q[11:], "N" * 30, P[100:130], P[100:110] + "N" + P[111:140]], 12)
    assert row(got[0]) == NONE and row(got[1]) == NONE and row(got[2]) == NONE  # runs of 10 and 11 around the N; N against N
    assert (int(got[3]["score"]), int(got[3]["mism"])) == (30, 0)
    assert (int(got[4]["score"]), int(got[4]["len"]), int(got[4]["mism"]), int(got[4]["run"])) == (37, 40, 1, 29)  # an N in the query is a mismatch


# ---- 4. orientation -------------------------------------------------------------------------------------------------------------------
def test_orientation_and_reversed(ctx):
    rng = np.random.default_rng(6)
    t = sm.draw(rng, 60)
    panel = [sm.draw(rng, 33) + t + sm.draw(rng, 21)]
    piece = t[5:45]
    texts = [piece, piece[::-1], piece[::-1], sm.revcomp(piece), "N" * 5 + sm.revcomp(piece), sm.revcomp(piece)[::-1]]
    got = check(ctx, panel, texts, 12, reversed_=[0, 0, 1, 0, 0, 1])
    assert row(got[0])[:9] == (1, 0, 0, 40, 40, 0, 40, 0, 38)
    assert row(got[1]) == NONE                                   # the same bytes backwards are another string ...
    assert got[2].tobytes() == got[0].tobytes()                  # ... and `reversed` reads them forwards again
    assert row(got[3])[:9] == (1, 0, 1, 40, 40, 0, 40, 0, 38)    # a hit in orientation 1 only
    assert row(got[4])[:9] == (1, 0, 1, 40, 40, 0, 40, 5, 38)    # q_start counts in q
    assert got[5].tobytes() == got[3].tobytes()
    # a reverse palindrome matches in both orientations at the same place: orientation 0 wins
    half = sm.draw(rng, 11)
    pal = half + sm.revcomp(half)
    r = check(ctx, [sm.draw(rng, 20) + pal + sm.draw(rng, 20)], [pal], 12)[0]
    assert row(r)[:9] == (1, 0, 0, 22, 22, 0, 22, 0, 20) and int(r["n_seeds"]) == 2 and int(r["seq2"]) == -1


# ---- 5. one case per level of the key; seq2 and score2 ---------------------------------------------------------------------------------
def test_tie_rules(ctx):
    rng = np.random.default_rng(7)
    Q = sm.draw(rng, 33)
    junk = lambda n: sm.draw(rng, n)  # noqa: E731
    # the score: a copy with one substitution in an earlier sequence loses to the exact one
    sub = Q[:16] + other(Q[16]) + Q[17:]
    r = check(ctx, [junk(10) + sub + junk(10), junk(14) + Q + junk(3)], [Q], 12)[0]
    assert row(r) == (1, 1, 0, 33, 33, 0, 33, 0, 14, 3, 0, 30)
    # the length: 33 cells with one mismatch and 30 exact ones both score 30; the shorter wins, in the later sequence
    cut = Q[:30] + other(Q[30]) + other(Q[31]) + other(Q[32])
    r = check(ctx, [junk(10) + sub + junk(10), junk(14) + cut + junk(3)], [Q], 12)[0]
    assert row(r) == (1, 1, 0, 30, 30, 0, 30, 0, 14, 3, 0, 30)
    mid = Q[:15] + other(Q[15]) + Q[16:]  # 15 + 17 around the mismatch: the whole scores 30 over 33 cells and no part more
    r = check(ctx, [junk(10) + other(Q[0]) + mid[1:] + junk(10), junk(14) + cut + junk(3)], [Q], 12)[0]
    assert (int(r["seq"]), int(r["score"]), int(r["len"]), int(r["seq2"]), int(r["score2"])) == (1, 30, 30, 0, 29)
    r = check(ctx, [junk(10) + mid + junk(10), junk(14) + cut + junk(3)], [Q], 12)[0]
    assert (int(r["seq"]), int(r["score"]), int(r["len"]), int(r["mism"]), int(r["seq2"]), int(r["score2"])) == (1, 30, 30, 0, 0, 30)  # equal score, the winner not the smallest index
    # the sequence: the same copy in two sequences
    r = check(ctx, [junk(40), junk(9) + Q + junk(5), junk(2) + Q + junk(5)], [Q], 12)[0]
    assert row(r) == (1, 1, 0, 33, 33, 0, 33, 0, 9, 2, 2, 33)
    # the orientation: forward in one place and reverse-complemented in an earlier one of the same sequence
    r = check(ctx, [junk(4) + sm.revcomp(Q) + junk(20) + Q + junk(5)], [Q], 12)[0]
    assert row(r) == (1, 0, 0, 33, 33, 0, 33, 0, 57, 2, -1, 0)
    # the start on the panel: two copies in one sequence
    r = check(ctx, [junk(4) + Q + junk(20) + Q + junk(5)], [Q], 12)[0]
    assert row(r) == (1, 0, 0, 33, 33, 0, 33, 0, 4, 2, -1, 0)
    # the start in the query: the query holds the panel's stretch twice
    T = Q[:15]
    r = check(ctx, [junk(20) + other(T[0]) + T[1:] + junk(20)], [T[1:] + "N" + T[1:]], 12)[0]
    assert row(r) == (1, 0, 0, 14, 14, 0, 14, 0, 21, 2, -1, 0)
    # seq2: none; below the winner; in a later and in an earlier sequence
    r = check(ctx, [junk(50), junk(9) + Q + junk(5), junk(30) + other(sm.revcomp(Q[25])) + sm.revcomp(Q[3:25]) + other(sm.revcomp(Q[2])) + junk(5)], [Q], 12)[0]
    assert row(r) == (1, 1, 0, 33, 33, 0, 33, 0, 9, 2, 2, 22)


def test_best_segment_off_the_seed(ctx):
    """a diagonal seeded by a run of 12 whose best segment, 11 + 1 + 11 cells of score 20, lies elsewhere on it"""
    rng = np.random.default_rng(8)
    P = sm.draw(rng, 120)
    a = 30
    q = list(P[a:a + 48])
    for i in range(12, 18):
        q[i] = other(q[i])   # six mismatches behind the run of 12: the sum is back at 0
    q[29] = other(q[29])     # 18 .. 28, a mismatch, 30 .. 40
    for i in range(41, 48):
        q[i] = other(q[i])
    r = check(ctx, [P], ["".join(q)], 12)[0]
    assert row(r) == (1, 0, 0, 20, 23, 1, 12, 18, a + 18, 1, -1, 0)


# ---- 6. repeated k-mers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [1, 64, 65, 200])
def test_a_kmer_that_the_panel_holds_many_times(ctx, copies):
    rng = np.random.default_rng(300 + copies)
    U = sm.draw(rng, 16)
    parts = []
    for c in range(copies):  # every copy between bases that differ from the query's around it
        parts.append(sm.draw(rng, int(rng.integers(3, 9))) + "G" + U + "C")
    seqs = ["".join(parts[:copies // 2]) + "ACGT", "".join(parts[copies // 2:]) + "ACGT"]
    got = check(ctx, seqs, ["T" + U + "A", sm.revcomp("T" + U + "A"), U[:13]], 12)
    assert int(got[0]["n_seeds"]) == copies and int(got[1]["n_seeds"]) == copies and int(got[0]["score"]) == 16
    assert int(got[2]["n_seeds"]) >= copies


def test_poly_a_against_poly_a(ctx):
    seqs = ["A" * 300, "C" + "A" * 30 + "G", "T" * 25]
    got = check(ctx, seqs, ["A" * 64, "A" * 256, "T" * 40, "A" * 11], 12, max_len=256)
    assert int(got[0]["n_seeds"]) == (300 + 64 - 1 - 2 * 11) + (30 + 64 - 1 - 2 * 11) + (25 + 64 - 1 - 2 * 11)
    assert row(got[0])[:9] == (1, 0, 0, 64, 64, 0, 64, 0, 0) and row(got[3]) == NONE


# ---- 7. sizes --------------------------------------------------------------------------------------------------------------------------
_BIG = {}


def big():
    """a panel of about 70 000 drawn bases in 40 sequences (the sort spans several tiles); 300 queries of 64 bases cut from it with
    substitutions at 0 %, 5 % and 15 %, and 50 drawn ones; the definition's rows, computed once"""
    if not _BIG:
        rng = np.random.default_rng(11)
        seqs = sm.drawn_panel(rng)
        queries = sm.cut_queries(rng, seqs, 100, 64, 0.0) + sm.cut_queries(rng, seqs, 100, 64, 0.05) + sm.cut_queries(rng, seqs, 100, 64, 0.15)
        queries += [sm.draw(rng, 64) for _ in range(50)]
        order = rng.permutation(len(queries))
        queries = [queries[i] for i in order]
        panel = sm.Panel(seqs)
        _BIG.update(panel=panel, queries=queries, exp=sm.expected_hits(panel, queries, 12), cut=order < 300, exact=order < 100)
    return _BIG


def test_a_panel_of_several_sort_tiles(ctx):
    b = big()
    assert 40 * 256 < b["panel"].kmers(12) and len(b["panel"].seqs) == 40
    probes, query = sm.pack(b["queries"])
    got = ctx.sequence_match(b["panel"].arrays(), probes, query, 12)
    assert_rows(got, b["exp"])
    assert (got["score"][b["exact"]] == 64).all() and got["found"][b["cut"]].sum() > 280
    assert len({int(s) for s in got["seq"][b["cut"]]}) > 30 and {int(o) for o in got["orient"][b["cut"]]} == {0, 1}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_counts(ctx, n):
    b = big()
    probes, query = sm.pack(b["queries"][:n], 64)
    assert_rows(ctx.sequence_match(b["panel"].arrays(), probes, query, 12), b["exp"][:n])


@pytest.mark.parametrize("seed", [8, 16])
def test_the_other_seeds_on_the_large_panel(ctx, seed):
    b = big()
    queries = b["queries"][:40]
    check(ctx, b["panel"], queries, seed)


# ---- 8. same bytes ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_permuted_probe_list_give_the_same_bytes(ctx):
    b = big()
    probes, query = sm.pack(b["queries"], 64)
    first = ctx.sequence_match(b["panel"].arrays(), probes, query, 12)
    again = ctx.sequence_match(b["panel"].arrays(), probes, query, 12)
    perm = np.random.default_rng(9).permutation(len(probes))
    moved = ctx.sequence_match(b["panel"].arrays(), probes[perm], query[perm], 12)
    assert first.tobytes() == again.tobytes() and first[perm].tobytes() == moved.tobytes()


# ---- 9. a clip consensus as it lies ------------------------------------------------------------------------------------------------------
def test_consensus_bases_feed_the_match(ctx):
    reads, sites = kc.designed_reads(), kc.designed()["sites"]
    rows, bases, _ = ctx.clip_consensus(reads, sites, QUAL, kc.MIN_CLIP, kc.MAX_LEN, kc.MIN_DEPTH)
    rng = np.random.default_rng(12)
    texts = [bytes(bases[k, :int(rows[k]["len"])]).decode() for k in range(len(sites))]
    used = [k for k, t in enumerate(texts) if len(t) >= 20]
    assert len(used) >= 8 and {int(sites[k]["dir"]) for k in used} == {0, 1}
    # every other consensus lies in the panel as the reads read it (BAM orientation), the rest reverse-complemented
    bam = {k: texts[k][::-1] if int(sites[k]["dir"]) else texts[k] for k in used}
    seqs = [sm.draw(rng, 30) + (sm.revcomp(bam[k]) if j % 2 else bam[k]) + sm.draw(rng, 30) for j, k in enumerate(used)]
    probes = np.zeros(len(sites), abi.SEQ_PROBE)
    probes["qlen"], probes["reversed"] = rows["len"], sites["dir"]
    got = ctx.sequence_match(sm.Panel(seqs).arrays(), probes, bases, 12)  # bases and its stride unchanged
    assert_rows(got, sm.expected_hits(seqs, texts, 12, reversed_=sites["dir"]))
    for j, k in enumerate(used):
        if "N" not in texts[k]:
            assert (int(got[k]["found"]), int(got[k]["score"]), int(got[k]["q_start"])) == (1, len(texts[k]), 0), (k, got[k])


# ---- 10. errors, limits, empty inputs ----------------------------------------------------------------------------------------------------
def raw_call(t, off, bases, probes, query, max_len, seed, n=None, n_seqs=None, null=()):
    C = capi.C
    s = abi.SeqPanel()
    s.n_seqs = len(off) - 1 if n_seqs is None else n_seqs
    s.off = None if "off" in null else off.ctypes.data
    s.bases = None if "bases" in null else bases.ctypes.data
    out = C.c_void_p()
    rc = t.L.bk_sequence_match(None if "ctx" in null else t.h, None if "panel" in null else C.byref(s), None if "probes" in null else probes.ctypes.data,
                               len(probes) if n is None else n, None if "query" in null else query.ctypes.data, max_len, seed, None if "out" in null else C.byref(out))
    return rc, (t.L.bk_last_error(t.h) or b"").decode()


def test_argument_and_limit_errors(ctx):
    panel = sm.Panel(sm.HAND_PANEL)
    off, bases = panel.arrays()
    queries = ["TTTTTTTTTGGTGGCTCACGCCTGTAATCC", "GGTGGCTCACGC"]
    probes, query = sm.pack(queries, 32)
    assert raw_call(ctx, off, bases, probes, query, 32, 12)[0] == abi.BK_OK
    for null in ("ctx", "panel", "probes", "query", "out", "off", "bases"):
        assert raw_call(ctx, off, bases, probes, query, 32, 12, null=(null,))[0] == abi.BK_ERR_ARG, null
    assert raw_call(ctx, off, bases, probes, query, 32, 12, n=0, null=("probes", "query"))[0] == abi.BK_OK
    assert raw_call(ctx, off, bases, probes, query, 32, 12, n_seqs=0, null=("off", "bases"))[0] == abi.BK_OK
    big_query = np.zeros((2, 257), np.uint8)
    for max_len, seed, word in ((0, 12, "max_len"), (257, 12, "max_len"), (32, 7, "seed"), (32, 17, "seed")):
        rc, msg = raw_call(ctx, off, bases, probes, big_query, max_len, seed)
        assert rc == abi.BK_ERR_ARG and word in msg, msg

    def changed(a, index, value):
        b = a.copy()
        b.reshape(-1)[index] = value
        return b
    p2 = probes.copy()
    p2["qlen"][1] = 33
    p3 = probes.copy()
    p3["reversed"][0] = 2
    for args, word in (((off, bases, p2, query), "qlen above max_len"), ((off, bases, p3, query), "reversed above 1"),
                       ((off, bases, probes, changed(query, 32 + 3, ord("g"))), "query byte outside ACGTN in column 3"),
                       ((off, changed(bases, 40, ord("a")), probes, query), "panel byte 40"), ((off, changed(bases, 5, ord("R")), probes, query), "panel byte 5"),
                       ((changed(off, 0, 1), bases, probes, query), "start at 0"), ((changed(off, 1, int(off[2]) + 1), bases, probes, query), "does not ascend")):
        rc, msg = raw_call(ctx, *args, 32, 12)
        assert rc == abi.BK_ERR_ARG and word in msg and "bk_sequence_match" in msg, msg
    assert raw_call(ctx, off, bases, probes, changed(query, 32 + 12, ord("g")), 32, 12)[0] == abi.BK_OK  # a byte behind qlen is not looked at
    # the limits are looked at before any array: the small ones are never read beyond their end
    rc, msg = raw_call(ctx, off, bases, probes, query, 32, 12, n=(1 << 30) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^30 probes" in msg, msg
    rc, msg = raw_call(ctx, off, bases, probes, query, 32, 12, n_seqs=(1 << 20) + 1)
    assert rc == abi.BK_ERR_LIMIT and "2^20 sequences" in msg, msg
    rc, msg = raw_call(ctx, changed(off, 3, (1 << 28) + 1), bases, probes, query, 32, 12)
    assert rc == abi.BK_ERR_LIMIT and "2^28 panel bases" in msg, msg
    s = capi.Context(cc.CONTIGS)
    s.upload(cc.quiet_tumor().to_soa())
    s._check(s.L.bk_shard_begin(s.h, 0, QUAL))
    with pytest.raises(capi.BreakIDError, match="sharded contexts") as e:
        s.sequence_match(sm.HAND_PANEL, probes, query)
    assert e.value.code == abi.BK_ERR_ARG
    s.close()
    assert_rows(ctx.sequence_match(sm.HAND_PANEL, probes, query), sm.expected_hits(panel, queries, 12))  # the context still works
    none = ctx.sequence_match(sm.HAND_PANEL, np.zeros(0, abi.SEQ_PROBE), np.zeros((0, 32), np.uint8))
    assert len(none) == 0 and none.dtype == abi.SEQ_HIT


# ---- 11. timing and fetch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [8, 12, 16])
def test_match_is_timed(seed):
    rng = np.random.default_rng(13)
    seqs = sm.drawn_panel(rng, 7, 5000) + ["ACGTNACGTACGTACGTACGTA", "ACG", ""]
    panel = sm.Panel(seqs)
    probes, query = sm.pack(sm.cut_queries(rng, seqs, 30, 40, 0.05), 48)
    t = capi.Context(cc.CONTIGS)
    t.timing_enable(True)
    t.sequence_match(panel.arrays(), probes, query, seed)
    names = [name for name, _, _ in t.timing()]
    tm = {name: (ms, by) for name, ms, by in t.timing()}
    touched = dict(zip(names, t.timing_touched()))
    assert names == ["sequence_match", "sequence_match_index", "sequence_match_probes"]
    B, M, passes = sum(panel.lens), panel.kmers(seed), (2 * seed + 7) // 8
    assert touched["sequence_match_index"] == B + 36 * M * passes and touched["sequence_match_probes"] == 30 * (56 + 48)
    assert touched["sequence_match"] == touched["sequence_match_index"] + touched["sequence_match_probes"]
    assert all(tm[k][0] > 0 and tm[k][1] == touched[k] for k in names)
    assert tm["sequence_match"][0] >= tm["sequence_match_index"][0] and tm["sequence_match"][0] >= tm["sequence_match_probes"][0]
    t.close()


def test_a_later_fetch_is_unchanged():
    ds = kc.designed()["ds"]
    t = capi.Context(ds.contigs)
    t.upload(ds.to_soa())
    t.run(qual=QUAL, fast=True)
    before = [t.fetch(stage)[0].tobytes() for stage in (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)]
    probes, query = sm.pack(["TTTTTTTTTGGTGGCTCACGCCTGTAATCC"])
    got = t.sequence_match(sm.HAND_PANEL, probes, query)
    assert int(got[0]["seq"]) == 1
    assert [t.fetch(stage)[0].tobytes() for stage in (abi.STAGE_CLUSTERED, abi.STAGE_SPLITS, abi.STAGE_CLUSTERS)] == before
    t.close()

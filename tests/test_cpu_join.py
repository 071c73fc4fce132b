"""The mate-join cases of tests/joincases.py without a GPU: the plain Python model against the oracle (oracle/oracle.cc, the port of
scan_discordant_pairs) field for field on every case, and every case on the edge it is named for - where its runs land in the
join's sorted order, how many pairs a run gives, which runs of equal upper hash halves are mixed and how long they are."""
import os
import re

import numpy as np
import pytest

from breakid_amd import abi
from oracle import pyoracle
from tests import joincases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = jc.table_cases() + [jc.rec_bits_case()]
BY_NAME = {c.name: c for c in CASES}


def oracle_pairs(case, q=jc.QUAL):
    o = pyoracle.Oracle(case.contigs, case.cols)
    try:
        o.discordant_pairs(q, case.w)
        return o.fetch(abi.STAGE_SCAN)
    finally:
        o.close()


def test_constants_of_the_source():
    src = open(os.path.join(ROOT, "breakid_amd", "csrc", "join.hip")).read()
    assert re.search(r"constexpr uint32_t JOIN_FIX_MAX = %d;" % jc.JOIN_FIX_MAX, src)
    assert "__launch_bounds__(%d) void k_join_pairs" % jc.WG in src and "__launch_bounds__(%d) void k_join_fix_runs" % jc.WG in src
    assert "dim3(cdiv(n_cand, %d)), dim3(%d), 0, st, cand, ks, vs" % (jc.WG, jc.WG) in src


def test_case_names_and_sizes():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        n = len(c.cols["tid"])
        assert n < jc.MAX_RECORDS, c.name
        t, p = c.cols["tid"].astype(np.int64) & 0xFFFFFFFF, c.cols["pos"].astype(np.int64)
        assert not np.any((t[:-1] > t[1:]) | ((t[:-1] == t[1:]) & (p[:-1] > p[1:]))), c.name  # coordinate sorted
        h, k = c.cols["qhash"], c.cols["qcheck"]
        assert len(set(zip(h.tolist(), k.tolist()))) == len(set(h.tolist())), c.name  # one second hash per hash: no forged collision


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_model_equals_oracle(case):
    exp, eoff = oracle_pairs(case)
    got, goff = jc.model(case.contigs, case.cols, jc.QUAL, case.w)
    assert got.dtype == exp.dtype and len(got) == len(exp)
    for f in abi.PAIR.names:
        assert np.array_equal(got[f], exp[f]), (case.name, f)
    if len(exp):
        assert np.array_equal(goff, eoff), case.name
    else:
        assert eoff is None or list(eoff) == [0]


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("tag", ["ranked", "spread"])
def test_run_length_cases(L, tag):
    c = BY_NAME["runs_of_%d_%s" % (L, tag)]
    lay = jc.layout(c.cols)
    made = jc.pairs_per_run(c)
    runs = [(h, l) for h, _, l in lay if l == L]
    assert len(runs) >= 40
    if L == 1:
        assert all(made.get(h, 0) == 0 for h, _ in runs)
        return
    # an odd run leaves its last record unpaired; some run gives every pair it can, and (from four records on) some run loses a
    # pair to the gate and still pairs the records behind it: the failed pair consumed both of its records
    assert all(made.get(h, 0) <= L // 2 for h, _ in runs)
    assert any(made.get(h, 0) == L // 2 for h, _ in runs)
    if L >= 4:
        assert any(0 < made.get(h, 0) < L // 2 for h, _ in runs)
    if L >= 4:
        assert max(made.values()) >= 2  # one lane, several pairs: the first through LDS, the others direct
    # arrival order against hash order: the records of some run arrive between the records of runs on both sides of it
    if tag == "ranked":
        cand = np.nonzero(jc.candidate_mask(c.cols))[0]
        first = {}
        for i in cand:
            first.setdefault(int(c.cols["qhash"][i]), int(i))
        order = [first[h] for h, _, _ in lay]
        assert sum(1 for a, b in zip(order[:-1], order[1:]) if a > b) > len(order) // 4


def test_runs_across_workgroups():
    for name in ("run_of_2_across_workgroups", "run_of_5_across_workgroups"):
        c = BY_NAME[name]
        at, L = c.witness["run_at"]
        hit = [(h, a, l) for h, a, l in jc.layout(c.cols) if a == at]
        assert hit and hit[0][2] == L and at < jc.WG < at + L, name
        assert jc.pairs_per_run(c).get(hit[0][0], 0) == L // 2, name  # and the run does pair: the pairs come from the lane in front of the edge
    c = BY_NAME["workgroups_all_none_failing"]
    lay, made = jc.layout(c.cols), jc.pairs_per_run(c)
    wg = lambda k: [(h, a, l) for h, a, l in lay if k * jc.WG <= a < (k + 1) * jc.WG]
    assert len(lay) == 128 + 256 + 128 and sum(l for _, _, l in lay) == 3 * jc.WG
    assert all(l == 2 and made.get(h, 0) == 1 for h, _, l in wg(c.witness["full"])) and len(wg(c.witness["full"])) == jc.WG // 2
    assert all(l == 1 for _, _, l in wg(c.witness["single"])) and len(wg(c.witness["single"])) == jc.WG
    assert all(l == 2 and made.get(h, 0) == 0 for h, _, l in wg(c.witness["failing"])) and len(wg(c.witness["failing"])) == jc.WG // 2
    c = BY_NAME["several_pairs_from_one_lane"]
    lay, made = jc.layout(c.cols), jc.pairs_per_run(c)
    assert sorted(made.get(h, 0) for h, _, l in lay if l > 2) == [4, 6]


def test_shared_upper_halves():
    for total in (jc.JOIN_FIX_MAX - 1, jc.JOIN_FIX_MAX, jc.JOIN_FIX_MAX + 1):
        c = BY_NAME["mixed_run_of_%d" % total]
        runs = jc.upper_runs(c.cols)
        assert runs[0] == c.witness["upper_run"] and runs[0][1] == total and runs[0][2] > 1
        assert all(names == 1 for _, _, names in runs[1:])  # the only mixed run: nothing else decides whether the join starts over
        # the order the stable sort on the upper half leaves (arrival order) is not the order of the whole hashes
        cand = np.nonzero(jc.candidate_mask(c.cols))[0]
        h = c.cols["qhash"][cand]
        arrival = h[(h >> np.uint64(32)) == np.uint64(0x40000000)]
        assert len(arrival) == total and np.any(arrival[:-1] > arrival[1:])
    c = BY_NAME["one_name_run_of_%d" % jc.JOIN_FIX_MAX]
    assert jc.upper_runs(c.cols)[0] == (0, jc.JOIN_FIX_MAX, 1) and all(names == 1 for _, _, names in jc.upper_runs(c.cols))
    c = BY_NAME["mixed_run_across_workgroups"]
    a, l, names = c.witness["upper_run"]
    assert (a, l, names) in jc.upper_runs(c.cols) and a < jc.WG < a + l and names > 1


@pytest.mark.parametrize("w", [500, 350.5])
def test_gate_case(w):
    c = BY_NAME["gate_w_%s" % w]
    W = int(w)
    cols = c.cols
    pairs, _ = jc.model(c.contigs, cols, jc.QUAL, c.w)
    made = set(int(r) for r in pairs["rec"])
    cand = np.nonzero(jc.candidate_mask(cols))[0]
    by = {}
    for i in cand:
        by.setdefault(int(cols["qhash"][i]), []).append(int(i))
    seen = {}
    for a, b in by.values():
        same = cols["tid"][a] == cols["tid"][b]
        d = abs(int(cols["pos"][a]) - int(cols["pos"][b]))
        if same:
            seen.setdefault(d, set()).add(b in made)
    # on one contig: the distance decides, at equality (integer w) and between two integers (w = 350.5)
    assert seen[W - 1] == {False} and seen[W + 1] == {True}
    assert seen[W] == ({True} if float(W) >= w else {False})
    assert any(cols["tid"][a] != cols["tid"][b] and abs(int(cols["pos"][a]) - int(cols["pos"][b])) < W and b in made for a, b in by.values())
    assert np.any(pairs["x"] == pairs["y"]) and np.any(pairs["p1_tid"] == -1) and np.any(pairs["p2_tid"] == -1)
    assert np.any((pairs["p1_tid"] == -1) & (pairs["p2_tid"] == -1))
    # wrapped genome positions: an x below its own position on a contig whose offset is not 0
    nt = len(c.contigs)
    assert sum(l for _, l in c.contigs[:3]) < 2 ** 32 < sum(l for _, l in c.contigs[:4])
    assert np.any(cols["mtid"][cand] >= nt) and np.any(cols["mtid"][cand] == -1)
    tie = pairs[pairs["x"] == pairs["y"]]
    assert np.all(tie["p1_pos"] >= tie["p2_pos"])  # c1 <= c2 at equality: the record that arrives second is side 1


def test_group_cases():
    for name in ("groups_of_one_pair", "single_group", "no_pair", "no_candidate", "groups_of_all_sizes"):
        c = BY_NAME[name]
        pairs, off = jc.model(c.contigs, c.cols, jc.QUAL, c.w)
        ng = len(off) - 1
        if name == "groups_of_all_sizes":
            assert ng >= c.witness["groups"] and len(pairs) >= c.witness["pairs"]
            sizes = np.diff(off.astype(np.int64))
            assert sizes.min() == 1 and sizes.max() >= 10
        else:
            assert (ng, len(pairs)) == (c.witness["groups"], c.witness["pairs"]), name
    assert not np.any(jc.candidate_mask(BY_NAME["no_candidate"].cols)) and np.any(jc.candidate_mask(BY_NAME["no_pair"].cols))
    # numeric and string order of the groups differ: the table is not sorted by its numeric chr-pair key
    c = BY_NAME["groups_of_one_pair"]
    pairs, _ = jc.model(c.contigs, c.cols, jc.QUAL, c.w)
    key = (pairs["p1_tid"].astype(np.int64) + 1) * 14 + pairs["p2_tid"] + 1
    assert np.any(key[:-1] > key[1:]) and np.array_equal(pairs["group"], np.arange(len(pairs)))


def test_rec_bits_case_shifts():
    c = jc.rec_bits_case()
    base, off = jc.model(c.contigs, c.cols, jc.QUAL, c.w)
    assert len(base) >= 300 and len(off) - 1 >= 30  # many groups: their order is what the record bits must not move
    for rb in jc.REC_BASES[1:]:
        got, _ = jc.model(c.contigs, c.cols, jc.QUAL, c.w, rec_base=rb)
        exp = base.copy()
        exp["rec"] += np.uint64(rb)
        assert np.array_equal(got, exp)
    nt = len(c.contigs)
    gbits = 1
    while (1 << gbits) < (nt + 1) * (nt + 1):
        gbits += 1
    bits = lambda v: max(1, int(v).bit_length())
    n = len(c.cols["tid"])
    assert bits(jc.REC_BASES[2] + n) + gbits <= 64 < bits(jc.REC_BASE_LIMIT + n) + gbits

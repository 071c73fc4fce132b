"""The stream-pass cases of tests/streamcases.py without a GPU: the numpy definition against the oracle (oracle/oracle.cc), every case on
the edge it is named for at the constants of the build - what each look at the two LDS bins finds, which records sit at the edge of
a wave, an iteration, the table and its tail - and the two debug entries exported, bound, declared and documented."""
import os
import re

import numpy as np
import pytest

from breakid_amd import abi, capi
from oracle import pyoracle
from tests import streamcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")
HOOKS = ("bk_debug_stream_info", "bk_debug_stream_blocks")


def _built():
    return os.path.exists(capi.LIB_PATH)


def geo():
    """the constants of the build when there is one (so the cases stay on their edges under -DBK_STREAM_V=8), else today's"""
    if _built():
        info = capi.stream_info()
        return sc.Geo({k: info[k] for k in sc.TODAY})
    return sc.Geo()


G = geo()


def test_hooks_exported_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    item = design[design.index("Test hooks of the C ABI"):]
    item = item[:item.index("\n* ")]
    for name in HOOKS:
        assert name in capi.EXPORTS, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in item, name
        if _built():
            assert hasattr(capi.lib(), name), name
    assert callable(capi.stream_info) and callable(capi.stream_blocks)
    assert "tests/test_gpu_stream.py" in item and "tests/test_gpu_join.py" in item
    assert abi.CAND.itemsize == 40 and abi.CAND.names[:2] == ("qhash", "rec")


def test_constants_of_the_source():
    src = open(os.path.join(CSRC, "stream.hip")).read()
    hdr = open(os.path.join(CSRC, "stream.h")).read()
    assert re.search(r"#define BK_STREAM_V %d\b" % sc.TODAY["STREAM_V"], hdr)
    assert re.search(r"constexpr int ST_CAND_CAP = %d;" % sc.TODAY["ST_CAND_CAP"], src) and re.search(r"constexpr int ST_SA_CAP = %d;" % sc.TODAY["ST_SA_CAP"], src)
    assert "nc >= ST_CAND_CAP / 2 || last_iter" in src and "ns >= ST_SA_CAP / 2 || last_iter" in src and "(iter_no & 3u) == 0" in src
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert "std::max<uint64_t>(1u << 16, n_expected / 8 + 1024)" in api and "std::max<uint64_t>(1u << 14, n_expected / 16 + 1024)" in api
    if _built():
        info = capi.stream_info()
        assert info["STREAM_V"] in (4, 8) and info["RESIDENT"] >= 0
        assert capi.lib().bk_debug_stream_info(None) == abi.BK_ERR_ARG
        capi.stream_blocks(0)  # (0 is the default: nothing changes)


def against_oracle(contigs, cols):
    """the definition's candidates and insert-size sums are the oracle's: its mean is sum / n, and with w = 0 its mate join pairs every
    two neighbouring candidates of one read name (streamcases.build gives records 2j and 2j + 1 one name)"""
    e = sc.expected(cols)
    o = pyoracle.Oracle(contigs, cols)
    try:
        mean, _ = o.isize_stats()
        if e.isize_n:
            assert mean == float(e.isize_sum) / float(e.isize_n)
        else:
            assert np.isnan(mean)
        o.discordant_pairs(sc.QUAL, 0.0)
        pairs, _ = o.fetch(abi.STAGE_SCAN)
    finally:
        o.close()
    c = set(int(r) for r in e.cand["rec"])
    both = sorted(r for r in c if r % 2 == 1 and r - 1 in c)
    assert sorted(int(r) for r in pairs["rec"]) == both
    return e, len(both)


# ---- the two bins --------------------------------------------------------------------------------------------------------------------------
def looks(cols, kind, blocks=1):
    mask = sc.candidate_mask(cols) if kind == "cand" else sc.sa_mask(cols)
    return G.bin_events(G.per_iteration(mask, blocks)[0], G.CC if kind == "cand" else G.SC)


@pytest.mark.parametrize("kind", ["cand", "sa"])
@pytest.mark.parametrize("edge", range(6))
def test_window_cases_sit_on_their_edges(kind, edge):
    cap = G.CC if kind == "cand" else G.SC
    first = (sc.cand_edges(G) if kind == "cand" else sc.sa_edges(G))[edge]
    assert (first - {0: cap // 2 - 1, 1: cap // 2, 2: cap - 1, 3: cap, 4: cap + 1, 5: G.W}[edge]) == 0 and G.W > cap + 1
    p = sc.window_case(G, kind, first)
    contigs, cols = sc.build(p)
    assert G.blocks(p.n, 1) == 1 and G.iterations(p.n, 1) == 5 and p.n % G.V == G.V - 1
    ev, spilled = looks(cols, kind)
    # the look after the fourth iteration finds `first` entries (the bin's capacity at most), the last look the 3 of the second window
    assert [it for it, _, _ in ev] == [3, 4]
    assert ev[0][1] == min(first, cap) and ev[0][2] == (first >= cap // 2)
    assert ev[1] == (4, 3 if first >= cap // 2 else first + 3, True)
    assert spilled == max(0, first - cap)
    other, ospill = looks(cols, "sa" if kind == "cand" else "cand")
    assert ospill == 0 and all(nc == 0 for _, nc, _ in other)
    e, paired = against_oracle(contigs, cols)
    assert (len(e.cand) if kind == "cand" else len(e.sa)) == first + 3
    assert e.isize_n > 0 and (kind == "sa" or paired > 0 or first < 700)


def test_both_bins_cases_sit_on_their_edges():
    seen = {}
    for tag, p in sc.both_bins_cases(G):
        contigs, cols = sc.build(p)
        (c, cs), (s, ss) = looks(cols, "cand"), looks(cols, "sa")
        assert cs == 0 and ss == 0 and c[0][0] == 3 and s[0][0] == 3
        seen[tag] = (c[0][1:], s[0][1:])
        against_oracle(contigs, cols)
    assert seen == {"cand_only": ((G.CC // 2, True), (G.SC // 2 - 1, False)), "sa_only": ((G.CC // 2 - 1, False), (G.SC // 2, True)),
                    "both": ((G.CC // 2, True), (G.SC // 2, True))}


@pytest.mark.parametrize("first", ["half", "below"])
def test_order_of_flushes_cases(first):
    n1 = G.CC // 2 - (first == "below")
    contigs, cols = sc.build(sc.order_of_flushes_case(G, n1))
    ev, spilled = looks(cols, "cand")
    if first == "half":
        assert ev[0] == (3, n1, True) and spilled == 2 * G.B - G.CC
    else:
        assert ev[0] == (3, n1, False) and spilled == n1 + 2 * G.B - G.CC
    assert G.B > G.CC  # the first iteration of the second window alone overflows the bin


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", sc.GEOMETRY_CAPS)
@pytest.mark.parametrize("k", sc.GEOMETRY_K)
def test_geometry_cases(cap, k):
    for rest in sc.geometry_rests(G):
        p = sc.geometry_case(G, cap, k, rest)
        assert p.n == k * G.B * max(cap, 1) + rest
        if not cap:
            continue  # the grid is the card's: what runs is asserted on the GPU (test_gpu_stream)
        blocks = G.blocks(p.n, cap)
        assert blocks == cap
        iters = G.iterations(p.n, blocks)
        assert iters == k + (1 if rest >= G.V else 0)
        assert p.n % G.V == rest % G.V
        if rest >= G.V and cap > 1:
            live = [min(max(p.n // G.V - ((iters - 1) * cap + b) * 256, 0), 256) for b in range(cap)]
            assert live[-1] == 0 and 0 < live[0] <= 256  # idle blocks in the last round; idle lanes beside live ones unless the block is full
            if rest in (G.V, G.B - 1):
                assert live[0] < 256
    contigs, cols = sc.build(sc.geometry_case(G, cap, k, G.B + 1))
    against_oracle(contigs, cols)
    if cap and k >= 4:
        spills = [G.bin_events(row, G.CC)[1] for row in G.per_iteration(sc.candidate_mask(cols), cap)]
        assert all(s > 0 for s in spills)  # four iterations of ~30 % candidates overflow every block's bin


def test_tail_only_sizes():
    assert sc.tail_only_sizes(G) == [1, G.V - 1]
    for n in sc.tail_only_sizes(G):
        assert n // G.V == 0 and G.blocks(n, 0) == 1 and G.iterations(n, 1) == 0


# ---- neighbours and order --------------------------------------------------------------------------------------------------------------------
def test_places():
    n = sc.places_n(G)
    pl = sc.places(G, n)
    nq = n // G.V
    assert len(set(pl.values())) == len(pl) == 9
    lane = lambda i: (i // G.V) % 64
    assert pl["inside_a_group"] % G.V != 0 and pl["between_groups_of_a_wave"] % G.V == 0 and lane(pl["between_groups_of_a_wave"]) not in (0, 63)
    assert lane(pl["last_lane_of_a_wave"]) == 63 and pl["last_lane_of_a_wave"] % G.V == G.V - 1
    assert lane(pl["lane_0_of_a_wave"]) == 0 and pl["lane_0_of_a_wave"] % G.V == 0 and 0 < pl["lane_0_of_a_wave"] < G.B
    assert pl["iteration_boundary"] == G.B and G.iterations(n, 1) == 2
    assert pl["first_of_last_group"] == (nq - 1) * G.V and pl["last_of_last_group"] == nq * G.V - 1 and lane(pl["last_of_last_group"]) != 63
    assert pl["first_tail_record"] == nq * G.V and pl["last_record"] == n - 1 > pl["first_tail_record"]


@pytest.mark.parametrize("place", sorted(sc.places(sc.Geo(), sc.places_n(sc.Geo()))))
def test_neighbour_cases(place):
    p, at = sc.neighbour_case(G, place)
    contigs, cols = sc.build(p)
    sp = sc.spans(cols)
    assert sp[at] == sc.LONG_SPAN and np.sum(sp == sc.LONG_SPAN) == 1 and np.max(np.delete(sp, at)) == 100
    e, _ = against_oracle(contigs, cols)
    assert e.max_span == sc.LONG_SPAN and list(e.cand["rec"]) == [at] and at in e.sa and len(e.sa) > 20
    co, ao = cols["cigar_off"].astype(np.int64), cols["aux_off"].astype(np.int64)
    assert co[at + 1] - co[at] == 4 and ao[at + 1] > ao[at]
    for k in (at - 1, at + 1):  # the offsets change exactly at the place
        if 0 <= k < p.n:
            assert co[k + 1] - co[k] == 1 and ao[k + 1] == ao[k]


@pytest.mark.parametrize("by", ["pos", "tid"])
@pytest.mark.parametrize("place", sorted(sc.places(sc.Geo(), sc.places_n(sc.Geo()))))
def test_unsorted_cases(place, by):
    p, at = sc.unsorted_case(G, place, by)
    _, cols = sc.build(p)
    assert list(sc.inversions(cols)) == [at]


def test_equal_neighbours_case():
    p = sc.equal_neighbours_case(G)
    contigs, cols = sc.build(p)
    assert len(sc.inversions(cols)) == 0
    for at in sc.places(G, p.n).values():
        assert cols["pos"][at] == cols["pos"][at - 1] and cols["tid"][at] == cols["tid"][at - 1]
    against_oracle(contigs, cols)


# ---- capacity, flags -------------------------------------------------------------------------------------------------------------------------
def test_capacity_cases():
    a, b = sc.capacity_cases()
    ca, cb = sc.build(a)[1], sc.build(b)[1]
    ea, eb = sc.expected(ca), sc.expected(cb)
    assert (a.n, len(ea.cand)) == (80_000, 70_000) and len(ea.cand) > sc.first_capacity(a.n)[0] and len(ea.sa) <= sc.first_capacity(a.n)[1]
    assert (b.n, len(eb.sa)) == (40_000, 20_000) and len(eb.sa) > sc.first_capacity(b.n)[1] and len(eb.cand) <= sc.first_capacity(b.n)[0]
    against_oracle(sc.CONTIGS, cb)


def test_flag_gate_case():
    p = sc.flag_gate_case()
    contigs, cols = sc.build(p)
    assert p.n == 128 and len(set(zip(cols["flag"].tolist(), cols["mapq"].tolist()))) == 128
    e = sc.expected(cols)
    # PAIRED, !PROPER, !SECONDARY, !DUP, any of UNMAP / QCFAIL, mapq = q: 4 candidates; PAIRED, !DUP: 32 SA-bearing; PAIRED, PROPER, none
    # of the four: 2 insert sizes
    assert (len(e.cand), len(e.sa), e.isize_n) == (4, 32, 2)
    assert np.all(e.cand["mapq"] == sc.QUAL)
    # every record twice, so that the oracle's mate join pairs exactly the candidates (its predicate, not the definition's)
    twice = sc.take(cols, np.repeat(np.arange(p.n), 2))
    twice["qhash"] = (np.arange(2 * p.n, dtype=np.uint64) // np.uint64(2) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    twice["qcheck"] = (np.arange(2 * p.n) // 2 + 1).astype(np.uint32)
    e2, paired = against_oracle(contigs, twice)
    assert paired == len(e.cand) and e2.isize_n == 2 * e.isize_n

"""CPU: the host side of `bk_clip_reads`: the numpy mirrors of its two structs, and the numpy definition the GPU tests check against
(tests/clipreadcases.py) itself - against the designed truth of clipcases.clip_tumor(), where the reads clipped at every breakpoint
are known by name, and against the two identities that tie the call to bk_clip_support, with the clusters of the CPU oracle."""
import numpy as np
import pytest

from breakid_amd import abi, capi
from oracle import pyoracle
from tests import clipcases as kc
from tests import clipreadcases as rc
from tests.callcases import QUAL
from tests.clipcases import LEFT, RIGHT

DIR = {"L": LEFT, "R": RIGHT}


def test_clip_reads_struct_layout():
    assert abi.CLIP_SITE.itemsize == 16 and abi.CLIP_READ.itemsize == 40
    assert [abi.CLIP_SITE.fields[f][1] for f in ("tid", "pos", "tol", "dir")] == [0, 4, 8, 12]
    assert [abi.CLIP_READ.fields[f][1] for f in ("rec", "qhash", "qcheck", "site", "tid", "p", "clip_len", "flag", "mapq", "dir")] == [0, 8, 16, 20, 24, 28, 32, 36, 38, 39]
    assert "bk_clip_reads" in capi.EXPORTS and callable(capi.Context.clip_reads)


@pytest.fixture(scope="module")
def designed():
    ds = kc.clip_tumor()
    return ds, ds.to_soa()


def test_designed_breakpoints_list_the_designed_reads(designed):
    ds, cols = designed
    sites, want = [], []
    for name, ta, bpa, da, tb, bpb, db in kc.CLIP_LOCI:
        if name not in ("b", "d", "e", "f"):
            continue
        na, nb, along = kc.CLIP_READS[name]
        for tag, t, bp, d, n in (("a", ta, bpa, DIR[da], na), ("b", tb, bpb, DIR[db], nb)):
            clipped = d if along else 1 - d  # locus e: its clipped reads point against its pairs
            sites.append((t, bp, 0, clipped))
            want.append({"%sC%s_%d" % (name, tag, j) for j in range(n)})
            sites.append((t, bp, 0, 1 - clipped))
            want.append(set())
    counts, rows, off = rc.expected_clip_reads(cols, rc.as_sites(sites), QUAL, 10)
    assert len(off) == len(sites) + 1 and int(off[-1]) == len(rows) == int(counts.sum()) == 6 + 6 + 6 + 0 + 6 + 6 + 2 + 2
    for k, names in enumerate(want):
        mine = rows[int(off[k]):int(off[k + 1])]
        assert int(counts[k]) == len(mine) == len(names), (sites[k], mine)
        assert {ds.recs[int(r["rec"])].qname for r in mine} == names, sites[k]
        assert np.all(mine["site"] == k) and np.all(mine["p"] == sites[k][1]) and np.all(mine["tid"] == sites[k][0]) and np.all(mine["dir"] == sites[k][3])
        assert np.all(mine["clip_len"] == 40) and np.all(mine["mapq"] == 60) and np.all(mine["flag"] & 0x40)  # clipcases.clipped_read
        assert np.all(np.diff(mine["rec"].astype(np.int64)) > 0)
        assert np.array_equal(mine["qhash"], cols["qhash"][mine["rec"]]) and np.array_equal(mine["qcheck"], cols["qcheck"][mine["rec"]])


def test_definition_details_by_hand(designed):
    """tolerance, overlap and the sites that count nothing, on locus b's side A (chr1:600000, six reads 60M40S ending there)"""
    _, cols = designed
    S = rc.as_sites([(0, 600_002, 2, LEFT), (0, 600_003, 2, LEFT), (0, 599_998, 2, LEFT), (0, 599_997, 2, LEFT), (-1, 600_000, 0, LEFT), (0, 600_000, 0, LEFT),
                     (0, 600_000, 0, LEFT), (4, 600_000, 0, LEFT), (0, 600_000, 2 ** 32 - 1, LEFT), (0, 2 ** 32 - 1, 2 ** 32 - 1, LEFT)])
    counts, rows, off = rc.expected_clip_reads(cols, S, QUAL, 10)
    assert counts[:8].tolist() == [6, 0, 6, 0, 0, 6, 6, 0]
    assert np.array_equal(rows[int(off[5]):int(off[6])]["rec"], rows[int(off[6]):int(off[7])]["rec"])  # equal sites: listed under both
    tid, p, d = kc.clip_events(cols, QUAL, 10)
    assert int(counts[8]) == int(counts[9]) == int(((tid == 0) & (d == LEFT)).sum())  # the whole contig: signed 64-bit bounds
    assert rc.expected_clip_reads(cols, S[:1], QUAL, 41)[0].tolist() == [0] and rc.expected_clip_reads(cols, S[:1], 61, 10)[0].tolist() == [0]
    c0, r0, o0 = rc.expected_clip_reads(cols, S[:0], QUAL, 10)
    assert len(c0) == 0 and len(r0) == 0 and o0.tolist() == [0]


@pytest.mark.parametrize("name", ["designed", "clipped"])
def test_identities_with_clip_support(name, designed):
    ds, cols = designed if name == "designed" else (lambda d: (d, d.to_soa()))(kc.clipped_tumor())
    o = pyoracle.Oracle(ds.contigs, cols)
    w, rcode = o.run(QUAL, fast=True)
    assert rcode == 0
    cl, _ = o.fetch(abi.STAGE_CLUSTERS)
    o.close()
    voted = (cl["flags"] & 2) != 0
    assert voted.any() and (~voted).any()
    for mapq_min, min_clip in ((QUAL, 10), (0, 1)):
        sup = kc.expected_clip_support(cl, cols, mapq_min, min_clip, w)
        sites, want = rc.identity_sites(cl, sup)
        counts, rows, off = rc.expected_clip_reads(cols, sites, mapq_min, min_clip)
        assert len(sites) == 4 * len(cl) + 4 * int(voted.sum())
        assert np.array_equal(counts, want), np.nonzero(counts != want)[0][:5]
        assert want.any() and np.array_equal(np.diff(off.astype(np.int64)), counts.astype(np.int64))

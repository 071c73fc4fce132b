"""Shared cases of the clip-read tests (test_gpu_clip_reads, test_cpu_clip_reads): the numpy definition of bk_clip_reads
(include/breakid_hip.h) over a record table, built on the events of clipcases.clip_events, and the sites the two identities with
bk_clip_support are checked at."""
import numpy as np

from breakid_amd import abi
from tests import clipcases as kc
from tests.clipcases import LEFT, RIGHT, NEVER, OP_S, OP_H


def clip_events_full(cols, mapq_min, min_clip):
    """clipcases.clip_events with, per event, the record it comes from and the length of the S op that made it:
    (tid, p, dir, rec, clip_len), in the order of clip_events (its first three results are checked to be those)"""
    n = len(cols["tid"])
    off = cols["cigar_off"].astype(np.int64)
    cig = cols["cigar"][:off[-1]].astype(np.int64)
    op, ln = cig & 15, cig >> 4
    aux_off = cols["aux_off"].astype(np.int64)
    flag = cols["flag"].astype(np.int64)
    pos = cols["pos"].astype(np.int64)
    consumed = np.concatenate([[0], np.cumsum(np.where(np.isin(op, [0, 2, 3, 7, 8]), ln, 0))])
    reflen = consumed[off[1:]] - consumed[off[:-1]]
    elig = (cols["tid"] >= 0) & ((flag & NEVER) == 0) & (cols["mapq"].astype(np.int64) >= mapq_min) & (aux_off[1:] == aux_off[:-1]) & (reflen > 0)
    not_h = np.nonzero(op != OP_H)[0]
    c0, c1 = off[:-1], off[1:]
    z = np.zeros(0, np.int64)
    if len(not_h) == 0 or len(cig) == 0:
        out = (z.astype(np.int32), z, z, z, z)
    else:
        a = np.searchsorted(not_h, c0, "left")
        b = np.searchsorted(not_h, c1, "left") - 1
        first = not_h[np.minimum(a, len(not_h) - 1)]
        last = not_h[np.maximum(b, 0)]
        has = (a < len(not_h)) & (first < c1) & (b >= 0) & (last >= c0)
        first, last = np.where(has, first, 0), np.where(has, last, 0)
        lead = elig & has & (op[first] == OP_S) & (ln[first] >= min_clip)
        trail = elig & has & (op[last] == OP_S) & (ln[last] >= min_clip)
        idx = np.arange(n, dtype=np.int64)
        out = (np.concatenate([cols["tid"][lead], cols["tid"][trail]]).astype(np.int32),
               np.concatenate([pos[lead] + 1, (pos + reflen)[trail]]),
               np.concatenate([np.full(int(lead.sum()), RIGHT, np.int64), np.full(int(trail.sum()), LEFT, np.int64)]),
               np.concatenate([idx[lead], idx[trail]]),
               np.concatenate([ln[first][lead], ln[last][trail]]))
    ref = kc.clip_events(cols, mapq_min, min_clip)
    assert all(np.array_equal(x, y) for x, y in zip(out[:3], ref))
    return out


def as_sites(sites):
    """abi.CLIP_SITE rows from (tid, pos, tol, dir) tuples"""
    out = np.zeros(len(sites), abi.CLIP_SITE)
    for k, s in enumerate(sites):
        out[k] = tuple(s)
    return out


def expected_clip_reads(cols, sites, mapq_min, min_clip):
    """(counts, rows, site_off) of bk_clip_reads: membership compared in Python integers, rows by site and then by record"""
    sites = np.ascontiguousarray(sites, abi.CLIP_SITE)
    tid, p, d, rec, clen = clip_events_full(cols, mapq_min, min_clip)
    counts = np.zeros(len(sites), np.uint32)
    site_off = np.zeros(len(sites) + 1, np.uint64)
    parts = []
    for k, s in enumerate(sites):
        lo, hi = int(s["pos"]) - int(s["tol"]), int(s["pos"]) + int(s["tol"])
        m = np.zeros(len(tid), bool) if s["tid"] < 0 else (tid == s["tid"]) & (d == int(s["dir"])) & (p >= lo) & (p <= hi)
        sel = np.nonzero(m)[0]
        sel = sel[np.argsort(rec[sel], kind="stable")]
        assert len(np.unique(rec[sel])) == len(sel)  # one event per record and direction
        rows = np.zeros(len(sel), abi.CLIP_READ)
        rows["rec"] = rec[sel]
        rows["qhash"] = cols["qhash"][rec[sel]]
        rows["qcheck"] = cols["qcheck"][rec[sel]] if "qcheck" in cols else 0
        rows["site"] = k
        rows["tid"] = tid[sel]
        rows["p"] = p[sel]
        rows["clip_len"] = clen[sel]
        rows["flag"] = cols["flag"][rec[sel]]
        rows["mapq"] = cols["mapq"][rec[sel]]
        rows["dir"] = d[sel]
        parts.append(rows)
        counts[k] = len(sel)
        site_off[k + 1] = site_off[k] + np.uint64(len(sel))
    rows = np.concatenate(parts) if parts else np.zeros(0, abi.CLIP_READ)
    return counts, rows, site_off


def identity_sites(cl, sup):
    """The sites of the two identities for every row of `cl` with its abi.CLIP_SUPPORT row: (sites, what each must count).  Every
    (row, side, dir) peak with tol 0 -> peak_n (a side without a contig, or without an event - peak_pos 0 - counts 0 = peak_n), and
    every voted (row, side, dir) at ps_exact with tol 2 -> at."""
    sites, want = [], []
    for c, s in zip(cl, sup):
        for side in (0, 1):
            T = int(c["p%d_tid" % (side + 1)])
            for dr in (LEFT, RIGHT):
                sites.append((T, int(s["peak_pos"][side][dr]), 0, dr))
                want.append(int(s["peak_n"][side][dr]))
                if c["flags"] & 2:
                    sites.append((T, int(c["p%d_exact" % (side + 1)]) & 0xFFFFFFFF, 2, dr))
                    want.append(int(s["at"][side][dr]))
    return as_sites(sites), np.asarray(want, np.uint32)


def assert_clip_reads_equal(got, exp):
    """byte for byte, every site"""
    (gc, gr, go), (ec, er, eo) = got, exp
    assert gc.dtype == np.uint32 and gr.dtype == abi.CLIP_READ and go.dtype == np.uint64
    assert np.array_equal(gc, ec), np.nonzero(gc != ec)[0][:5]
    assert np.array_equal(go, eo)
    assert len(gr) == len(er)
    bad = np.nonzero(gr != er)[0]
    assert len(bad) == 0, [(gr[i], er[i]) for i in bad[:3]]
    assert gr.tobytes() == er.tobytes()

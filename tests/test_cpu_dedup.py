"""Unique support without a GPU: the row layout and the export, the numpy definition (tests/dedupcases.py) against the designed truth
of its datasets over the CPU oracle's stage tables, its invariants, the mirrored tile constants, and the CPU build's refusal of -dedup."""
import os
import re
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from oracle import pyoracle
from tests import callcases as cc
from tests import dedupcases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
CSRC = os.path.join(ROOT, "breakid_amd", "csrc")


def test_unique_support_row_layout_and_export():
    assert abi.UNIQUE_SUPPORT.itemsize == 16
    assert {f: abi.UNIQUE_SUPPORT.fields[f][1] for f in abi.UNIQUE_SUPPORT.names} == {"uniq_pairs": 0, "top_pairs": 4, "uniq_splits": 8, "top_splits": 12}
    assert all(abi.UNIQUE_SUPPORT.fields[f][0] == np.dtype("<u4") for f in abi.UNIQUE_SUPPORT.names)
    assert "bk_unique_support" in capi.EXPORTS and hasattr(capi.Context, "unique_support")
    assert hasattr(capi.lib(), "bk_unique_support")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_unique_support { uint32_t uniq_pairs, top_pairs, uniq_splits, top_splits; };" in header
    assert "typedef struct bk_unique_support" not in header


def test_tile_constants_are_the_kernels():
    m = re.search(r"constexpr int UNIQUE_TILE = (\d+);", open(os.path.join(CSRC, "unique.h")).read())
    assert m and int(m.group(1)) == dc.UNIQUE_TILE
    m = re.search(r"constexpr int RS_ROWS = (\d+);", open(os.path.join(CSRC, "prims.h")).read())
    assert m and 256 * int(m.group(1)) == dc.RADIX_TILE
    assert dc.DEEP_COPIES > dc.RADIX_TILE + dc.UNIQUE_TILE


def oracle_tables(ds, cols, fast):
    o = pyoracle.Oracle(ds.contigs, {k: v for k, v in cols.items() if k != "target_len"})
    o.run(cc.QUAL, fast=fast)
    cl, clustered, splits = (o.fetch(st)[0] for st in (abi.STAGE_CLUSTERS, abi.STAGE_CLUSTERED, abi.STAGE_SPLITS))
    o.close()
    return cl, clustered, splits


@pytest.mark.parametrize("fast", [True, False])
def test_definition_on_the_designed_duplicates(fast):
    ds, cols = dc.dedup_tumor()
    names = [r.qname for r in ds.recs]
    cl, clustered, splits = oracle_tables(ds, cols, fast)
    rows, first = dc.expected_unique_support(cl, clustered, splits, cols)
    ev, off, keys = dc.fragment_keys(cl, clustered, splits, cols)
    dc.check_invariants(ev, off, rows, first)
    for name, ta, bpa, da, tb, bpb, db in cc.LOCI:
        at = cc.rows_of(cl, ta, bpa, tb, bpb)
        assert len(at) == 1, name  # voted at the designed breakpoints
        c = at[0][0]
        a, b = int(off[c]), int(off[c + 1])
        sr = np.flatnonzero(ev["kind"][a:b] == abi.EV_SPLIT) + a
        pe = np.flatnonzero(ev["kind"][a:b] == abi.EV_PAIR) + a
        assert (len(sr), int(rows[c]["uniq_splits"]), int(rows[c]["top_splits"])) == (16, 5, 6), (name, rows[c])
        # a fragment of split rows is the copies of one designed read: same m1, whatever the copy number
        for r in sr:
            assert names[int(ev["rec"][r])].rsplit("_", 1)[0] == names[int(ev["rec"][int(first[r])])].rsplit("_", 1)[0]
        assert len({names[int(ev["rec"][r])].rsplit("_", 1)[0] for r in sr}) == 5
        # ... and a fragment of pair rows the copies of one designed pair; the rows are what isolation and clustering kept
        stems = [names[int(ev["rec"][r])].rsplit("_", 1)[0] for r in pe]
        assert len(pe) == int(cl[c]["n_drp"]) == (10 if fast else 12) and int(rows[c]["uniq_pairs"]) == len(set(stems))
        assert 5 <= int(rows[c]["uniq_pairs"]) <= 7 and (fast or int(rows[c]["uniq_pairs"]) == 7), (name, rows[c])
        for r in pe:
            assert stems[r - a] == names[int(ev["rec"][int(first[r])])].rsplit("_", 1)[0]


@pytest.mark.parametrize("fast", [True, False])
def test_near_key_dataset_covers_its_fields(fast):
    ds, cols = dc.near_key_tumor()
    cl, clustered, splits = oracle_tables(ds, cols, fast)
    assert len(cl) == 1 and cl[0]["flags"] & 2
    covered = dc.fields_differing_alone(cl, clustered, splits, cols)
    assert dc.NEAR_REQUIRED <= covered and "p1_pos" in covered, covered
    rows, first = dc.expected_unique_support(cl, clustered, splits, cols)
    dc.check_invariants(*dc.fragment_keys(cl, clustered, splits, cols)[:2], rows, first)
    # five split reads designed twice each (two tuples a read): base, another mate, a longer far end, m1 = 50 and 70 once each
    assert (int(rows[0]["uniq_splits"]), int(rows[0]["top_splits"])) == (5, 4)


def test_deep_call_straddles_the_tiles():
    ds, cols = dc.deep_tumor()
    cl, clustered, splits = oracle_tables(ds, cols, True)
    rows, first = dc.expected_unique_support(cl, clustered, splits, cols)
    dc.check_invariants(*dc.fragment_keys(cl, clustered, splits, cols)[:2], rows, first)
    dc.deep_rows_expected(rows)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_dedup(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-dedup"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -dedup needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-dedup", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -dedup needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-dedup", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-dedup cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-dedup" in r.stderr

"""Junction consensus without a GPU: the row layout and the exports, the Python definition (tests/consensuscases.py) against the
designed truth of its BAM and its invariants, bk_bam_reads against bamio.read_records of the same file in both block layouts, and
the CPU build's refusal of -consensus."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi
from tests import consensuscases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_consensus_row_layout_and_exports():
    assert abi.CONSENSUS.itemsize == 16
    assert {f: abi.CONSENSUS.fields[f][1] for f in abi.CONSENSUS.names} == {"n_reads": 0, "len": 4, "match": 8, "total": 12}
    assert all(abi.CONSENSUS.fields[f][0] == np.dtype("<u4") for f in abi.CONSENSUS.names)
    assert [n for n, _ in abi.READS_COLS] == ["tid", "pos", "flag", "mapq", "key", "cigar_off", "cigar", "l_seq", "seq_off", "seq"]
    assert capi.C.sizeof(abi.Reads) == 8 * 12
    for name in ("bk_clip_consensus", "bk_bam_reads", "bk_reads_free"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    assert hasattr(capi.Context, "clip_consensus") and hasattr(capi, "bam_reads")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_consensus { uint32_t n_reads, len, match, total; };" in header
    assert "typedef struct bk_consensus" not in header and "typedef struct bk_reads {" in header


@pytest.fixture(scope="module")
def designed_bams(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cons")
    paths = {}
    for aligned in (True, False):
        paths[aligned] = str(tmp / ("a%d.bam" % aligned))
        kc.write_designed_bam(paths[aligned], aligned=aligned)
    return paths


@pytest.fixture(scope="module")
def designed_table(designed_bams):
    return kc.reads_of_bam(designed_bams[True])


def test_definition_on_the_designed_truth(designed_table):
    reads, names = designed_table
    d = kc.designed()
    sites = d["sites"]
    rows, bases, depth = kc.expected_consensus(reads, sites, 20, kc.MIN_CLIP, kc.MAX_LEN, kc.MIN_DEPTH)
    kc.check_invariants(rows, bases, depth, kc.MAX_LEN)
    by = {(int(s["tid"]), int(s["pos"]), int(s["dir"])): k for k, s in enumerate(sites)}
    assert len(d["truth"]) == 18  # both sides of the eight loci and of the mixed one
    for key, text in d["truth"].items():
        k = by[key]
        assert bytes(bases[k, :int(rows[k]["len"])]).decode() == text, (key, rows[k])
        assert len(text) in (40, 60) and rows[k]["n_reads"] >= 8
    # the designed variations, by their numbers
    (_, ta, bpa, _, tb, bpb, _) = kc.cc.LOCI[0]
    a0, b0 = by[(ta, bpa, kc.LEFT)], by[(tb, bpb, kc.RIGHT)]
    assert int(rows[a0]["n_reads"]) == 11 and list(depth[a0, [0, 11, 12, 24, 25, 39, 40]]) == [11, 11, 10, 10, 9, 9, 0]  # clips 40, 25, 12; 9 is short
    assert int(rows[a0]["total"]) - int(rows[a0]["match"]) == 1  # the minority base
    assert int(rows[b0]["n_reads"]) == 10 and int(rows[b0]["len"]) == 60 and list(depth[b0, [39, 40, 59, 60, 63]]) == [10, 9, 9, 1, 1]
    (_, ta, bpa, _, tb, bpb, _) = kc.cc.LOCI[1]
    a1, b1 = by[(ta, bpa, kc.LEFT)], by[(tb, bpb, kc.LEFT)]
    assert int(rows[a1]["total"]) - int(rows[a1]["match"]) == 8  # two columns tied 4 : 4
    assert int(depth[b1, 3]) == 8 and int(rows[b1]["total"]) - int(rows[b1]["match"]) == 2  # N and R count in the depth only
    (_, ta, bpa, _, tb, bpb, _) = kc.cc.LOCI[2]
    a2, b2 = by[(ta, bpa, kc.RIGHT)], by[(tb, bpb, kc.RIGHT)]
    assert int(rows[a2]["n_reads"]) == 8 and rows[a2]["match"] == rows[a2]["total"]  # none of the five reads that must not count
    two = by[kc.TWO_CLIP_SITE[:2] + (kc.LEFT,)]
    assert int(rows[b2]["n_reads"]) == 9 and int(rows[two]["n_reads"]) == 1 and int(rows[two]["len"]) == 0 and int(depth[two, 29]) == 1
    (_, ta, bpa, _, tb, bpb, _) = kc.cc.LOCI[3]
    b3 = by[(tb, bpb, kc.LEFT)]
    assert int(rows[b3]["n_reads"]) == 10 and rows[b3]["match"] == rows[b3]["total"]  # both nibble parities read the right bases
    # min_depth 1 keeps the columns one read reaches
    r1, b1_, _ = kc.expected_consensus(reads, sites, 20, kc.MIN_CLIP, kc.MAX_LEN, 1)
    assert int(r1[b0]["len"]) == 64 and int(r1[two]["len"]) == 30


def test_definition_on_the_crowd_table():
    reads, sites = kc.crowd_table()
    rows, bases, depth = kc.expected_consensus(reads, sites, 20, 10, 100, 2)
    kc.check_invariants(rows, bases, depth, 100)
    assert list(rows["n_reads"]) == [300, 0, 0, 300, 50, 0] and int(rows[0]["len"]) == 90 and rows[0].tobytes() == rows[3].tobytes()
    assert 0 < int(rows[0]["match"]) < int(rows[0]["total"]) == 300 * 90 and 20 <= int(rows[4]["len"]) <= 90
    perm = np.random.default_rng(1).permutation(len(reads["tid"]))
    again = kc.expected_consensus(kc.permuted(reads, perm), sites, 20, 10, 100, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (rows, bases, depth)))


def assert_tables_equal(got, exp):
    for name, dt in abi.READS_COLS:
        assert got[name].dtype == np.dtype(dt) and np.array_equal(got[name], np.asarray(exp[name], dt)), name


@pytest.mark.parametrize("aligned", [True, False])
def test_bam_reads_equals_the_records_of_the_file(designed_bams, aligned):
    reads, names = kc.reads_of_bam(designed_bams[aligned])
    assert (reads["l_seq"] == 0).sum() == 1 and (reads["l_seq"] == 99).sum() == 1 and (reads["l_seq"] == 90).sum() == 1
    picked = [b"LR_xS_0", b"xNoseq", b"xOddLen", b"xShort", b"xBoth", b"MIXS_3", b"p17", b"RR_sD_2"]
    keys = np.concatenate([kc.keys_of(picked), kc.keys_of([b"no_such_read"]), kc.keys_of([b"p17", b"p18"], qcheck=False)])
    got = capi.bam_reads(designed_bams[aligned], keys)
    exp = kc.selected(reads, names, keys)
    assert_tables_equal(got, exp)
    # three alignments of a split read, two of every other name; p17 under its first key, p18 under the hash-only one
    assert len(got["tid"]) == 3 * 2 + 2 * 7 and set(got["key"].tolist()) == set(range(8)) | {10}
    assert (got["l_seq"] == 0).sum() == 1 and (np.diff(got["seq_off"].astype(np.int64)) == (got["l_seq"].astype(np.int64) + 1) // 2).all()
    # the whole file through a hash-only key per name
    every = capi.bam_reads(designed_bams[aligned], kc.keys_of(sorted(set(names)), qcheck=False))
    assert len(every["tid"]) == len(names)
    for name, dt in abi.READS_COLS:
        if name != "key":
            assert np.array_equal(every[name], np.asarray(reads[name], dt)), name


def test_bam_reads_empty_duplicate_and_truncated(designed_bams, tmp_path):
    path = designed_bams[True]
    got = capi.bam_reads(path, np.zeros(0, abi.READ_KEY))
    assert len(got["tid"]) == 0 and list(got["cigar_off"]) == [0] and list(got["seq_off"]) == [0] and len(got["seq"]) == 0
    got = capi.bam_reads(path, kc.keys_of([b"no_such_read"]))
    assert len(got["tid"]) == 0
    with pytest.raises(capi.BreakIDError, match="bk_bam_reads: duplicate key 2") as e:
        capi.bam_reads(path, kc.keys_of([b"p17", b"p18", b"p17"]))
    assert e.value.code == abi.BK_ERR_ARG
    raw = open(path, "rb").read()
    cut = tmp_path / "cut.bam"
    cut.write_bytes(raw[:len(raw) // 2])
    with pytest.raises(capi.BreakIDError) as e:
        capi.bam_reads(str(cut), kc.keys_of([b"p17"]))
    assert e.value.code == abi.BK_ERR_IO
    with pytest.raises(capi.BreakIDError) as e:
        capi.bam_reads(str(tmp_path / "absent.bam"), kc.keys_of([b"p17"]))
    assert e.value.code == abi.BK_ERR_IO
    C = capi.C
    err = C.create_string_buffer(64)
    assert capi.lib().bk_bam_reads(os.fsencode(path), None, 0, None, err, 64) == abi.BK_ERR_ARG and b"null output" in err.value
    t = abi.Reads()
    assert capi.lib().bk_bam_reads(os.fsencode(path), None, 1, C.byref(t), err, 64) == abi.BK_ERR_ARG and t.n == 0 and not t.owner
    capi.lib().bk_reads_free(C.byref(t))  # a table that was not filled needs no free, and takes one


def test_bam_extract_is_unchanged_by_the_shared_walk(designed_bams, tmp_path):
    """the pass bk_bam_reads shares with bk_bam_extract still writes the records it selects, tagged, and gives the names back"""
    keys = np.concatenate([kc.keys_of([b"xBoth", b"LR_xS_0"]), kc.keys_of([b"no_such_read"])])
    out = str(tmp_path / "x.bam")
    names, n = capi.bam_extract(designed_bams[False], out, keys, ["t0"])
    assert names == ["xBoth", "LR_xS_0", ""] and n == 5
    _, src = bamio.read_records(designed_bams[False])
    _, got = bamio.read_records(out)
    want = [r + b"bkZt0\0" for r in src if r[32:32 + r[8]].split(b"\0")[0] in (b"xBoth", b"LR_xS_0")]
    assert got == want
    with pytest.raises(capi.BreakIDError, match="bk_bam_extract: duplicate key 1"):
        capi.bam_extract(designed_bams[False], None, kc.keys_of([b"a", b"a"]), ["t0"])


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_consensus(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-consensus"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -consensus needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-consensus", "-conslen", "100", "-all", "-fast", "-minclip", "12"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -consensus needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-consensus", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-consensus cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-conslen", "100"], capture_output=True, text=True)
    assert r.returncode == 1 and "-conslen needs -consensus" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-minclip", "12"], capture_output=True, text=True)
    assert r.returncode == 1 and "-minclip and -clipsupport need -clip" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-consensus" in r.stderr and "-conslen" in r.stderr

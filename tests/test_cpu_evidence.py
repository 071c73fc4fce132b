"""CPU: the host side of the evidence export (`-evidence`, `bk_evidence`, `bk_bam_extract`): the numpy mirror of the row, the
extractor (one streaming pass, hashes back to names, a BGZF writer with htslib's layout) on files whose records stay inside
their blocks and on files whose records cross them, its failure cases, and the command line built over the CPU oracle
(oracle/cpu_shim.cc), which has no `bk_evidence` and must refuse `-evidence` cleanly."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")
CONTIGS = [("chr1", 5_000_000), ("chr2", 4_000_000), ("chrUn_x", 90_000)]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
NEW = ("bk_evidence", "bk_bam_extract", "bk_bam_names_free")


def test_evidence_row_layout():
    assert abi.EVIDENCE.itemsize == 48 and abi.READ_KEY.itemsize == 16
    off = {f: abi.EVIDENCE.fields[f][1] for f in abi.EVIDENCE.names}
    assert off == {"rec": 0, "qhash": 8, "qcheck": 16, "call": 20, "tid1": 24, "pos1": 28, "tid2": 32, "pos2": 36, "flag1": 40, "flag2": 42,
                   "mapq1": 44, "mapq2": 45, "kind": 46, "sides": 47}
    assert abi.EVIDENCE.fields["tid1"][0] == np.dtype("<i4") and abi.EVIDENCE.fields["pos1"][0] == np.dtype("<u4")
    assert abi.EVIDENCE.fields["rec"][0] == np.dtype("<u8") and abi.EVIDENCE.fields["flag2"][0] == np.dtype("<u2")
    assert {f: abi.READ_KEY.fields[f][1] for f in abi.READ_KEY.names} == {"qhash": 0, "qcheck": 8, "tag": 12}
    assert (abi.EV_PAIR, abi.EV_SPLIT) == (1, 2)
    for name in NEW:
        assert name in capi.EXPORTS
    assert hasattr(capi.Context, "evidence") and hasattr(capi, "bam_extract")


def test_exports_are_in_the_library():
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name)


# ---- a table with known names ---------------------------------------------------------------------------------------------
N_REC, N_NAMES, LONG_AT = 6000, 2300, 1234  # ~75 bytes a record: the stream crosses several 0xff00-byte blocks


def qhash(name):
    return capi.lib().bk_qname_hash(name, len(name))


def qcheck(name):
    return capi.lib().bk_qname_check(name, len(name))


def make_table():
    rng = np.random.default_rng(7)
    tid = np.sort(rng.integers(0, 2, N_REC)).astype(np.int32)
    pos = rng.integers(0, 3_000_000, N_REC).astype(np.int32)
    order = np.lexsort((pos, tid))
    tid, pos = tid[order], pos[order]
    names = [b"read%05d/x" % int(k) for k in rng.integers(0, N_NAMES, N_REC)]
    flag = rng.choice(np.array([99, 147, 83, 163, 97, 145, 2147, 2195, 355, 1123], np.uint16), N_REC)
    mapq = rng.choice(np.array([0, 3, 20, 60], np.uint8), N_REC)
    cig_rows, aux_rows = [], []
    for i in range(N_REC):
        if i == LONG_AT:  # a record longer than a BGZF block: 20000 CIGAR words
            cig_rows.append([(1 << 4) | 0, (1 << 4) | 1] * 10000)
        elif i % 5 == 0:
            cig_rows.append([(60 << 4) | 0, (40 << 4) | 4])
        else:
            cig_rows.append([(100 << 4) | 0])
        aux_rows.append(b"chr2,%d,+,40S60M,60,0;" % (1000 + i) if i % 5 == 0 else b"")
    cols = {"tid": tid, "pos": pos, "mtid": tid.copy(), "mpos": (pos + 300).astype(np.int32), "isize": np.full(N_REC, 400, np.int32), "flag": flag, "mapq": mapq,
            "qhash": np.array([qhash(n) for n in names], np.uint64), "qcheck": np.array([qcheck(n) for n in names], np.uint32),
            "cigar_off": np.concatenate([[0], np.cumsum([len(c) for c in cig_rows])]).astype(np.uint32),
            "cigar": np.array([w for c in cig_rows for w in c], np.uint32),
            "aux_off": np.concatenate([[0], np.cumsum([len(a) for a in aux_rows])]).astype(np.uint32),
            "aux": np.frombuffer(b"".join(aux_rows), np.uint8).copy()}
    return cols, names


@pytest.fixture(scope="module")
def table():
    return make_table()


@pytest.fixture(scope="module", params=[True, False], ids=["records_inside_blocks", "records_across_blocks"])
def bam(request, table, tmp_path_factory):
    cols, names = table
    path = str(tmp_path_factory.mktemp("ev") / ("in_%d.bam" % request.param))
    bamio.write_bam_from_soa(path, CONTIGS, cols, names, aligned=request.param)
    return path


def make_keys(names):
    """40 names of the table (a low-mapq mate and a supplementary alignment among their records), one of them by qhash alone, one name
    the file does not hold, one with the right qhash and a wrong qcheck"""
    present = sorted(set(names))
    chosen = present[::len(present) // 39][:39] + [names[LONG_AT]]
    chosen = list(dict.fromkeys(chosen))
    keys = np.zeros(len(chosen) + 2, abi.READ_KEY)
    for k, n in enumerate(chosen):
        keys[k] = (qhash(n), qcheck(n), k % 3)
    keys[3]["qcheck"] = 0
    absent = b"not-in-the-file"
    keys[len(chosen)] = (qhash(absent), qcheck(absent), 1)
    wrong = present[1] if present[1] not in chosen else present[2]
    assert wrong not in chosen
    keys[len(chosen) + 1] = (qhash(wrong), qcheck(wrong) ^ 0x5A5A, 2)
    return keys, chosen


def rule(cols, keys):
    """per record: the index of the first key it matches, or -1 (the definition of include/breakid_hip.h)"""
    out = np.full(len(cols["tid"]), -1, np.int64)
    for i in range(len(out)):
        for k in range(len(keys)):
            if cols["qhash"][i] == keys[k]["qhash"] and (keys[k]["qcheck"] == 0 or cols["qcheck"][i] == keys[k]["qcheck"]):
                out[i] = k
                break
    return out


def inflated(path):
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


def split_stream(d):
    """(header bytes, [record bytes without block_size])"""
    assert d[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        p += 4 + l_name + 4
    header, recs = d[:p], []
    while p < len(d):
        bs, = struct.unpack_from("<i", d, p)
        assert bs >= 32 and p + 4 + bs <= len(d)
        recs.append(d[p + 4:p + 4 + bs])
        p += 4 + bs
    return header, recs


def bgzf_blocks(raw):
    """[(payload bytes)] of every block, CRC32 and ISIZE checked"""
    out, p = [], 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 10:p + 16] == b"\x06\x00BC\x02\x00", p
        bsize, = struct.unpack_from("<H", raw, p + 16)
        data = zlib.decompress(raw[p + 18:p + bsize + 1 - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, p + bsize + 1 - 8)
        assert crc == zlib.crc32(data) & 0xFFFFFFFF and isize == len(data)
        out.append(data)
        p += bsize + 1
    assert p == len(raw)
    return out


def htslib_layout(header, records):
    """payload sizes of the blocks htslib writes: the header's block flushed, a block flushed before a record that would not fit, 0xff00
    bytes a block at most, the empty EOF block last"""
    sizes, fill = [len(header)], 0
    for r in records:
        n = len(r)
        if fill + n > 0xFF00 and fill:
            sizes.append(fill)
            fill = 0
        while n:
            take = min(n, 0xFF00 - fill)
            fill += take
            n -= take
            if fill == 0xFF00:
                sizes.append(fill)
                fill = 0
    if fill:
        sizes.append(fill)
    return sizes + [0]


def test_extract_selects_by_name(bam, table, tmp_path):
    cols, names = table
    keys, chosen = make_keys(names)
    tags = ["bk0", "bk0,bk3", "bk17"]
    which = rule(cols, keys)
    sel = np.flatnonzero(which >= 0)
    # the rule takes what a name's records are, whatever their flags and mapq: supplementary and low-mapq records are among them
    assert 60 < len(sel) < N_REC and (cols["flag"][sel] & 0x800).any() and (cols["mapq"][sel] == 0).any() and LONG_AT in sel
    assert set(names[i] for i in sel) == set(chosen)
    out = str(tmp_path / "out.bam")
    got_names, n_written = capi.bam_extract(bam, out, keys, tags)
    assert n_written == len(sel)
    assert got_names == [n.decode() for n in chosen] + ["", ""]
    assert sorted(os.listdir(tmp_path)) == ["out.bam"]
    # read back through the project's own reader: the columns are the selected rows, in file order
    contigs, got = capi.decode_bam(out)
    assert contigs == CONTIGS
    for k in ("tid", "pos", "mtid", "mpos", "isize", "flag", "mapq", "qhash", "qcheck"):
        assert np.array_equal(got[k], cols[k][sel]), k
    for name, off in (("cigar", "cigar_off"), ("aux", "aux_off")):
        exp = [cols[name][cols[off][i]:cols[off][i + 1]] for i in sel]
        assert np.array_equal(got[name], np.concatenate(exp)) and np.array_equal(np.diff(got[off].astype(np.int64)), [len(e) for e in exp]), name
    # read back with gzip + struct: header bytes, records, the appended tag, block_size (split_stream checks it), the BGZF layout
    h_in, r_in = split_stream(inflated(bam))
    h_out, r_out = split_stream(inflated(out))
    assert h_out == h_in and len(r_out) == len(sel) and len(r_in) == N_REC
    for j, i in enumerate(sel):
        tail = b"bkZ" + tags[keys[which[i]]["tag"]].encode() + b"\0"
        assert r_out[j] == r_in[i] + tail, (j, i)
        l_name = r_out[j][8]
        assert r_out[j][32:32 + l_name] == names[i] + b"\0"
    with open(out, "rb") as f:
        raw = f.read()
    assert raw[-28:] == EOF_BLOCK
    blocks = bgzf_blocks(raw)
    assert [len(b) for b in blocks] == htslib_layout(h_out, [struct.pack("<i", len(r)) + r for r in r_out])
    assert max(len(b) for b in blocks) <= 0xFF00 and any(len(r) > 0xFF00 for r in r_out)


def test_extract_names_only_and_empty_key_set(bam, table, tmp_path):
    cols, names = table
    keys, chosen = make_keys(names)
    got_names, n_written = capi.bam_extract(bam, None, keys, ["a", "b", "c"])
    assert got_names == [n.decode() for n in chosen] + ["", ""] and n_written == int((rule(cols, keys) >= 0).sum())
    assert os.listdir(tmp_path) == []
    out = str(tmp_path / "empty.bam")
    assert capi.bam_extract(bam, out, np.zeros(0, abi.READ_KEY), []) == ([], 0)
    h_in, _ = split_stream(inflated(bam))
    assert split_stream(inflated(out)) == (h_in, [])
    with open(out, "rb") as f:
        raw = f.read()
    assert raw[-28:] == EOF_BLOCK and [len(b) for b in bgzf_blocks(raw)] == [len(h_in), 0]
    contigs, got = capi.decode_bam(out)
    assert contigs == CONTIGS and len(got["tid"]) == 0
    # the extractor reads its own output: a second tag is appended (a documented limit)
    keys2 = keys[:5].copy()
    first = str(tmp_path / "first.bam")
    n1 = capi.bam_extract(bam, first, keys2, ["x", "y", "z"])[1]
    again = str(tmp_path / "again.bam")
    assert capi.bam_extract(first, again, keys2, ["x", "y", "z"])[1] == n1
    r1, r2 = split_stream(inflated(first))[1], split_stream(inflated(again))[1]
    assert all(b[:len(a)] == a and b[len(a):len(a) + 3] == b"bkZ" for a, b in zip(r1, r2))


def expect_failure(tmp_path, code, in_bam, keys, tags, out_name="out.bam", raw_tags=None):
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(capi.BreakIDError) as e:
        capi.bam_extract(in_bam, str(tmp_path / out_name), keys, tags)
    assert e.value.code == code, str(e.value)
    assert len(str(e.value)) > len("libbreakid_hip error -1: ")
    assert sorted(os.listdir(tmp_path)) == before  # no output file, no temporary file


def test_extract_failures_leave_no_file(bam, table, tmp_path):
    cols, names = table
    keys, _ = make_keys(names)
    tags = ["a", "b", "c"]
    with open(bam, "rb") as f:
        raw = f.read()
    expect_failure(tmp_path, abi.BK_ERR_IO, str(tmp_path / "missing.bam"), keys, tags)
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as f:
        f.write(raw[:len(raw) // 2 + 7])  # inside a block
    expect_failure(tmp_path, abi.BK_ERR_IO, cut, keys, tags)
    bad = bytearray(raw)
    first_len = struct.unpack_from("<H", raw, 16)[0] + 1
    for k in range(40, 60):
        bad[first_len + k] ^= 0xFF  # the deflate data of the second block
    badp = str(tmp_path / "bad.bam")
    with open(badp, "wb") as f:
        f.write(bytes(bad))
    expect_failure(tmp_path, abi.BK_ERR_IO, badp, keys, tags)
    nogz = str(tmp_path / "nogz.bam")
    with open(nogz, "wb") as f:
        f.write(b"this is not a BGZF file at all, but it is long enough")
    expect_failure(tmp_path, abi.BK_ERR_IO, nogz, keys, tags)
    # a record that claims more bytes than the stream holds
    h_in, r_in = split_stream(inflated(bam))
    longrec = str(tmp_path / "longrec.bam")
    w = bamio.BgzfWriter(longrec)
    w.write(h_in + struct.pack("<i", len(r_in[0])) + r_in[0] + struct.pack("<i", len(r_in[1]) + 1000) + r_in[1])
    w.close()
    expect_failure(tmp_path, abi.BK_ERR_IO, longrec, keys, tags)
    dup = np.concatenate([keys, keys[7:8]])
    expect_failure(tmp_path, abi.BK_ERR_ARG, bam, dup, tags)
    high = keys.copy()
    high[2]["tag"] = 3
    expect_failure(tmp_path, abi.BK_ERR_ARG, bam, high, tags)
    expect_failure(tmp_path, abi.BK_ERR_IO, bam, keys, tags, out_name=os.path.join("no_such_dir", "out.bam"))
    L = capi.lib()
    err = C.create_string_buffer(256)
    assert L.bk_bam_extract(None, None, None, 0, None, 0, None, None, err, 256) == abi.BK_ERR_ARG and err.value


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_evidence(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-evidence"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -evidence needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-evidence", "-all", "-fast"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -evidence needs the GPU library" in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-evidence", "-gpus", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "-evidence cannot be combined with -gpus" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-evidence" in r.stderr

"""GPU feed on records shaped like aligner output (breakid_amd/dress.py: bases, qualities, typed aux fields around SA / OC,
hand-written aux LAYOUTS): every decoder path against the generator's own table, the pipeline on the decoded table against
the REAL reference's stage dumps (tests/golden/edge_dressed.*), and the command line against its txt files.

Wall times on an MI355X (pytest --durations): 20 tests, 8.7 s in all; the first decode of the process 1.7 s; writing the four
dressed files once 0.8 s; the run with every output 0.7 s; the decoy files 0.7 / 0.5 s; each command-line case 0.3-0.6 s; parts
0.1-0.3 s; small feed chunks 0.1-0.2 s; across blocks, the pipeline and the overlapped stream pass under 0.1 s."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from breakid_amd import abi, bamio, capi, synth
from tests import dresscases, refdump
from tests.callcases import device_cols
from tests.test_gpu_feed import packed_variant  # noqa: F401  (fixture: records across blocks in chunks / as one batch)
from tools import make_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")


def _cfg():
    """the _dataset() recipe of test_gpu_feed.py at a third of its size"""
    contigs = [("chr1", 3_000_000), ("chr2", 2_000_000), ("chrX", 900_000)]
    ds = synth.make_cfg(9, contigs, 20_000, 40, 30, 300, jitter=200, read_len=100)
    for i in range(0, len(ds.recs), 311):
        ds.recs[i].sa = "chr2,%d,+,40S60M,60,0;" % (100 + i)
        if i % 2:
            ds.recs[i].oc = "60M40S"
    return ds


@pytest.fixture(scope="module")
def files():
    """name -> (Dataset, expected table, {aligned: path}), dressed and written once"""
    with tempfile.TemporaryDirectory() as t:
        out = {}
        for name, ds in (("edge", dresscases.edge_dressed()), ("cfg", _cfg())):
            paths = {}
            for aligned in (True, False):
                paths[aligned] = os.path.join(t, "%s.%d.bam" % (name, aligned))
                dresscases.write_dressed(ds, paths[aligned], aligned=aligned)
            out[name] = (ds, ds.to_soa(), paths)
        yield out


def _check(files, name, aligned):
    ds, ref, paths = files[name]
    table = capi.decode_bam_device(paths[aligned])
    try:
        assert table.contigs == ds.contigs
        dresscases.assert_table(ds, device_cols(table), ref)
    finally:
        table.close()


def test_device_decode_of_dressed_records_in_aligned_blocks(files):
    _check(files, "edge", True)
    _check(files, "cfg", True)


def test_device_decode_of_dressed_records_across_blocks(files, packed_variant):  # noqa: F811
    _check(files, "edge", False)
    _check(files, "cfg", False)


@pytest.mark.parametrize("chunk_mb", ["0.07", "0.25"])
def test_device_decode_of_dressed_records_in_chunks(files, monkeypatch, chunk_mb):
    monkeypatch.setenv("BREAKID_FEED_CHUNK_MB", chunk_mb)
    _check(files, "edge", True)
    _check(files, "cfg", True)
    monkeypatch.setenv("BREAKID_FEED_PACKED_CHUNKS", "1")
    _check(files, "edge", False)
    _check(files, "cfg", False)


@pytest.mark.parametrize("parts", [2, 3, 7])
def test_parts_of_a_dressed_file_tile_its_record_table(files, parts):
    for name in ("edge", "cfg"):
        ds, ref, paths = files[name]
        for aligned in (True, False):
            tables = [capi.decode_bam_device_part(paths[aligned], k, parts) for k in range(parts)]
            try:
                got = [device_cols(tb) for tb in tables]
                assert sum(tb.soa.n for tb in tables) == len(ds.recs)
                cols = {}
                for k, dt in abi.SOA_COLS_ALL:
                    if k in ("cigar_off", "aux_off"):   # offsets restart with every part
                        lens = np.concatenate([np.diff(g[k].astype(np.int64)) for g in got])
                        cols[k] = np.concatenate([[0], np.cumsum(lens)]).astype(dt)
                    else:
                        cols[k] = np.concatenate([g[k] for g in got])
                dresscases.assert_table(ds, cols, ref)
            finally:
                for tb in tables:
                    tb.close()


@pytest.fixture(scope="module")
def dumps(golden_dir):
    return {m: refdump.parse_stages(os.path.join(golden_dir, "edge_dressed.%s.stages.txt" % m)) for m in ("fast", "ahc")}


@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_pipeline_on_the_dressed_device_table_matches_the_reference_dump(files, dumps, mode):
    ds, ref, paths = files["edge"]
    table = capi.decode_bam_device(paths[True])
    ctx = capi.Context(ds.contigs)
    try:
        ctx.attach_device_table(table)
        mean, sd = ctx.isize_stats()
        w, _ = ctx.run(qual=20, fast=(mode == "fast"))
        refdump.compare_with_dump(dumps[mode], [n for n, _ in ds.contigs], ctx.fetch, mean, sd, w)
    finally:
        ctx.close()
        table.close()


def test_stream_pass_overlapped_with_the_feed_of_a_dressed_file(files, dumps, monkeypatch, capfd):
    """bk_bam_decode_device_ctx: the table it leaves is ds.to_soa() (layouts named), the stream pass did run on pieces of the
    file while the rest arrived, and the stages equal the reference dump"""
    ds, ref, paths = files["edge"]
    monkeypatch.setenv("BREAKID_FEED_CHUNK_MB", "0.25")
    monkeypatch.setenv("BK_DEBUG", "feed")
    ctx, table = capi.decode_bam_device_ctx(paths[True], qual=20)
    try:
        err = capfd.readouterr().err
        assert "[feed/stream] stream pass overlapped" in err, err[-600:]
        done, total = [int(v) for v in err.split("[feed/stream] stream pass overlapped:")[1].split("records")[0].replace("of", " ").split()]
        assert total == len(ds.recs) and 0 < done <= total, (done, total)
        assert ctx.contigs == ds.contigs
        dresscases.assert_table(ds, device_cols(table), ref)
        mean, sd = ctx.isize_stats()
        w, _ = ctx.run(qual=20, fast=True)
        refdump.compare_with_dump(dumps["fast"], [n for n, _ in ds.contigs], ctx.fetch, mean, sd, w)
        dresscases.assert_table(ds, device_cols(table), ref)   # the pipeline leaves the table as it was
    finally:
        ctx.close()
        table.close()


@pytest.mark.parametrize("feed", ["gpu", "across", "host"])
@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_cli_reproduces_the_reference_txt_on_the_dressed_file(golden_dir, mode, feed):
    env = {"BK_DEBUG": "feed"}
    if feed == "host":
        env["BREAKID_HOST_DECODE"] = "1"
    err = dresscases.check_cli_reproduces_reference_txt(BIN, golden_dir, mode, aligned=(feed == "gpu"), env_extra=env)
    assert ("[feed/gpu]" in err) == (feed != "host") and ("[feed]" in err) == (feed == "host"), err[-500:]
    assert ("records across blocks" in err) == (feed == "across"), err[-500:]


def _evidence_rows(in_bam, ev_bam):
    """[(read name, flag, tid, pos, bk text)] of an evidence file, after checking it against its input: every record is an
    input record's bytes, unchanged, with bk:Z behind them, in input order"""
    _, recs_in = bamio.read_records(in_bam)
    _, recs_out = bamio.read_records(ev_bam)
    rows, at = [], 0
    for o in recs_out:
        while at < len(recs_in) and not (o.startswith(recs_in[at] + b"bkZ") and o.endswith(b"\0") and b"\0" not in o[len(recs_in[at]) + 3:-1]):
            at += 1
        assert at < len(recs_in), "a record of the evidence file is no input record + bk:Z, or out of order: %r" % o[32:72]
        r = recs_in[at]
        at += 1
        rows.append((r[32:32 + r[8]], r[14:16], r[0:4], r[4:8], o[len(r) + 3:-1]))
    return rows


def test_cli_with_every_output_equals_the_run_on_the_bare_file():
    """-all -genotype -vcf -evidence -clip: every output of the run on the dressed file is, byte for byte, the output of the
    same run on the same records written bare; out_evidence.bam holds the same reads with the same bk tags, as dressed records"""
    ds = dresscases.edge_dressed()
    with tempfile.TemporaryDirectory() as tmp:
        side = synth.write_side_files(ds, tmp, refgene_lines=make_golden.EDGE_REFGENE)
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"])
        env.pop("BREAKID_HOST_DECODE", None)
        outs = {}
        for kind in ("bare", "dressed"):
            d = os.path.join(tmp, kind)
            os.makedirs(d)
            bam = os.path.join(d, "in.bam")
            if kind == "bare":
                ds.write_bam(bam, aligned=True)
            else:
                dresscases.write_dressed(ds, bam, aligned=True)
            bamio.write_bai(bam)
            r = subprocess.run([BIN, "-i", bam, "-o", os.path.join(d, "out"), "-n", side["nib"], "-all", "-fast", "-genotype", "-vcf", "-evidence", "-clip"],
                               env=env, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[kind] = d
        names = sorted(f for f in os.listdir(outs["bare"]) if f.startswith("out"))
        assert names == sorted(f for f in os.listdir(outs["dressed"]) if f.startswith("out")) and "out_evidence.bam" in names and len(names) >= 8, names
        for f in names:
            a, b = (open(os.path.join(outs[k], f), "rb").read() for k in ("bare", "dressed"))
            if f == "out_evidence.bam":
                continue
            if f == "out_performance.txt":   # header + the five deterministic columns; clock() columns follow
                a, b = (b"\n".join([x.split(b"\n")[0], b"\t".join(x.split(b"\n")[1].split(b"\t")[:5])]) for x in (a, b))
            assert a.replace(outs["bare"].encode(), b"<D>") == b.replace(outs["dressed"].encode(), b"<D>"), f
        rows = {k: _evidence_rows(os.path.join(outs[k], "in.bam"), os.path.join(outs[k], "out_evidence.bam")) for k in outs}
        assert rows["bare"] == rows["dressed"] and len(rows["bare"]) > 0


@pytest.mark.parametrize("ends_with_record", [False, True], ids=["chain_at_block_start", "chain_ends_with_its_record"])
def test_decoy_records_inside_a_payload_never_give_another_table(golden_dir, monkeypatch, ends_with_record):
    """a B:C array longer than a BGZF block whose bytes are a chain of more than GUESS_CHAIN well-formed records, the first at
    the first byte of a block (where k_bam_guess looks first): the exact table, or BK_ERR_IO / BK_ERR_LIMIT - never another
    table - and the command line prints the calls of the bare file (it takes the host decoder by itself).  A legal file,
    handled by error codes.  Outcome on an MI355X, in chunks and as one batch alike: chain at a block start
    with payload behind it: BK_ERR_IO "corrupt BAM record"; chain that ends with its record: BK_ERR_IO "record boundaries
    could not be established"; the command line falls back in both."""
    ds = synth.make_g1()
    ref = ds.to_soa()
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, "g1.bam")
        dresscases.write_decoy_chain_file(ds, bam, ends_with_record)
        for variant in ("chunks", "batch"):
            if variant == "batch":
                monkeypatch.setenv("BREAKID_FEED_PACKED_BATCH", "1")
            try:
                table = capi.decode_bam_device(bam)
            except capi.BreakIDError as e:
                print("decoy chain (%s, %s): %s" % ("ends with its record" if ends_with_record else "at a block start", variant, e))
                assert e.code in (abi.BK_ERR_IO, abi.BK_ERR_LIMIT), e
                continue
            try:
                print("decoy chain (%s, %s): decoded" % ("ends with its record" if ends_with_record else "at a block start", variant))
                dresscases.assert_table(ds, device_cols(table), ref)
            finally:
                table.close()
        monkeypatch.delenv("BREAKID_FEED_PACKED_BATCH", raising=False)
        bamio.write_bai(bam)
        side = synth.write_side_files(ds, tmp, refgene_lines=synth.G1_REFGENE)
        prefix = os.path.join(tmp, "out")
        r = subprocess.run([BIN, "-i", bam, "-o", prefix, "-n", side["nib"], "-all", "-fast"], env=dict(os.environ, BREAKID_INSTALLDIR=side["install"]),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for suffix in ("_fusion.txt", "_fusion_all.txt"):
            assert open(prefix + suffix).read() == open(os.path.join(golden_dir, "g1.fast" + suffix)).read(), suffix

"""Checks shared by the feed tests on records shaped like aligner output (test_cpu_dressed, test_gpu_dressed).  The dresser
itself - dressed_records(ds, seed), LAYOUTS, the decoy-chain writer - is breakid_amd/dress.py and is re-exported here."""
import struct

from breakid_amd import bamio, synth
from breakid_amd.dress import *  # noqa: F401,F403
from breakid_amd.dress import LAYOUTS, edge_dressed, write_dressed


def layout_failures(ds, cols):
    """names of the layouts whose record has another blob in the table `cols` than the layout states"""
    bad = []
    by_name = {lay.qname: lay for lay in LAYOUTS}
    aux, off = cols["aux"].tobytes(), cols["aux_off"]
    for i, r in enumerate(ds.recs):
        lay = by_name.get(r.qname)
        if lay is None or not r.flag & 0x40 or r.flag & 0x900 or i + 1 >= len(off):
            continue
        got = aux[int(off[i]):int(off[i + 1])]
        if got != synth.encode_aux(lay.sa, lay.oc):
            bad.append("%s: %r" % (lay.name, got[:80]))
    return bad


def assert_table(ds, cols, ref=None):
    """cols == ds.to_soa() in every column; a wrong layout blob is reported by the layout's name"""
    import numpy as np
    from breakid_amd import abi
    ref = ds.to_soa() if ref is None else ref
    bad = layout_failures(ds, cols)
    assert not bad, "layouts decoded wrongly: " + "; ".join(bad)
    for k, dt in abi.SOA_COLS_ALL:
        n = len(ref[k])   # (an empty cigar / aux column may come back as one placeholder element)
        assert (len(cols[k]) == n or (n == 0 and len(cols[k]) <= 1)) and np.array_equal(np.asarray(cols[k][:n]), ref[k]), "column %s differs" % k


def check_cli_reproduces_reference_txt(binary, golden_dir, mode, aligned, env_extra=None, name="edge_dressed"):
    """`binary` on the dressed edge file: the four txt files the reference wrote for it; returns the run's stderr"""
    import os
    import subprocess
    import tempfile
    from tools import make_golden
    ds = edge_dressed()
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, name + ".bam")
        write_dressed(ds, bam, aligned=aligned)
        bamio.write_bai(bam)  # the reference loads the index before it calls breakpoints
        side = synth.write_side_files(ds, tmp, refgene_lines=make_golden.EDGE_REFGENE)
        prefix = os.path.join(tmp, "out")
        cmd = [binary, "-i", bam, "-o", prefix, "-n", side["nib"], "-all"] + (["-fast"] if mode == "fast" else [])
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        env.update(env_extra or {})
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        for suffix in ("_fusion.txt", "_fusion_all.txt"):
            got = open(prefix + suffix).read()
            exp = open(os.path.join(golden_dir, "%s.%s%s" % (name, mode, suffix))).read()
            assert got == exp, (suffix, got[:600], exp[:600])
        got = open(prefix + "_params.txt").read().replace(tmp, "<TMP>").replace("out_file\t<TMP>/out", "out_file\t<TMP>/out_" + mode)
        assert got == open(os.path.join(golden_dir, "%s.%s_params.txt" % (name, mode))).read()
        perf = open(prefix + "_performance.txt").read().split("\n")
        exp = open(os.path.join(golden_dir, "%s.%s_perf5.txt" % (name, mode))).read().split("\n")
        assert perf[0] == exp[0] and perf[1].split("\t")[:5] == exp[1].split("\t") and len(perf[1].split("\t")) == 9, (perf, exp)
        return r.stderr


def check_extract(in_bam, out_bam, tag_of_name):
    """out_bam holds, in input order, exactly the records of in_bam whose read name is listed, each with its bytes unchanged
    and bk:Z:<tag> appended (block_size grown by exactly that); tag_of_name: {read name bytes: tag text}"""
    head_in, recs_in = bamio.read_records(in_bam)
    head_out, recs_out = bamio.read_records(out_bam)
    assert head_in == head_out
    exp = []
    for r in recs_in:
        name = r[32:32 + r[8]].split(b"\0")[0]
        if name in tag_of_name:
            exp.append(r + b"bkZ" + tag_of_name[name].encode() + b"\0")
    assert len(recs_out) == len(exp), (len(recs_out), len(exp))
    for i, (a, b) in enumerate(zip(recs_out, exp)):
        assert a == b, "record %d of the extract (%r) differs" % (i, b[32:32 + b[8]][:40])
    return len(exp)

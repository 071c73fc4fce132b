"""CPU: the product's HOST code - command line (breakid_main.cc: options, fatal paths, refGene / nib annotation, writers,
_performance.txt) and host BAM decoder (bam_reader.cc) - linked over the CPU oracle by oracle/cpu_shim.cc (test
infrastructure, `make -C oracle cpucli asan ubsan`), plain and under AddressSanitizer / UBSan, against the REFERENCE's
golden txt files.  The same command-line checks run against the real GPU binary in tests/test_gpu_cli.py."""
import os
import subprocess
import sys
import tempfile

import pytest

from breakid_amd import synth
from breakid_amd import bamio
from tools import make_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "oracle", "_san")


@pytest.fixture(scope="module")
def binaries():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "-j3", "san"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return {k: os.path.join(SAN, "BreakID_cpu" + ("" if k == "plain" else "_" + k)) for k in ("plain", "asan", "ubsan")}


def _dataset(name):
    for n, ds, refgene in make_golden.datasets():
        if n == name:
            return ds, refgene
    raise KeyError(name)


def run_cli(binary, name, mode, golden_dir, aligned=True):
    ds, refgene = _dataset(name)
    with tempfile.TemporaryDirectory() as tmp:
        bam = os.path.join(tmp, name + ".bam")
        ds.write_bam(bam, aligned=aligned)
        bamio.write_bai(bam)  # the reference loads the index before it calls breakpoints (BreakID.cc:411-416)
        side = synth.write_side_files(ds, tmp, refgene_lines=refgene)
        prefix = os.path.join(tmp, "out")
        cmd = [binary, "-i", bam, "-o", prefix, "-n", side["nib"], "-all"] + (["-fast"] if mode == "fast" else [])
        env = dict(os.environ, BREAKID_INSTALLDIR=side["install"], ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
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


@pytest.mark.parametrize("name", ["g1", "g2", "small", "ties", "edge"])
@pytest.mark.parametrize("mode", ["fast", "ahc"])
def test_host_code_reproduces_reference_txt(binaries, golden_dir, name, mode):
    run_cli(binaries["plain"], name, mode, golden_dir, aligned=(mode == "fast"))


@pytest.mark.parametrize("san", ["asan", "ubsan"])
@pytest.mark.parametrize("name,mode", [("edge", "fast"), ("ties", "ahc"), ("small", "fast")])
def test_host_code_clean_under_sanitizers(binaries, golden_dir, san, name, mode):
    run_cli(binaries[san], name, mode, golden_dir, aligned=(name != "ties"))


@pytest.mark.parametrize("san", ["asan", "ubsan"])
def test_oracle_unit_entry_points_clean_under_sanitizers(binaries, san):
    """the oracle's unit entry points (CIGAR table, AHC, masks, votes, regions) against the reference's vectors, sanitized"""
    env = dict(os.environ, BREAKID_ORACLE_LIB=os.path.join(SAN, "liboracle_%s.so" % san), ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    if san == "asan":
        env["LD_PRELOAD"] = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_golden.py")],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "runtime error" not in (r.stdout + r.stderr), (r.stdout[-2000:], r.stderr[-2000:])


def fatal_cases(tmp, ds, refgene):
    """(description, argv tail, env patch, expected exit code, expected stderr text) - BreakID.cc:78-91, :1917-1921, :1399-1404,
    :411-416, RefSeqTranscript.cc:212-216"""
    bam = os.path.join(tmp, "in.bam")
    ds.write_bam(bam, aligned=True)
    bamio.write_bai(bam)  # the reference loads the index before it calls breakpoints (BreakID.cc:411-416)
    side = synth.write_side_files(ds, tmp, refgene_lines=refgene)
    noidx = os.path.join(tmp, "noidx.bam")
    ds.write_bam(noidx, aligned=True)
    # an index that is there but does not load (hts_idx_load_local: short read of the magic / foreign magic / file ends inside the
    # bin count of a reference) is the same fatal path as no index at all; an index named <stem>.bai is found like <bam>.bai
    bad = {}
    for what, content in (("emptyidx", b""), ("foreignidx", b"XYZ\1" + bytes(64)), ("shortidx", b"BAI\1" + (len(ds.contigs)).to_bytes(4, "little") + bytes(2))):
        bad[what] = os.path.join(tmp, what + ".bam")
        ds.write_bam(bad[what], aligned=True)
        open(bad[what] + ".bai", "wb").write(content)
    stem = os.path.join(tmp, "stem.bam")
    ds.write_bam(stem, aligned=True)
    bamio.write_bai(stem, os.path.join(tmp, "stem.bai"))
    empty_nib = os.path.join(tmp, "empty_nib")
    os.makedirs(empty_nib)
    no_inst = os.path.join(tmp, "no_install")
    os.makedirs(no_inst)
    ok_env = {"BREAKID_INSTALLDIR": side["install"]}
    return [
        ("help", ["-h"], ok_env, 1, "Usage"),
        ("no output prefix", ["-i", bam], ok_env, 1, "Error: input- and output file is required."),
        ("no nib dir", ["-i", bam, "-o", os.path.join(tmp, "o")], ok_env, 1, "Error: nib file's root dir is required."),
        ("missing bam", ["-i", os.path.join(tmp, "nope.bam"), "-o", os.path.join(tmp, "o"), "-n", side["nib"]], ok_env, 1,
         "Error: can not open bam-file: " + os.path.join(tmp, "nope.bam")),
        ("missing ref_names.txt", ["-i", bam, "-o", os.path.join(tmp, "o"), "-n", empty_nib], ok_env, 1, "Error: cannot open reference names file."),
        ("missing index", ["-i", noidx, "-o", os.path.join(tmp, "o"), "-n", side["nib"], "-fast"], ok_env, 1, "Error: please index bam-file first:\t" + noidx),
        ("empty index", ["-i", bad["emptyidx"], "-o", os.path.join(tmp, "o"), "-n", side["nib"], "-fast"], ok_env, 1, "Error: please index bam-file first:\t" + bad["emptyidx"]),
        ("foreign index", ["-i", bad["foreignidx"], "-o", os.path.join(tmp, "o"), "-n", side["nib"], "-fast"], ok_env, 1, "Error: please index bam-file first:\t" + bad["foreignidx"]),
        ("truncated index", ["-i", bad["shortidx"], "-o", os.path.join(tmp, "o"), "-n", side["nib"], "-fast"], ok_env, 1, "Error: please index bam-file first:\t" + bad["shortidx"]),
        ("index named after the stem", ["-i", stem, "-o", os.path.join(tmp, "o2"), "-n", side["nib"], "-fast"], ok_env, 0, ""),
        ("missing refGene.txt", ["-i", bam, "-o", os.path.join(tmp, "o"), "-n", side["nib"], "-fast"], {"BREAKID_INSTALLDIR": no_inst}, 1,
         "Error: cannot open \t" + os.path.join(no_inst, "ref_files", "refGene.txt")),
    ]


def check_fatal_paths(binary):
    ds, refgene = _dataset("g1")
    with tempfile.TemporaryDirectory() as tmp:
        for what, argv, envp, code, text in fatal_cases(tmp, ds, refgene):
            r = subprocess.run([binary] + argv, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **envp), capture_output=True, text=True)
            assert r.returncode == code and text in r.stderr, (what, r.returncode, r.stderr[-400:])


@pytest.mark.parametrize("which", ["plain", "asan", "ubsan"])
def test_fatal_paths_match_the_reference_messages(binaries, which):
    check_fatal_paths(binaries[which])


# (options behind `-i in.bam -o out -n nib`, the one "Error:" line of the CPU build, that of the GPU build where it differs): command
# lines that break one option rule, or two at once - which message wins is behaviour.  A line that starts with a blank stands behind
# the help text.  Every answer has exit status 1 and comes before any file is opened for writing or the GPU is touched; in.bam does not
# exist, so a command line the GPU build accepts ends at "can not open bam-file".  The CPU build has none of the per-call entry points
# of the library: where the GPU build goes on to an option's ranges, it stops at "needs the GPU library".  Recorded from the binaries
# of the commit in front of the split of main() into stages.
GPU_LIB = "Error: %s needs the GPU library"
NO_GPUS = " Error: %s cannot be combined with -gpus."
REFUSALS = [
    ("-clip -gpus 2", GPU_LIB % "-clip", NO_GPUS % "-clip"),  # -clip looks for the library first, every other option for -gpus
    ("-vcf -gpus 2", NO_GPUS % "-vcf", None),
    ("-homology", " Error: -homology needs -consensus.", None),
    ("-consensus -homology -gpus 2", NO_GPUS % "-homology", None),
    ("-homshift 3", " Error: -homshift and -homins need -homology.", None),
    ("-conslen 0 -consensus", GPU_LIB % "-consensus", " Error: -conslen must be a number from 1 to 256."),
    ("-consensus -minclip 0", GPU_LIB % "-consensus", " Error: -minclip must be a number from 1 to 2147483647."),
    ("-minclip 5", " Error: -minclip and -clipsupport need -clip.", None),
    ("-consensus -minclip 5", GPU_LIB % "-consensus", "Error: can not open bam-file: in.bam"),
    ("-anchor 3", " Error: -anchor needs -genotype.", None),
    ("-genotype -anchor -1", " Error: -anchor must be a number from 0 to 2147483647.", None),
    ("-clip -clipsupport 0", GPU_LIB % "-clip", " Error: -minclip and -clipsupport must be numbers from 1 to 2147483647."),
    ("-normal /nonexistent", GPU_LIB % "-normal", "Error: can not open normal bam-file: /nonexistent"),
    ("-x /nonexistent", GPU_LIB % "-x", "Error: can not open exclude file: /nonexistent"),
    ("-dedup -evidence -gpus 2", NO_GPUS % "-evidence", None),
    ("-normal /nonexistent -gpus 2", NO_GPUS % "-normal", None),
    ("-genotype -gpus 2", NO_GPUS % "-genotype", None),
    ("-consensus -gpus 2", NO_GPUS % "-consensus", None),
    ("-dedup -gpus 2", NO_GPUS % "-dedup", None),
    ("-consensus -homology -homins 65", GPU_LIB % "-homology", " Error: -homshift and -homins must be numbers from 0 to 64."),
    ("-conslen 5", " Error: -conslen needs -consensus.", None),
    ("-clipsupport 2", " Error: -minclip and -clipsupport need -clip.", None),
    ("-homology -gpus 2", " Error: -homology needs -consensus.", None),
    ("-vcf -clip -gpus 2", NO_GPUS % "-vcf", None),
    ("-anchor 3 -vcf -gpus 2", " Error: -anchor needs -genotype.", None),
    ("-consensus -conslen 0 -minclip 0", GPU_LIB % "-consensus", " Error: -conslen must be a number from 1 to 256."),
    ("-clip -x /nonexistent -gpus 2", GPU_LIB % "-clip", NO_GPUS % "-clip"),
    ("-clip -minclip 0 -gpus 2", GPU_LIB % "-clip", NO_GPUS % "-clip"),
    ("-consensus -homology -homshift -1 -conslen 0", GPU_LIB % "-homology", " Error: -homshift and -homins must be numbers from 0 to 64."),
    ("-evidence", GPU_LIB % "-evidence", "Error: can not open bam-file: in.bam"),
]


def check_refusals(binary, gpu_build):
    with tempfile.TemporaryDirectory() as tmp:
        for options, cpu_line, gpu_line in REFUSALS:
            line = gpu_line if gpu_build and gpu_line is not None else cpu_line
            r = subprocess.run([binary, "-i", "in.bam", "-o", "out", "-n", "nib"] + options.split(), cwd=tmp, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"),
                               capture_output=True, text=True)
            errors = [l for l in r.stderr.split("\n") if "Error" in l]
            assert r.returncode == 1 and errors == [line] and ("Usage" in r.stderr) == line.startswith(" "), (options, r.returncode, r.stderr[-400:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
            assert os.listdir(tmp) == [], options


@pytest.mark.parametrize("which", ["plain", "asan", "ubsan"])
def test_option_rules_refuse_with_the_recorded_message(binaries, which):
    check_refusals(binaries[which], gpu_build=False)

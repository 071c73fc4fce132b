#!/usr/bin/env python3
"""Record tests/golden/cli_matrix.json: what the BreakID command line writes for a matrix of option combinations on two designed
inputs.  The recording pins the host side of the program (breakid_amd/csrc/breakid_main.cc) byte for byte: it is made ONCE, on the
GPU, from the binary of the commit named in it, and tests/test_gpu_cli.py compares every later binary against it.

    python tools/make_cli_matrix.py [--binary breakid_amd/bin/BreakID] [--commit HASH] [--out tests/golden/cli_matrix.json]

Inputs (the designed BAMs of the CLI tests, with their side files): "plus" is the BAM of tests/test_gpu_homology.py with real bases
and nib files of the same genome; "clip" is the BAM of tests/test_gpu_clip.py whose unvoted clusters are rescued.  Every run has the
input's directory as working directory and relative paths, so that _params.txt and stdout are stable.

Per run: the files written, per text file its sha256, line count and data-line count, _performance.txt by its header and first five
columns (four clock() columns follow), each .bam by the sha256 of its inflated bytes (the deflate stream is zlib's business), stdout
without the "costs time" line, the exit status.  The inputs are pinned the same way (BAM by its inflated bytes)."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_matrix.json")
BIN = os.path.join(ROOT, "breakid_amd", "bin", "BreakID")
INPUTS = ("plus", "clip")
# -x: background records go, the designed loci stay (tests/callcases.py: EXCLUDE)
BED = "# exclude list of the command-line matrix\nchr1\t50000\t60000\nchr4 100000 120000\n"

ALONE = [("normal", ["-normal", "t.bam"]), ("x", ["-x", "x.bed"]), ("genotype", ["-genotype"]), ("vcf", ["-vcf"]), ("evidence", ["-evidence"]), ("clip", ["-clip"]),
         ("dedup", ["-dedup"]), ("consensus_homology", ["-consensus", "-homology"])]
EVERYTHING = ["-fast", "-normal", "t.bam", "-x", "x.bed", "-genotype", "-anchor", "7", "-vcf", "-evidence", "-clip", "-minclip", "12", "-clipsupport", "2", "-dedup",
              "-consensus", "-conslen", "50", "-homology", "-homshift", "40", "-homins", "10"]

TWINS = ("", "_normal", "_genotype", "_clip", "_dedup", "_consensus", "_homology")
# every kind of file that holds calls: each must have a data line in at least one run of the matrix
KINDS = tuple("_fusion%s%s.txt" % (a, t) for t in TWINS for a in ("", "_all")) + (
    "_fusion_rescued.txt", "_fusion_rescued_normal.txt", "_fusion.vcf", "_fusion_rescued.vcf", "_evidence.txt", "_evidence_rescued.txt")


def command_lines():
    """[(name of the run, the options behind -i t.bam -o <name> -n nib)]"""
    runs = [("none", []), ("all", ["-all"])]
    runs += [("all_" + name, ["-all"] + args) for name, args in ALONE]
    runs += [("all_everything", ["-all"] + EVERYTHING), ("everything", list(EVERYTHING)), ("all_x_gpus1_local", ["-all", "-x", "x.bed", "-gpus", "1", "-comm", "local"])]
    return runs


def build_inputs(root):
    """{input: its directory}: t.bam (+ .bai), nib/, install/ref_files/refGene.txt, x.bed"""
    from breakid_amd import bamio, synth
    from tests import callcases, clipcases, homologycases
    dirs = {}
    for which in INPUTS:
        d = dirs[which] = os.path.join(root, which)
        os.makedirs(d)
        bam = os.path.join(d, "t.bam")
        if which == "plus":
            homologycases.write_plus_bam(bam)
            bamio.write_bai(bam)
            side = synth.write_side_files(homologycases.designed_plus()["ds"], d, refgene_lines=callcases.designed_refgene())
            homologycases.write_nib_dir(side["nib"], homologycases.genome())
        else:
            ds = clipcases.clip_tumor()
            callcases.write_indexed(ds, bam)
            synth.write_side_files(ds, d, refgene_lines=callcases.designed_refgene())
        with open(os.path.join(d, "x.bed"), "w") as f:
            f.write(BED)
    return dirs


def sha(data):
    return hashlib.sha256(data).hexdigest()


def input_hashes(d):
    out = {"t.bam (inflated)": sha(gzip.decompress(open(os.path.join(d, "t.bam"), "rb").read()))}
    for rel in ["x.bed", "install/ref_files/refGene.txt"] + sorted("nib/" + f for f in os.listdir(os.path.join(d, "nib"))):
        out[rel] = sha(open(os.path.join(d, rel), "rb").read())
    return out


def run_one(binary, d, name, args):
    env = dict(os.environ, BREAKID_INSTALLDIR=os.path.join(d, "install"))
    for k in ("BREAKID_HOST_DECODE", "BK_DEBUG", "BREAKID_FEED_CHUNK_MB"):
        env.pop(k, None)
    r = subprocess.run([binary, "-i", "t.bam", "-o", name, "-n", "nib"] + args, cwd=d, env=env, capture_output=True, text=True, timeout=120)
    rec = {"args": args, "exit": r.returncode, "stdout": [l for l in r.stdout.split("\n") if "costs time" not in l], "files": {}}
    if r.returncode != 0:
        rec["stderr"] = r.stderr[-2000:]
    for f in sorted(os.listdir(d)):
        if not f.startswith(name + "_"):
            continue
        suffix, data = f[len(name):], open(os.path.join(d, f), "rb").read()
        if suffix.endswith(".bam"):
            rec["files"][suffix] = {"sha256 (inflated)": sha(gzip.decompress(data))}
        elif suffix == "_performance.txt":
            lines = data.decode().split("\n")
            rec["files"][suffix] = {"header": lines[0], "first5": lines[1].split("\t")[:5], "columns": len(lines[1].split("\t")), "lines": len(lines) - 1}
        else:
            lines = data.decode().split("\n")[:-1]
            head = sum(l.startswith("#") for l in lines) if suffix.endswith(".vcf") else 1
            rec["files"][suffix] = {"sha256": sha(data), "lines": len(lines), "data": len(lines) - head}
    return rec


def kinds_without_data(matrix):
    """the kinds of file that have no data line in any run of the recording"""
    have = set()
    for runs in matrix["runs"].values():
        for rec in runs.values():
            have.update(s for s, f in rec["files"].items() if f.get("data", 0) > 0)
    return [k for k in KINDS if k not in have]


def record(binary, dirs):
    """every run of the matrix; the first run that fails ends the recording (nothing else is started behind a failed program)"""
    matrix = {"inputs": {which: input_hashes(dirs[which]) for which in INPUTS}, "runs": {which: {} for which in INPUTS}}
    for which in INPUTS:
        for name, args in command_lines():
            rec = matrix["runs"][which][name] = run_one(binary, dirs[which], name, args)
            if rec["exit"] != 0:
                raise RuntimeError("%s / %s: exit %d: %s" % (which, name, rec["exit"], rec["stderr"]))
    return matrix


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--binary", default=BIN)
    ap.add_argument("--commit", help="the commit whose breakid_main.cc the binary was built from (default: HEAD, which must hold it unchanged)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    commit = a.commit
    if not commit:
        main_cc = os.path.join("breakid_amd", "csrc", "breakid_main.cc")
        if subprocess.run(["git", "diff", "--quiet", "HEAD", "--", main_cc], cwd=ROOT).returncode != 0:
            sys.exit("make_cli_matrix: %s differs from HEAD: commit it, or name the commit it was built from with --commit" % main_cc)
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        matrix = record(os.path.abspath(a.binary), build_inputs(tmp))
    matrix = dict(commit=commit, source="breakid_amd/csrc/breakid_main.cc", **matrix)
    with open(a.out, "w") as f:
        json.dump(matrix, f, indent=1, sort_keys=True)
        f.write("\n")
    print("cli matrix: %d runs, commit %s -> %s" % (sum(len(r) for r in matrix["runs"].values()), commit, a.out))
    if kinds_without_data(matrix):
        sys.exit("make_cli_matrix: kinds of file without a data line in any run: %s" % kinds_without_data(matrix))


if __name__ == "__main__":
    main()

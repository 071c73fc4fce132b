"""CPU: the host side of the soft-clip evidence (`-clip`, `bk_clip_support`, `bk_clip_rescue`): the numpy mirror of the row, the
rescue rule of the library over hand-made rows, the numpy definition the GPU tests check against on records worked out by hand, and
the command line built over the CPU oracle (oracle/cpu_shim.cc), which has no `bk_clip_support` and must refuse `-clip` cleanly."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi, synth
from tests import clipcases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_clip_support_row_layout():
    assert abi.CLIP_SUPPORT.itemsize == 64
    assert [abi.CLIP_SUPPORT.fields[f][1] for f in ("at", "peak_pos", "peak_n", "events")] == [0, 16, 32, 48]
    s = np.zeros(1, abi.CLIP_SUPPORT)
    s["peak_n"][0, 1, 0] = 7  # [side][dir], the side is the slower index
    assert s.view(np.uint32)[8 + 2] == 7
    assert all(name in capi.EXPORTS for name in ("bk_clip_support", "bk_base_depth", "bk_clip_rescue"))


def row(flags=1, t1=0, t2=1, pairs=(14, 0, 0, 0), splits=(0, 0, 0, 0), peak_n=((0, 0), (0, 0)), peak_pos=((0, 0), (0, 0))):
    c, j, s = np.zeros(1, abi.CLUSTER), np.zeros(1, abi.JUNCTION), np.zeros(1, abi.CLIP_SUPPORT)
    c["flags"], c["p1_tid"], c["p2_tid"] = flags, t1, t2
    j["pairs"][0], j["splits"][0] = pairs, splits
    s["peak_n"][0], s["peak_pos"][0] = peak_n, peak_pos
    return c[0], j[0], s[0]


# (row, min_support, what bk_clip_rescue must give).  pairs[2 * p1_rev + p2_rev]: a forward read lies left of its breakpoint (dir 0),
# a reverse read right of it (dir 1)
RESCUE = [
    # both pairs forward: (LEFT, LEFT); three reads at 500 and four at 900
    (row(pairs=(14, 0, 0, 0), peak_n=((3, 0), (4, 0)), peak_pos=((500, 0), (900, 0))), 3, (500, 900, 3, 4)),
    # one below the threshold on side 2
    (row(pairs=(14, 0, 0, 0), peak_n=((3, 0), (2, 0)), peak_pos=((500, 0), (900, 0))), 3, None),
    (row(pairs=(14, 0, 0, 0), peak_n=((3, 0), (2, 0)), peak_pos=((500, 0), (900, 0))), 2, (500, 900, 3, 2)),
    # the peaks lie in the other direction than the pairs say
    (row(pairs=(14, 0, 0, 0), peak_n=((0, 9), (0, 9)), peak_pos=((0, 500), (0, 900))), 3, None),
    # (forward, reverse): (LEFT, RIGHT)
    (row(pairs=(0, 14, 0, 0), peak_n=((5, 1), (1, 6)), peak_pos=((500, 7), (8, 900))), 3, (500, 900, 5, 6)),
    # (reverse, forward): (RIGHT, LEFT)
    (row(pairs=(0, 0, 14, 0), peak_n=((1, 5), (6, 1)), peak_pos=((7, 500), (900, 8))), 3, (500, 900, 5, 6)),
    # (reverse, reverse), and the smallest index wins a tie among the pairs: 7 : 7 between bins 1 and 3 gives bin 1
    (row(pairs=(0, 0, 0, 14), peak_n=((0, 5), (0, 6)), peak_pos=((0, 500), (0, 900))), 3, (500, 900, 5, 6)),
    (row(pairs=(0, 7, 0, 7), peak_n=((5, 0), (0, 6)), peak_pos=((500, 0), (0, 900))), 3, (500, 900, 5, 6)),
    # a voted row is never rescued, whatever its peaks
    (row(flags=3, pairs=(14, 0, 0, 0), peak_n=((9, 9), (9, 9)), peak_pos=((500, 500), (900, 900))), 3, None),
    # a side without a chromosome
    (row(t1=-1, pairs=(14, 0, 0, 0), peak_n=((9, 9), (9, 9)), peak_pos=((500, 500), (900, 900))), 3, None),
    (row(t2=-1, pairs=(14, 0, 0, 0), peak_n=((9, 9), (9, 9)), peak_pos=((500, 500), (900, 900))), 3, None),
    # no pair at all: index 1, (LEFT, RIGHT)
    (row(pairs=(0, 0, 0, 0), peak_n=((3, 0), (0, 3)), peak_pos=((500, 0), (0, 900))), 3, (500, 900, 3, 3)),
    # exactly at a large threshold
    (row(pairs=(14, 0, 0, 0), peak_n=((2 ** 32 - 1, 0), (2 ** 32 - 1, 0)), peak_pos=((500, 0), (900, 0))), 2 ** 32 - 1, (500, 900, 2 ** 32 - 1, 2 ** 32 - 1)),
]


def test_clip_rescue_over_hand_made_rows():
    for k, ((c, j, s), support, want) in enumerate(RESCUE):
        assert capi.clip_rescue(c, j, s, support) == want, k
        assert kc.expected_rescue(c, j, s, support) == want, k
    c, j, s = RESCUE[0][0]
    with pytest.raises(capi.BreakIDError) as e:
        capi.clip_rescue(c, j, s, 0)
    assert e.value.code == abi.BK_ERR_ARG
    assert capi.lib().bk_clip_rescue(None, None, None, 3, None, None, None, None) == abi.BK_ERR_ARG


def test_definition_on_records_worked_out_by_hand():
    """One cluster chr1 / chr2, p1 in [1000, 1200], p2 in [5000, 5100], voted at 1100 / 5050, W = 100: windows [900, 1300] and
    [4900, 5200].  Records on chr1 unless said otherwise, min_clip 10, mapq_min 20:
      r0  pos 1040  60M40S        trailing at 1040 + 60 = 1100 (LEFT): in the window, |1100 - 1100| <= 2
      r1  pos 1042  5H60M38S5H    trailing at 1102 (LEFT): the H is skipped; in the window, at the breakpoint too
      r2  pos 1099  40S60M        leading at 1100 (RIGHT)
      r3  pos 1040  60M40S        trailing at 1100 again: the LEFT peak is 1100 with 2 reads
      r4  pos 839   20S60M20S     leading at 840 (outside), trailing at 899 (outside: the window begins at 900)
      r5  pos 840   20S60M20S     leading at 841 (outside), trailing at 900 (the first position of the window)
      r6  pos 1240  30M200N30M9S  trailing clip of 9 < 10: nothing (at min_clip 9: trailing at 1500, outside)
      r7  pos 1103  12S88M        leading at 1104 (RIGHT): in the window, 4 bp from the breakpoint
      r8  pos 1040  60M40S mapq 19, r9 0x400, r10 with an SA tag, r11 100S: nothing
      r12 chr2 pos 4899 40S60M    leading at 4900 on side 2 (RIGHT), the first position of its window
      r13 chr2 pos 5140 40M5D20M40S  trailing at 5140 + 65 = 5205 (outside: the window ends at 5200)
    So side 1: events LEFT 4 (1100 x 2, 1102, 900), RIGHT 2 (1100, 1104); peaks LEFT (1100, 2), RIGHT (1100, 1: the smaller of a
    tie); at LEFT 3, at RIGHT 1.  Side 2: events RIGHT 1, peak (4900, 1), nothing at the breakpoint."""
    R = synth.Rec
    F = 0x1 | 0x2 | 0x20 | 0x40
    recs = [R("r0", F, 0, 1040, 60, "60M40S", 0, 1300, 300), R("r1", F, 0, 1042, 60, "5H60M38S5H", 0, 1300, 300), R("r2", F, 0, 1099, 60, "40S60M", 0, 1300, 300),
            R("r3", F, 0, 1040, 60, "60M40S", 0, 1300, 300), R("r4", F, 0, 839, 60, "20S60M20S", 0, 1300, 300), R("r5", F, 0, 840, 60, "20S60M20S", 0, 1300, 300),
            R("r6", F, 0, 1240, 60, "30M200N30M9S", 0, 1300, 300), R("r7", F, 0, 1103, 60, "12S88M", 0, 1300, 300), R("r8", F, 0, 1040, 19, "60M40S", 0, 1300, 300),
            R("r9", F | 0x400, 0, 1040, 60, "60M40S", 0, 1300, 300), R("r10", F, 0, 1040, 60, "60M40S", 0, 1300, 300, sa="chr2,5000,+,60S40M,60,0;"),
            R("r11", F, 0, 1040, 60, "100S", 0, 1300, 300), R("r12", F, 1, 4899, 60, "40S60M", 1, 5200, 300), R("r13", F, 1, 5140, 60, "40M5D20M40S", 1, 5400, 300)]
    ds = synth.Dataset([("chr1", 100_000), ("chr2", 100_000)], recs)
    ds.sort()
    cols = ds.to_soa()
    cl = np.zeros(2, abi.CLUSTER)
    for c in cl:
        c["p1_tid"], c["p2_tid"], c["p1_min"], c["p1_max"], c["p2_min"], c["p2_max"], c["p1_exact"], c["p2_exact"] = 0, 1, 1000, 1200, 5000, 5100, 1100, 5050
    cl["flags"] = (3, 1)  # the same row voted and unvoted
    got = kc.expected_clip_support(cl, cols, 20, 10, 100.9)
    v = got[0]
    assert v["events"].tolist() == [[4, 2], [0, 1]]
    assert v["peak_n"].tolist() == [[2, 1], [0, 1]]
    assert v["peak_pos"].tolist() == [[1100, 1100], [0, 4900]]
    assert v["at"].tolist() == [[3, 1], [0, 0]]
    u = got[1]
    assert not u["at"].any() and all(np.array_equal(u[f], v[f]) for f in ("events", "peak_n", "peak_pos"))
    # the parameters: a shorter clip lets r6 in (outside the window all the same) ...
    tid, p, d = kc.clip_events(cols, 20, 9)
    assert (0, 1500, kc.LEFT) in set(zip(tid.tolist(), p.tolist(), d.tolist()))
    assert (0, 1500, kc.LEFT) not in set(zip(*[x.tolist() for x in kc.clip_events(cols, 20, 10)]))
    # ... a lower mapq threshold r8, and a wider window r4's trailing event and r13's
    assert kc.expected_clip_support(cl, cols, 19, 10, 100.9)[0]["peak_n"].tolist() == [[3, 1], [0, 1]]
    wide = kc.expected_clip_support(cl, cols, 20, 10, 105.0)[0]
    assert wide["events"].tolist() == [[5, 2], [1, 1]] and wide["peak_pos"].tolist() == [[1100, 1100], [5205, 4900]]


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_clip(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    for extra in (["-clip"], ["-clip", "-gpus", "2"], ["-clip", "-minclip", "12", "-clipsupport", "2"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "Error: -clip needs the GPU library" in r.stderr, r.stderr[-2000:]
    for extra in (["-minclip", "12"], ["-clipsupport", "2"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "need -clip" in r.stderr, r.stderr[-2000:]
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())

"""Window context without a GPU: the row layout and the exports, the two statements of the definition (tests/contextcases.py) against
each other on random and on designed tables, additivity of adjacent windows, the formatting of the twin columns, and the command line's
refusals."""
import os
import subprocess

import numpy as np
import pytest

from breakid_amd import abi, capi
from tests import contextcases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BIN = os.path.join(ROOT, "oracle", "_san", "BreakID_cpu")


def test_row_layout_and_exports():
    assert abi.WINDOW_CTX.itemsize == 40
    assert list(abi.WINDOW_CTX.names) == ["mapq_sum", "reads", "mq0", "lowq", "clipped", "improper", "orphan", "dup", "secsup"]
    assert [abi.WINDOW_CTX.fields[f][1] for f in abi.WINDOW_CTX.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36]
    assert abi.WINDOW_CTX.fields["mapq_sum"][0] == np.dtype("<u8") and all(abi.WINDOW_CTX.fields[f][0] == np.dtype("<u4") for f in abi.WINDOW_CTX.names[1:])
    assert "bk_window_context" in capi.EXPORTS and hasattr(capi.lib(), "bk_window_context") and hasattr(capi.Context, "window_context")
    header = open(os.path.join(ROOT, "include", "breakid_hip.h")).read()
    assert "struct bk_window_ctx { uint64_t mapq_sum; uint32_t reads, mq0, lowq, clipped, improper, orphan, dup, secsup; };" in header
    assert "int bk_window_context(bk_ctx *records, const struct bk_cov_window *windows, uint64_t n, int mapq_min, const struct bk_window_ctx **out);" in header
    assert "NOT by overlap" in header and "are not modelled" in header


def windows_around(cols, rng, n_targets, lengths):
    rows = [(-1, 0, 100), (n_targets, 0, 100), (0, 50, 50), (0, 60, 50), (0, 0, 1 << 31), (n_targets - 1, 0, 0xFFFFFFFF)]
    for i in range(len(cols["tid"])):
        t, p = int(cols["tid"][i]), int(cols["pos"][i])
        if t >= 0 and rng.random() < 0.3:
            rows += [(t, max(0, p + d), p + d2) for d in (-1, 0, 1) for d2 in (0, 1, 2)] + [(t, p, p + 1), (t, 0, p), (t, p, lengths[t])]
    for _ in range(20):
        a = int(rng.integers(0, 1000))
        rows.append((int(rng.integers(0, n_targets)), a, a + int(rng.integers(0, 400))))
    return xc.as_windows(rows)


def test_the_two_statements_agree_on_random_tables():
    rng = np.random.default_rng(31)
    seen = dict.fromkeys(xc.FIELDS, 0)
    for case in range(40):
        n = int(rng.integers(0, 80))
        cols = xc.random_table(rng, n, [(0, 600), (2, 900)], read_len=int(rng.integers(5, 80)), unmapped=case % 3)
        windows = windows_around(cols, rng, 3, [600, 500, 900])
        for q in (0, 20, 61, 300):
            fast, slow = xc.expected_ctx(cols, 3, windows, q), xc.expected_ctx_slow(cols, 3, windows, q)
            assert fast.tobytes() == slow.tobytes(), (case, q)
            for f in xc.FIELDS:
                seen[f] += int(fast[f].sum())
        assert not fast[:4].tobytes().strip(b"\0")
        assert not int(xc.expected_ctx(cols, 3, windows, 0)["lowq"].sum())
    assert all(v > 100 for v in seen.values()), seen


# each record is one interesting case; q = 20.  (tid, pos, flag, mapq, cigar): the positions are all different
Q = 20
DESIGNED = [
    (0, 100, 0x0, 60, "100M"),                 # unpaired, plain
    (0, 110, 0x4, 60, "100M"),                 # tid >= 0 with 0x4: counts nowhere
    (0, 120, 0x100, 60, "100M"), (0, 130, 0x200, 60, "100M"), (0, 140, 0x400, 60, "100M"), (0, 150, 0x800, 60, "100M"),
    (0, 160, 0x4 | 0x100, 60, "100M"), (0, 170, 0x4 | 0x400, 60, "100M"), (0, 180, 0x4 | 0x800, 60, "100M"), (0, 190, 0x4 | 0x200, 60, "100M"),
    (0, 200, 0x100 | 0x200, 60, "100M"),       # still secsup
    (0, 210, 0x100 | 0x400, 60, "100M"), (0, 220, 0x100 | 0x800, 60, "100M"), (0, 230, 0x200 | 0x400, 60, "100M"), (0, 240, 0x200 | 0x800, 60, "100M"),
    (0, 250, 0x400 | 0x800, 60, "100M"),       # secsup and not dup
    (0, 300, 0x1 | 0x2, 0, "100M"), (0, 310, 0x1 | 0x2, Q - 1, "100M"), (0, 320, 0x1 | 0x2, Q, "100M"), (0, 330, 0x1 | 0x2, 255, "100M"),
    (0, 400, 0x1, 60, "100M"),                 # improper
    (0, 410, 0x1 | 0x8, 60, "100M"),           # orphan
    (0, 420, 0x1 | 0x8 | 0x2, 60, "100M"),     # orphan whatever 0x2 says
    (0, 430, 0x8, 60, "100M"),                 # unpaired: 0x8 means nothing
    (0, 440, 0x1 | 0x4 | 0x8, 0, ""),          # a placed unmapped mate
    (0, 500, 0x1 | 0x2, 60, "10S90M"), (0, 510, 0x1 | 0x2, 60, "90M10S"), (0, 520, 0x1 | 0x2, 60, "5H10S85M"), (0, 530, 0x1 | 0x2, 60, "85M10S5H"),
    (0, 540, 0x1 | 0x2, 60, "5H95M"), (0, 550, 0x1 | 0x2, 60, "95M5H"), (0, 560, 0x1 | 0x2, 60, "100S"), (0, 570, 0x1 | 0x2, 60, ""),
    (0, 580, 0x1 | 0x2, 60, "50M10S40M"), (0, 590, 0x1 | 0x2, 60, "7S"), (0, 600, 0x1 | 0x2, 60, "5H"), (0, 610, 0x1 | 0x2, 60, "5H5H"),
    (0, 620, 0x1 | 0x2, 60, "5H10S5H"), (0, 630, 0x1 | 0x2, 60, "5H5H10S90M"),  # (two leading H: only one is skipped)
    (0, 640, 0x400, 60, "10S90M"),             # a clipped duplicate is a duplicate and nothing else
]
BY_HAND = {100: {"reads": 1, "mapq_sum": 60}, 110: {}, 120: {"secsup": 1}, 130: {}, 140: {"dup": 1}, 150: {"secsup": 1}, 160: {}, 170: {}, 180: {}, 190: {},
           200: {"secsup": 1}, 210: {"secsup": 1}, 220: {"secsup": 1}, 230: {}, 240: {"secsup": 1}, 250: {"secsup": 1},
           300: {"reads": 1, "mq0": 1, "lowq": 1}, 310: {"reads": 1, "lowq": 1, "mapq_sum": Q - 1}, 320: {"reads": 1, "mapq_sum": Q}, 330: {"reads": 1, "mapq_sum": 255},
           400: {"reads": 1, "mapq_sum": 60, "improper": 1}, 410: {"reads": 1, "mapq_sum": 60, "orphan": 1}, 420: {"reads": 1, "mapq_sum": 60, "orphan": 1},
           430: {"reads": 1, "mapq_sum": 60}, 440: {},
           500: {"reads": 1, "mapq_sum": 60, "clipped": 1}, 510: {"reads": 1, "mapq_sum": 60, "clipped": 1}, 520: {"reads": 1, "mapq_sum": 60, "clipped": 1},
           530: {"reads": 1, "mapq_sum": 60, "clipped": 1}, 540: {"reads": 1, "mapq_sum": 60}, 550: {"reads": 1, "mapq_sum": 60}, 560: {"reads": 1, "mapq_sum": 60, "clipped": 1},
           570: {"reads": 1, "mapq_sum": 60}, 580: {"reads": 1, "mapq_sum": 60}, 590: {"reads": 1, "mapq_sum": 60, "clipped": 1}, 600: {"reads": 1, "mapq_sum": 60},
           610: {"reads": 1, "mapq_sum": 60}, 620: {"reads": 1, "mapq_sum": 60, "clipped": 1}, 630: {"reads": 1, "mapq_sum": 60}, 640: {"dup": 1}}


def designed_table():
    cols = xc.make_cols(DESIGNED)
    windows = xc.as_windows([(0, r[1], r[1] + 1) for r in DESIGNED] + [(0, 0, 1000), (0, 100, 300), (0, 300, 1000), (0, 101, 640)])
    return cols, windows


def test_designed_records_by_hand():
    cols, windows = designed_table()
    assert len({r[1] for r in DESIGNED}) == len(DESIGNED) == len(BY_HAND)
    for q in (Q, 0):
        fast, slow = xc.expected_ctx(cols, 1, windows, q), xc.expected_ctx_slow(cols, 1, windows, q)
        assert fast.tobytes() == slow.tobytes()
        for k, r in enumerate(DESIGNED):
            want = dict(BY_HAND[r[1]])
            if q == 0:
                want.pop("lowq", None)
            assert {f: int(fast[k][f]) for f in xc.FIELDS if int(fast[k][f])} == want, (r, q)
        assert {f: int(fast[len(DESIGNED)][f]) for f in xc.FIELDS} == xc.class_totals(cols, q)
    assert [xc.is_clipped(t) for t in ("", "S", "H", "HH", "HS", "SH", "HSH", "MSM", "HMH", "HHS", "HHSM")] == [False, True, False, False, True, True, True, False, False, True, False]


def test_adjacent_windows_add():
    rng = np.random.default_rng(32)
    cols = xc.random_table(rng, 400, [(0, 5000), (1, 3000)], read_len=60, unmapped=3)
    for _ in range(200):
        t = int(rng.integers(0, 2))
        a = int(rng.integers(0, 3000))
        b = a + int(rng.integers(1, 2500))
        m = int(rng.integers(a, b + 1))
        whole, left, right = xc.expected_ctx(cols, 2, xc.as_windows([(t, a, b), (t, a, m), (t, m, b)]), 20)
        assert xc.add_rows(left, right).tobytes() == whole.tobytes(), (t, a, m, b)
    total = xc.expected_ctx(cols, 2, xc.as_windows([(0, 0, 5000), (1, 0, 3000)]), 20)
    assert {f: int(total[f].sum()) for f in xc.FIELDS} == xc.class_totals(cols, 20)


def ctx_row(**values):
    r = np.zeros(1, abi.WINDOW_CTX)[0]
    for f, v in values.items():
        r[f] = v
    return r


def test_column_formatting():
    assert xc.COLUMNS[:3] == ["Cx_Reads1", "Cx_MeanMQ1", "Cx_MQ01"] and xc.COLUMNS[9] == "Cx_Reads2" and xc.COLUMNS[-1] == "Cx_SecSup2" and len(xc.COLUMNS) == 18
    # no read: the five ratios are dots, the counts stay
    assert xc.side_columns(ctx_row(orphan=0, dup=4, secsup=2)) == ["0", ".", ".", ".", ".", ".", "0", "4", "2"]
    # thirds, and a share of 0.0005 (1 in 2000): printf's rounding of the quotient of two doubles
    assert xc.side_columns(ctx_row(reads=3, mapq_sum=100, mq0=1, lowq=2, clipped=3, improper=0, orphan=1)) == ["3", "33.3", "0.333", "0.667", "1.000", "0.000", "1", "0", "0"]
    # 1 / 2000 and 3 / 2000 are doubles just above 0.0005 and 0.0015, 999 / 2000 one just below 0.4995
    assert xc.side_columns(ctx_row(reads=2000, mapq_sum=2000 * 60 - 1, mq0=1, lowq=3, clipped=999))[:5] == ["2000", "60.0", "0.001", "0.002", "0.499"]
    # 1 / 16 and 1 / 4 are exact ties: printf rounds them to the even digit
    assert xc.side_columns(ctx_row(reads=16, mq0=1, mapq_sum=4))[1:3] == ["0.2", "0.062"] and xc.side_columns(ctx_row(reads=8, mq0=1))[2] == "0.125"
    assert xc.side_columns(ctx_row(reads=4, mapq_sum=4 * 255))[1] == "255.0" and xc.side_columns(ctx_row(reads=3, mapq_sum=2))[1] == "0.7"
    pair = (ctx_row(reads=1, mapq_sum=60), ctx_row())
    assert xc.expected_columns(pair) == ["1", "60.0", "0.000", "0.000", "0.000", "0.000", "0", "0", "0", "0", ".", ".", ".", ".", ".", "0", "0", "0"]
    s = xc.add_rows(ctx_row(reads=1, mapq_sum=(1 << 40), secsup=7), ctx_row(reads=2, mapq_sum=5, secsup=1))
    assert (int(s["reads"]), int(s["mapq_sum"]), int(s["secsup"])) == (3, (1 << 40) + 5, 8)


@pytest.fixture(scope="module")
def cpu_bin():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "cpucli"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return CPU_BIN


def test_cpu_build_refuses_context(cpu_bin, tmp_path):
    bam = tmp_path / "t.bam"
    bam.write_bytes(b"")
    base = [cpu_bin, "-i", str(bam), "-o", str(tmp_path / "o"), "-n", str(tmp_path)]
    r = subprocess.run(base + ["-context"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -context needs the GPU library" in r.stderr and "Usage" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run(base + ["-context", "-ctxflank", "300", "-all", "-fast", "-coverage"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -coverage needs the GPU library" in r.stderr, r.stderr[-2000:]  # (an earlier row of the table)
    r = subprocess.run(base + ["-context", "-ctxflank", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: -context needs the GPU library" in r.stderr, r.stderr[-2000:]  # (the library row stands before the range)
    # the usage refusals stand behind the help text, in the order of the table
    for args, word in ((["-ctxflank", "100"], "Error: -ctxflank needs -context."), (["-context", "-gpus", "2"], "Error: -context cannot be combined with -gpus."),
                       (["-ctxflank", "100", "-gpus", "2"], "Error: -ctxflank needs -context."), (["-context", "-ctxflank", "0", "-gpus", "2"], "Error: -context cannot be combined with -gpus."),
                       (["-ctxflank", "100", "-covflank", "9"], "Error: -covflank needs -coverage.")):
        r = subprocess.run(base + args, capture_output=True, text=True)
        errors = [l for l in r.stderr.split("\n") if "Error" in l]
        assert r.returncode == 1 and errors == [" " + word] and "Usage" in r.stderr, (args, r.stderr[-2000:])
    assert not any(p.name.startswith("o_") for p in tmp_path.iterdir())
    r = subprocess.run([cpu_bin, "-h"], capture_output=True, text=True)
    assert "-context" in r.stderr and "-ctxflank" in r.stderr and "Error" not in r.stderr

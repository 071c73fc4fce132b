"""The std::sort replay on every size at which it changes its code path (tests/sortcases.py; tests/test_cpu_sort_edges.py proves
without a GPU that every case sits on its edge): the permutation of every call against libstdc++'s, exactly, and what the task
dispatch's job counted - its longest heap segment and the elements in heap segments - against the oracle's probe of the same keys.

Which segments count.  A heap TASK is pushed in two places (sortsvc.inc): by a partition node for a segment whose depth budget is
used up - svc_part, at the start of a task with depth 0 or for the side it would carry on with; every segment a node holds or
hands on as a node has more than FIN_MAX keys - and by the finisher, behind fin2_body, for a depth-0 sub-segment of more than
F2_HB keys (smaller ones are heapsorted in the finishing wave's own buffer and never leave).  Both go through svc_push_heap, which
does max_heap = max(.., length) and n_heap += length.  So max_heap and n_heap are the maximum and the sum over the probe's
segments of more than F2_HB keys (sortcases.expected_heaps).  A job of the resident service is not read back: there the two words
read 0xFFFFFFFF and only the permutation is checked.

Partition-node lengths (node_*): 2048 (the finisher's), 2049, 2050 (one node), and L - 1, L, L + 1 around the trips svc_part
really takes: a wave's count and place pass run TL_UNROLL * 64 = 1536 keys a trip behind the pivot, i.e. 6144 keys for the four
waves of a narrow node (lengths 6144, 6145, 6146; 12289 = two trips) and 24576 for the sixteen of a wide one (24576, 24577,
24578); 16384 / 16385 = SVC_WIDE_MIN: the last narrow and the first wide node, as a group of its own and carried down to by a
wide workgroup (node_carried_*); the swap pass takes 4 * 256 (4 * 1024) pairs a trip, which the all-equal groups (every key a
stopper on both sides, length / 2 swaps) cross at each of these lengths.

One child process per form (the switches are read once per process) and part: the edges, and the window sorts' many small calls."""
import os
import subprocess
import sys

import pytest

from tests import bigcases

pytestmark = pytest.mark.gpu
ROOT_DIR = bigcases.ROOT

CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
from breakid_amd import capi
from oracle import pyoracle
from tests import sortcases as sc

want_tasks, windows = sys.argv[1] == "tasks", sys.argv[2] == "windows"
ctx = capi.Context([("chr1", 1000)])
c = ctx.debug_sort_info()
assert (c["max_heap"], c["n_heap"]) == (0, 0), c
assert {k: c[k] for k in sc.DOCUMENTED} == sc.DOCUMENTED, c  # (a constant that moves takes the CPU cases with it: update DOCUMENTED)
assert c["cap32"] & 1 and 2 * (c["cap32"] + 1) > c["HEAP_RANKED_MAX"] and c["HEAP_BIG_MIN"] < c["cap32"] - 2 and c["cap32"] + 2 < c["HEAP_RANKED_MAX"] - 1, c
print("CONSTANTS", " ".join("%%s=%%d" %% (k, c[k]) for k in capi.Context.SORT_INFO[:11]))
calls, seen = 0, (0, 0, 0)
NOT_READ = 0xFFFFFFFF


def run(k):
    global calls
    exp = pyoracle.unit_std_sort(k.key, k.off)
    segs = sorted(pyoracle.unit_sort_shape(k.key, k.off))
    if k.claims is not None:
        assert segs == k.claims, ("the case is not on its edge at this build's constants", k.name, segs[:4], k.claims[:4])
    got = ctx.debug_std_sort(k.key, k.off)
    calls += 1
    info = ctx.debug_sort_info()
    heaps = (info["max_heap"], info["n_heap"])
    if not k.name.startswith("win_") or heaps not in ((0, 0), (NOT_READ, NOT_READ)):
        print("CASE %%s n=%%d groups=%%d segments=%%d longest=%%d device max_heap=%%d n_heap=%%d" %% (k.name, len(k.key), len(k.off) - 1, len(segs), max([m for _, m in segs] + [0]), heaps[0], heaps[1]))
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (k.name, len(bad), int(bad[0]), segs[:4])
    assert np.array_equal(got, exp), k.name
    global seen
    forms = ctx.sort_forms()
    assert forms[0] + forms[1] == calls and forms[2] == 0, forms
    as_task = forms[1] == seen[1] + 1
    seen = forms
    if want_tasks:
        assert forms == (0, calls, 0), forms
    if as_task:
        assert heaps == sc.expected_heaps(segs, c), (k.name, heaps, sc.expected_heaps(segs, c))
    else:
        assert heaps == (NOT_READ, NOT_READ), (k.name, heaps, forms)
    return got


cases = sc.cases(c, ("win",) if windows else tuple(f for f, _ in sc.FAMILIES if f != "win"))
for k in cases:
    run(k)
# the hybrid heap and the global heapsort three times over in one process: the same bytes every time
by = {k.name: k for k in cases}
for name in () if windows else ("heap_%%d" %% (c["cap32"] + 1), "heap_%%d" %% (c["HEAP_RANKED_MAX"] + 1), "fill_two_%%d" %% (c["cap32"] + 1), "fill_equal_%%d" %% (c["HEAP_RANKED_MAX"] + 1)):
    first = run(by[name]).tobytes()
    for rep in range(2):
        assert run(by[name]).tobytes() == first, (name, rep)
forms = ctx.sort_forms()
print("FORMS", *forms)
print("CALLS", calls)
ctx.close()
print("SE_OK")
""" % ROOT_DIR


def _child(form, part, **env_extra):
    env = dict(os.environ, **env_extra)
    if form == "tasks":
        # (test_gpu_sort_tasks._run's environment: four hardware queues, the switches unset but for the one that picks the form)
        env["GPU_MAX_HW_QUEUES"] = "4"
        for k in ("BREAKID_QUIET", "BREAKID_GROUP_LANES", "BK_DEBUG"):
            env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD, form, part], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT_DIR)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "SE_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    forms = [int(v) for v in r.stdout.split("FORMS", 1)[1].split()[:3]]
    calls = int(r.stdout.split("CALLS", 1)[1].split()[0])
    assert calls >= {"edges": 130, "windows": 250}[part], calls  # (every case was a call)
    return forms, calls


PARTS = ("edges", "windows")  # the window sorts' many small calls in a child of their own


@pytest.mark.parametrize("part", PARTS)
def test_every_edge_as_task_dispatches(part):
    """BREAKID_SORT_SERVICE=0: every call is one task dispatch (sort_forms() == (0, calls, 0), asserted after every call), and
    max_heap / n_heap of every call are what the probe says."""
    forms, calls = _child("tasks", part, BREAKID_SORT_SERVICE="0")
    assert forms == [0, calls, 0], (forms, calls)


@pytest.mark.parametrize("part", PARTS)
def test_every_edge_in_the_default_form(part):
    """The environment untouched: whichever form the context picks (printed), the same permutations; the job's statistics wherever
    that form reads them back."""
    forms, calls = _child("default", part)
    print("default form: %d jobs of the resident service, %d task dispatches" % (forms[0], forms[1]))
    assert forms[0] + forms[1] == calls and forms[2] == 0, (forms, calls)

"""Per sort of the task-dispatch form (sortsvc.inc, k_sort_job): how long after the dispatch started the sort's longest heap
started, how long it took, and when the partition and finisher tasks and the whole job were done.  A task dispatch is one
kernel, so a kernel trace cannot tell: the times come from the workgroups' own clocks, which the driver prints per sort under
BK_DEBUG=svc.

    BK_DEBUG=lanes,svc python bench.py --steps 1 --warmup 1 --cpu-sample 0 2> run.err
    python tools/task_dispatch_heap_waits.py run.err
"""
import re
import sys

LINE = re.compile(r"\[svc\] task dispatch (\d+): (\d+) elements in (\d+) groups on (\d+) wide \+ (\d+) narrow workgroups; longest heap (\d+) "
                  r"elements started ([\d.]+) ms after the dispatch and took ([\d.]+) ms; partitions and finisher done after ([\d.]+) ms, "
                  r"job after ([\d.]+) ms")


def main(path):
    rows = [m for m in map(LINE.search, open(path, errors="replace")) if m]
    if not rows:
        print("no '[svc] task dispatch' lines in %s (run with BK_DEBUG=svc)" % path)
        return 1
    print("%6s %10s %6s %10s %12s %10s %12s %10s %12s" % ("sort", "elements", "groups", "heap", "heap start", "heap ms", "parts done", "job ms",
                                                        "after heap"))
    waits = []
    for m in rows:
        sort, n, ng, _, _, heap = (int(m.group(k)) for k in range(1, 7))
        start, took, parts, job = (float(m.group(k)) for k in range(7, 11))
        # what the job took beyond its longest heap: the part of the sort that is not the inherently serial pops
        tail = job - (start + took) if heap else job
        waits.append(start)
        print("%6d %10d %6d %10d %9.3f ms %10.3f %9.3f ms %10.3f %9.3f ms" % (sort, n, ng, heap, start, took, parts, job, tail))
    waits.sort()
    print("%d sorts; longest heap started after the dispatch: median %.3f ms, max %.3f ms" % (len(waits), waits[len(waits) // 2], waits[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))

"""Offline reading of tools/gpu_timeline.sh's kernel timeline (bench --steps 2 --warmup 1): in the last timed step, dispatches per
hardware queue and, for every long heap kernel (k_se_heapsort<2> or k_se_heaps_fused with its big heaps), the dispatch that starts
next on the same queue and how long after the heap ended.  A start right at the heap's end (0 us) is a dispatch that was queued
behind the heap.
Usage: python tools/timeline_heap_waits.py TRACE [--write-step OUT.csv]
  TRACE  the script's kernel_trace_product.csv.gz (whole run), or a step file this tool wrote (name, queue, start_us, end_us)
  --write-step  also write the last timed step as such a plain CSV (times in us from the step's k_stream)"""
import collections
import csv
import gzip
import sys

if len(sys.argv) < 2 or sys.argv[1].startswith("--"):
    sys.exit(__doc__)
fn = sys.argv[1]
if fn.endswith(".gz"):
    rows = [(r["name"].replace("void ", ""), int(r["queue"]), int(r["start"]), int(r["end"])) for r in csv.DictReader(gzip.open(fn, "rt"))]
    rows.sort(key=lambda r: r[2])
    ks = [r[2] for r in rows if r[0] == "k_stream"]
    t0 = ks[2]  # warm-up step, first timed step, last timed step (the from-bam side measurement comes after)
    t1 = min([t for t in ks if t > t0] + [t0 + int(200e6)])
    step = [(r[0], r[1], r[2] - t0, r[3] - t0) for r in rows if t0 <= r[2] < t1]
else:
    step = [(r["name"], int(r["queue"]), int(round(float(r["start_us"]) * 1e3)), int(round(float(r["end_us"]) * 1e3))) for r in csv.DictReader(open(fn))]
    step.sort(key=lambda r: r[2])
if "--write-step" in sys.argv:
    with open(sys.argv[sys.argv.index("--write-step") + 1], "w") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["name", "queue", "start_us", "end_us"])
        for r in step:
            w.writerow([r[0], r[1], "%.1f" % (r[2] / 1e3), "%.1f" % (r[3] / 1e3)])
print("last timed step: %d dispatches in %.1f ms; per queue: %s" % (len(step), max(r[3] for r in step) / 1e6, dict(sorted(collections.Counter(r[1] for r in step).items()))))
for b in step:
    if "heapsort<2>" not in b[0] and "heaps_fused" not in b[0]:
        continue
    nxt = [r for r in step if r[1] == b[1] and r[2] >= b[3] - 1000][:1]
    print("%8.3f ms  %-24s %6.2f ms on queue %d -> next there: %-34s after %8.1f us" % (b[2] / 1e6, b[0][:24], (b[3] - b[2]) / 1e6, b[1], nxt[0][0][:34] if nxt else "-", (nxt[0][2] - b[3]) / 1e3 if nxt else 0.0))

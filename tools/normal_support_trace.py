"""Reduce a rocprofv3 kernel trace of tools/gpu_normal_cost.py to the kernels of each bk_normal_support call (from its
k_keys_numeric to its k_normal_depth): per call the device span, and per kernel the dispatches and summed time.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o prof -- python tools/gpu_normal_cost.py --reps 3
    python tools/normal_support_trace.py DIR/prof_kernel_trace.csv > profiles/r07_normal_support_kernels_620M.csv"""
import collections
import csv
import re
import sys


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    out = csv.writer(sys.stdout)
    out.writerow(["call", "kernel", "dispatches", "ms", "call_span_ms"])
    call, cur = 0, None
    for r in rows:
        name = r["Kernel_Name"]
        if "k_keys_numeric" in name or "k_keys_pos" in name:
            cur = [int(r["Start_Timestamp"]), collections.OrderedDict()]
        if cur is None:
            continue
        m = re.search(r"(k_\w+)", name)
        k = m.group(1) if m else name[:40]
        a = cur[1].setdefault(k, [0, 0.0])
        a[0] += 1
        a[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "k_normal_depth" in name:
            span = (int(r["End_Timestamp"]) - cur[0]) / 1e6
            for k, (n, ms) in cur[1].items():
                out.writerow([call, k, n, "%.4f" % ms, "%.4f" % span])
            call, cur = call + 1, None


if __name__ == "__main__":
    main(sys.argv[1])

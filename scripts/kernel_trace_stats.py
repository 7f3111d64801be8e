"""Per-kernel launch statistics of a `rocprofv3 --kernel-trace` output directory (rocpd / SQLite): calls, total, mean and the
launch-to-launch standard deviation, which the `top_kernels` summary of --stats does not carry.

usage: python scripts/kernel_trace_stats.py <trace_dir> <out.csv> [substring of a kernel name to print]"""
import collections
import csv
import glob
import os
import sqlite3
import statistics
import sys


def durations(trace_dir):
    per = collections.defaultdict(list)
    for f in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):
        cur = sqlite3.connect(f).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            per[name].append((end - start) / 1000.0)
    return per


def main():
    trace_dir, out_csv = sys.argv[1], sys.argv[2]
    show = sys.argv[3] if len(sys.argv) > 3 else None
    per = durations(trace_dir)
    total = sum(sum(v) for v in per.values()) or 1.0
    rows = sorted(per.items(), key=lambda kv: -sum(kv[1]))
    with open(out_csv, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["Name", "Calls", "TotalDurationUs", "AverageUs", "Percentage", "StdDevUs"])
        for name, v in rows:
            sd = statistics.stdev(v) if len(v) > 1 else 0.0
            w.writerow([name, len(v), round(sum(v), 3), round(sum(v) / len(v), 3), 100.0 * sum(v) / total, round(sd, 3)])
            if show and show in name:
                print("%s: calls %d mean %.2f us sigma %.2f min %.2f max %.2f" % (show, len(v), sum(v) / len(v), sd, min(v), max(v)))


if __name__ == "__main__":
    main()

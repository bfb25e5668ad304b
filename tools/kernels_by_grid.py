"""Folds a rocprofv3 kernel_trace.csv by (kernel, grid): launches, mean / median / min duration in us and the workgroup count.
python tools/kernels_by_grid.py <kernel_trace.csv> [substring ...]     (only kernels whose name contains one of the substrings)
The group launches of a bench step and the solo clones of its other legs run the same symbols at different grids: this keeps them apart."""
import csv, re, sys
from collections import defaultdict
rows = list(csv.DictReader(open(sys.argv[1])))
want = sys.argv[2:]
by = defaultdict(list)
for r in rows:
    name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void sc::", "").replace("sc::", "")
    if want and not any(w in name for w in want):
        continue
    wg = int(r["Grid_Size_X"]) // max(int(r.get("Workgroup_Size_X", "1") or 1), 1)
    by[(name, wg)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("%-72s %8s %7s %9s %9s %9s" % ("kernel", "wgs", "n", "mean_us", "median_us", "min_us"))
for (name, wg), d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    d.sort()
    print("%-72s %8d %7d %9.2f %9.2f %9.2f" % (name[:72], wg, len(d), sum(d) / len(d), d[len(d) // 2], d[0]))

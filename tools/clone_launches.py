"""The ordered (kernel, workgroup count) list of one steady-state clone, from a kernel trace of tools/solo_trace.py:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/solo_trace.py 2048 6;  python tools/clone_launches.py DIR
The launches in dispatch order; the clone is the shortest tail of that list that repeats the launches in front of it.  Two builds
enqueue the same launches exactly when their lists are equal (profiles/solo_trace_schedule*.txt)."""
import csv, glob, re, sys
path = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[0]
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
def wgs(r):
    n = 1
    for a in "XYZ":
        n *= max(1, int(r["Grid_Size_" + a]) // max(int(r["Workgroup_Size_" + a] or 1), 1))
    return n
seq = [(re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void sc::", "").replace("sc::", ""), wgs(r)) for r in rows]
for K in range(5, len(seq) // 2):
    if seq[-K:] == seq[-2 * K:-K]:
        break
else:
    sys.exit("no repeating tail in %d launches" % len(seq))
print("# %d launches per clone (of %d in the trace)" % (K, len(seq)))
for name, n in seq[-K:]:
    print(name, n)

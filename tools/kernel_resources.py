"""The compiler's kernel-resource-usage remarks of HIP sources, one sorted line per kernel instantiation (the format of
profiles/cycle0_resources_*.txt): python tools/kernel_resources.py [--root <tree>] sc_cycle0.hip sc_sweep_tb.hip > out.txt
Compiles the device side only, with the Makefile's flags; nothing is linked or written.
--code-size (anywhere on the line): also each kernel's size in bytes of machine code ("code N" at the end of its line), read from the symbol table of the
device object, which is then compiled into a temporary file."""
import os, re, subprocess, sys, tempfile
args = sys.argv[1:]
code_size = "--code-size" in args
args = [a for a in args if a != "--code-size"]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    i = args.index("--root")
    root, args = os.path.abspath(args[i + 1]), args[:i] + args[i + 2:]
csrc = os.path.join(root, "seamlesscloneoptimization_amd", "csrc")
FLAGS = "-O3 -std=c++17 -fPIC -pthread --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fvisibility=hidden".split()
NAMES = {"k_cycle0": ("T", "NW", "R", "PRO", "GEN", "ZEROIN", "TAG"), "k_rb_tb": ("T", "NW", "R", "SOR", "GEN", "FLAGS", "HXQ"),
         "k_jacobi_tb": ("T", "NW", "R", "TAG", "HXQ")}
KEYS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
        ("Occupancy [waves/SIMD]", "occupancy"))
lines = []
sizes = {}
for src in args:
    obj = tempfile.NamedTemporaryFile(suffix=".o") if code_size else None
    err = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj.name if obj else os.devnull] + (["--no-gpu-bundle-output"] if obj else []),
                         cwd=csrc, capture_output=True, text=True, check=True).stderr
    if obj:
        for l in subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-sW", obj.name], capture_output=True, text=True, check=True).stdout.splitlines():
            f = l.split()
            if len(f) == 8 and f[3] == "FUNC":
                sizes[f[7]] = int(f[2], 0)
        obj.close()
    cur = None
    for l in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", l)
        if m:
            cur = {"name": m.group(1)}
            lines.append(cur)
            continue
        m = re.search(r"remark:\s+(?:[^:]*:\d+:\d+:\s+)?([A-Za-z][^:]*): (\S+)", l)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
names = subprocess.run(["c++filt"], input="\n".join(c["name"] for c in lines), capture_output=True, text=True, check=True).stdout.splitlines()
out = []
for c, n in zip(lines, names):
    n = n.replace("(anonymous namespace)::", "")
    m = re.match(r"(?:void )?(?:sc::)?(\w+)<(.*)>\(", n)
    if m and m.group(1) in NAMES:
        vals = [{"false": "0", "true": "1"}.get(v.strip(), v.strip()) for v in m.group(2).split(",")]
        n = "%s<%s>" % (m.group(1), ",".join("%s=%s" % kv for kv in zip(NAMES[m.group(1)], vals)))
    else:
        n = re.sub(r"\(.*", "", n).replace("void ", "").replace("sc::", "")
    out.append(n + " " + " ".join("%s %s" % (short, c.get(k, "?")) for k, short in KEYS) + " spill %s %s" % (c.get("SGPRs Spill", "?"), c.get("VGPRs Spill", "?"))
               + (" code %s" % sizes.get(c["name"], "?") if code_size else ""))
print("\n".join(sorted(out)))

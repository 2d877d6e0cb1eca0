"""Compares the device instruction streams of one HIP source in two trees, kernel by kernel:

    python tools/kernel_isa_diff.py <tree A> <tree B> sa_dense.hip [--json out.json]

Each tree's pointnet-like-pose-estimation_amd/csrc/<source> is compiled to gfx950 assembly with
the flags csrc/Makefile of that tree gives the file (make -n; --offload-device-only -S as its
ASMCHECK rule).  Per kernel symbol: "same" when the instructions are equal line by line (comments
and directives stripped, labels kept), else both instruction counts and the first differing line.
The kernel descriptor's resource numbers (next free VGPR / SGPR, accumulator offset, LDS and
scratch bytes) are compared with the instructions and printed wherever anything differs.
A kernel whose parameter list changed is paired by its name and template arguments.
Host only; it compares and searches for nothing.  Exit status 1 when any kernel differs."""
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = "pointnet-like-pose-estimation_amd/csrc"


def assembly(tree, source):
    csrc = os.path.join(os.path.abspath(tree), CSRC)
    obj = "../build/%s.o" % source
    plan = subprocess.run(["make", "-n", "-B", "-C", csrc, os.path.abspath(os.path.join(csrc, obj))],
                          capture_output=True, text=True, check=True).stdout
    cmd = next(c for c in map(shlex.split, plan.splitlines()) if "-c" in c and os.path.join(csrc, source) in c)
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    i = cmd.index("-c")
    cmd = cmd[:i] + ["--offload-device-only", "-S"] + cmd[i + 1:cmd.index("-o")] + ["-o", out]
    subprocess.run(cmd, check=True, cwd=csrc)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text


def kernels(text):
    """{symbol: [instruction and label lines]} of every .amdhsa_kernel of the assembly."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        line = re.sub(r"\s*(;|//).*$", "", line).strip()
        m = re.match(r"^(\S+):$", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line and not line.startswith("."):
            cur.append(line)
        elif cur is not None and re.match(r"^\.L\S+:$", line):
            cur.append(line)
    return out


RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
             "private_segment_fixed_size")


def resources(text):
    """{symbol: {descriptor field: value}} from the .amdhsa_kernel blocks."""
    out = {}
    for sym, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        out[sym] = {k: int(v, 0) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\w+)", body) if k in RESOURCES}
    return out


def main():
    a, b, source = sys.argv[1:4]
    with ThreadPoolExecutor(2) as ex:  # the two compilations side by side
        ta, tb = ex.map(lambda tree: assembly(tree, source), (a, b))
    ka, kb, ra, rb = kernels(ta), kernels(tb), resources(ta), resources(tb)

    def demangled(syms):
        return subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")

    names = demangled(sorted(ka))
    by_name = {n.split("(")[0]: s for s, n in zip(sorted(kb), demangled(sorted(kb)))}
    report, diff, paired = {}, 0, set()
    for sym, name in zip(sorted(ka), names):
        if sym not in kb and name.split("(")[0] in by_name:  # same kernel, other parameters
            sb = by_name[name.split("(")[0]]
            kb[sym], rb[sym] = kb[sb], rb[sb]
            paired.add(sb)
        x, y = ka[sym], kb.get(sym)
        if y is None:
            report[name] = "missing in B"
        elif x == y and ra[sym] == rb[sym]:
            report[name] = "same (%d)" % len(x)
        else:
            i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            report[name] = "DIFF %d vs %d, first at %d: %r | %r; resources %s | %s" % (
                len(x), len(y), i, "".join(x[i:i + 1]), "".join(y[i:i + 1]), ra[sym], rb[sym])
        diff += report[name][:4] != "same"
        print("%-100s %s" % (name[:100] if report[name][:4] == "same" else name, report[name]))
    for sym in sorted(set(kb) - set(ka) - paired):
        diff += 1
        report[sym] = "only in B"
        print("%s only in B" % sym)
    print("%s: %d kernels, %d differ" % (source, len(ka), diff))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump({"source": source, "kernels": len(ka), "differ": diff, "report": report}, f, indent=1)
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()

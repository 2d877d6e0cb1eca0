"""Compares the device instruction streams of one HIP source in two trees, kernel by kernel:

    python tools/kernel_isa_diff.py <tree A> <tree B> sa_dense.hip [--json out.json]

Each tree's pointnet-like-pose-estimation_amd/csrc/<source> is compiled to gfx950 assembly with
the flags csrc/Makefile of that tree gives the file (make -n; --offload-device-only -S as its
ASMCHECK rule).  Per kernel symbol: "same" when the instructions are equal line by line (comments
and directives stripped, labels kept), else both instruction counts and the first differing line.
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


def main():
    a, b, source = sys.argv[1:4]
    with ThreadPoolExecutor(2) as ex:  # the two compilations side by side
        ka, kb = (kernels(t) for t in ex.map(lambda tree: assembly(tree, source), (a, b)))
    names = subprocess.run(["c++filt"], input="\n".join(sorted(ka)), capture_output=True, text=True).stdout.split("\n")
    report, diff = {}, 0
    for sym, name in zip(sorted(ka), names):
        x, y = ka[sym], kb.get(sym)
        if y is None:
            report[name] = "missing in B"
        elif x == y:
            report[name] = "same (%d)" % len(x)
        else:
            i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            report[name] = "DIFF %d vs %d, first at %d: %r | %r" % (len(x), len(y), i, "".join(x[i:i + 1]), "".join(y[i:i + 1]))
        diff += report[name][:4] != "same"
        print("%-100s %s" % (name[:100], report[name]))
    for sym in sorted(set(kb) - set(ka)):
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

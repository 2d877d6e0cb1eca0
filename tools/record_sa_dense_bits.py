"""Records the bits of the dense SA layer kernels (csrc/sa_dense.hip): a CRC32 of the raw output
bytes of every case of tests/test_gpu_dense_bits.py::golden_cases (register-staged, LDS-staged and
fused-pair launches, every pool mode, fp32 and bf16; inputs and weights from fixed seeds).
tests/test_gpu_dense_bits.py::test_bits_are_the_recorded_ones recomputes and compares them.

tests/golden/sa_dense_bits.json was produced with the kernels of commit 98bca14 ("FC heads under
autograd: one forward and one backward kernel template"), before any piece of the three dense
kernels was a shared helper.  Record again only when the arithmetic of a dense layer changes on
purpose.  Needs a ROCm device.

Routing: with --markers a tiny torch bitwise_xor launch precedes every case; run that under a
kernel trace, then `--routing <kernel_trace.csv> --out <json>` (no device needed) lists per case
the dense kernels seen and how the case's last layer pools, by the planner's rule (pool_mode is
a run-time argument: the trace's kernel names cannot show it;
profiles/sa_dense/refactor_routing.json)."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")]


def routing(trace, out):
    import test_gpu_dense_bits as T
    keys = [k for k, _, _ in T.golden_cases()]
    with open(trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    per, i = {}, -1
    for r in rows:
        name = r["Kernel_Name"]
        if "xor" in name.lower():
            i += 1
        elif i >= 0 and re.search(r"pn2::(dense_|unkey|sa_chain|chain_)", name):
            short = re.sub(r"^void |pn2::|\(.*$", "", name)
            if short not in per.setdefault(keys[i], []):
                per[keys[i]].append(short)
    assert i == len(keys) - 1, "markers %d != cases %d" % (i + 1, len(keys))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"what": "kernels of each case of tests/test_gpu_dense_bits.py (kernel trace of one recorder run)",
                   "pool": "how the case's last layer pools (test_gpu_dense_bits.py _split_pool / _lds_pool: the "
                           "planner's rule; pool_mode is a run-time argument the trace does not show)",
                   "kernels": sorted({k for v in per.values() for k in v}),
                   "pool_routes": sorted(set(T.POOL_NOTES.values())),
                   "cases": {k: {"pool": T.POOL_NOTES[k], "kernels": per.get(k, [])} for k in keys}}, f, indent=1)
        f.write("\n")
    print("record_sa_dense_bits: routing of %d cases -> %s" % (len(per), out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--markers", action="store_true")
    ap.add_argument("--routing", default=None, metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.routing:
        return routing(a.routing, a.out or os.path.join(ROOT, "profiles", "sa_dense", "refactor_routing.json"))
    import torch
    import test_gpu_dense_bits as T
    if not torch.cuda.is_available():
        sys.exit("record_sa_dense_bits: needs a ROCm device")
    mark = torch.zeros(64, dtype=torch.int32, device="cuda")
    crc = T.golden_bits((lambda: mark.bitwise_xor_(mark)) if a.markers else None)
    head = {"what": "CRC32 of the raw bytes of each case's output buffer (+ zero side job tensor); "
                    "key = case and precision (tests/test_gpu_dense_bits.py golden_cases)",
            "kernels_of_commit": "98bca14", "device": torch.cuda.get_device_name(0), "cases": len(crc)}
    out = a.out or T.GOLDEN
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:  # a case per line
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in head.items()))
        f.write(' "crc32": {\n' + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in crc.items()))
        f.write("\n }\n}\n")
    print("record_sa_dense_bits: %d cases -> %s" % (len(crc), out))


if __name__ == "__main__":
    main()

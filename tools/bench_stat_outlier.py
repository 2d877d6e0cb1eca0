"""pn2.collect.delet_outlier_statistical timed at the reference's defaults (nb_neighbors = 120,
std_ratio = 0.1) on tools/bench_collect.py's synthetic frame:

  frame      the 640 x 480 float64 frame after clip_distance
  N30000     one 30000-point float64 cloud (the same scene at the same density)
  N30000_f32 the same cloud as float32

Per case: the k-NN entry alone (pn2_knn_mean_dist_f64: ms and pairs per second), the statistics
launch alone (pn2_stat_outlier_flags), the whole call on a device tensor and from and to host
arrays, and pn2_radius_count_f64 on the same cloud in the same run, with the ratio of the two
pair rates and the statistics launch's share of the device call.

bench_common's method: HIP events around `reps` back-to-back calls, `rounds` rounds after `warmup`
calls, the median of the rounds with min and max.  Open3D is not a dependency, so the only host
baseline is the numpy restatement tests/stat_outlier_ref.py at 30000 points (wall clock, one
call), named as such.  Needs a ROCm device.  Writes one JSON document (default
profiles/stat_outlier/timing.json)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]
import stat_outlier_ref  # noqa: E402
from bench_collect import FULL, frame, rounds_of  # noqa: E402
from pn2 import collect  # noqa: E402

K, RATIO = 120, 0.1


def gpu_case(pc, a):
    dev = torch.from_numpy(pc).cuda()
    N = len(pc)
    out = {"N": N, "dtype": str(pc.dtype)}
    mean = collect._knn_mean(dev, K)
    out["rows_kept"] = len(collect.delet_outlier_statistical(dev, K, RATIO))
    out["knn_kernel"] = rounds_of(lambda: collect._knn_mean(dev, K), a, 1)
    out["knn_kernel"]["pairs_per_s"] = round(N * N / (out["knn_kernel"]["median"] * 1e-3), -6)
    out["stats_launch"] = rounds_of(lambda: collect._stat_flags(mean, RATIO), a, a.reps)
    out["call_device"] = rounds_of(lambda: collect.delet_outlier_statistical(dev, K, RATIO), a, 1)
    out["call_host"] = rounds_of(lambda: collect.delet_outlier_statistical(pc, K, RATIO), a, 1)
    out["radius_count_kernel"] = rounds_of(lambda: collect._counts(dev, 0.05), a, 1)
    out["radius_count_kernel"]["pairs_per_s"] = round(N * N / (out["radius_count_kernel"]["median"] * 1e-3), -6)
    out["knn_over_count_pair_rate"] = round(out["knn_kernel"]["pairs_per_s"]
                                            / out["radius_count_kernel"]["pairs_per_s"], 3)
    out["stats_share_of_call_device"] = round(out["stats_launch"]["median"] / out["call_device"]["median"], 3)
    return out


def host_baseline(pc):
    t0 = time.perf_counter()
    kept = stat_outlier_ref.delet_outlier_statistical(pc, K, RATIO)
    return {"what": "the numpy restatement tests/stat_outlier_ref.py (brute force over 256-row slabs, a full sort "
                    "per row), wall clock of one call; Open3D is not importable here",
            "N": len(pc), "rows_kept": len(kept), "call_ms": round((time.perf_counter() - t0) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", type=int, default=30000)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline (about a minute)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stat_outlier", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stat_outlier: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "unit": "ms per call", "nb_neighbors": K, "std_ratio": RATIO, "C": 6, "gpu": {}}
    clipped = collect.clip_distance(frame(FULL))
    small = frame(a.small)
    doc["gpu"]["frame"] = gpu_case(clipped, a)
    doc["gpu"]["N%d" % a.small] = gpu_case(small, a)
    doc["gpu"]["N%d_f32" % a.small] = gpu_case(small.astype("float32"), a)
    if not a.no_host:
        doc["host_baseline"] = host_baseline(small)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

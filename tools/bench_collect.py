"""The camera-cloud front end (pn2.collect) timed on a synthetic frame: a plane of clutter, three
dense objects and sparse stray points, seeded, float64, at N = 30000 and N = 307200 (640 x 480).
The scene keeps its point density at every N, so the reference's defaults (clip [0, 2],
nb_points = 200 within 0.05, eps = 0.03 with min_points = 500) select the same things.

  clip / radius_filter / cluster_point   each function alone, host array in, host array out
  chain                                  clip -> filter -> cluster_point on device tensors
  pair_kernel                            pn2_radius_count_f64 alone: ms and pairs per second

bench_common's method: HIP events around `reps` back-to-back calls, `rounds` rounds after `warmup`
calls, the median of the rounds with min and max.  The host baseline is Open3D where it is
importable; where it is not, the numpy brute force of tests/collect_ref.py for the clip and the
radius filter at N = 30000 only (wall clock, one call), and the document says which.
Needs a ROCm device.  Writes one JSON document (default profiles/collect/timing.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]
import collect_ref  # noqa: E402
from bench_common import summary, timed  # noqa: E402
from pn2 import collect  # noqa: E402

FULL = 307200


def frame(N, seed=0):
    """60 % plane at z = 1, three filled balls of 10 % each above it, 10 % strays (a part of
    them outside the clip range); lengths scaled so that the density is that of the full frame."""
    rng = np.random.RandomState(seed)
    s2, s3 = (N / FULL) ** 0.5, (N / FULL) ** (1.0 / 3.0)
    n_ball = N // 10
    n_stray = N // 10
    n_plane = N - 3 * n_ball - n_stray
    plane = np.stack([rng.uniform(-0.5, 0.5, n_plane) * s2, rng.uniform(-0.375, 0.375, n_plane) * s2,
                      1.0 + rng.normal(0, 0.001, n_plane)], 1)
    balls = []
    for k in range(3):
        v = rng.normal(size=(n_ball, 3))
        v *= (0.06 * s3 * rng.uniform(0, 1, (n_ball, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
        balls.append(v + [(k - 1) * 0.3 * s2, 0.0, 0.7])
    stray = rng.uniform([-1, -1, -0.5], [1, 1, 3.0], (n_stray, 3))
    xyz = np.vstack([plane] + balls + [stray])[rng.permutation(N)]
    return np.hstack([xyz, rng.uniform(0, 1, (N, 3))])  # xyz + colour, as the camera delivers


def rounds_of(fn, a, reps):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    return summary([timed(fn, reps) for _ in range(a.rounds)])


def gpu_case(pc, a):
    dev = torch.from_numpy(pc).cuda()
    N = len(pc)
    out = {"N": N}
    out["clip"] = rounds_of(lambda: collect.clip_distance(pc), a, a.reps)
    out["radius_filter"] = rounds_of(lambda: collect.delet_outlier_radius(pc), a, 1)
    out["pair_kernel"] = rounds_of(lambda: collect._counts(dev, 0.05), a, 1)
    out["pair_kernel"]["pairs_per_s"] = round(N * N / (out["pair_kernel"]["median"] * 1e-3), -6)
    clipped = collect.clip_distance(dev)
    kept = collect.delet_outlier_radius(clipped)
    out["rows_after_clip"], out["rows_after_filter"] = len(clipped), len(kept)
    np.random.seed(0)
    clusters = collect.cluster_point(kept)
    out["clusters"] = None if clusters is None else list(clusters.shape)

    def cluster():
        np.random.seed(0)
        collect.cluster_point(kept)

    def chain():
        np.random.seed(0)
        collect.cluster_point(collect.delet_outlier_radius(collect.clip_distance(dev)))

    out["dbscan_labels"] = rounds_of(lambda: collect._labels(kept, 0.03, 500), a, 1)
    out["cluster_point"] = rounds_of(cluster, a, 1)
    out["chain"] = rounds_of(chain, a, 1)
    return out


def host_baseline(pc):
    try:
        import open3d
    except ImportError:
        open3d = None
    out = {}
    if open3d is not None:
        out["what"] = "Open3D %s on the host (kd-tree), wall clock of one call" % open3d.__version__
        pcd = open3d.geometry.PointCloud()
        pcd.points = open3d.utility.Vector3dVector(pc[:, :3])
        t0 = time.perf_counter()
        pcd.remove_radius_outlier(200, 0.05)
        out["radius_filter_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        pcd.cluster_dbscan(eps=0.03, min_points=500)
        out["dbscan_labels_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    else:
        out["what"] = ("Open3D is not importable here: the numpy brute force of tests/collect_ref.py "
                       "(rule 2 over 500-row slabs), wall clock of one call")
        t0 = time.perf_counter()
        counts = np.concatenate([collect_ref.neighbour_matrix(pc, 0.05, slice(r, r + 500)).sum(1)
                                 for r in range(0, len(pc), 500)])
        pc[counts > 200]
        out["radius_filter_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    collect_ref.clip_distance(pc)
    out["clip_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["N"] = len(pc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[30000, FULL])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_collect: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "unit": "ms per call", "dtype": "float64", "C": 6, "gpu": {}}
    for N in a.sizes:
        doc["gpu"]["N%d" % N] = gpu_case(frame(N), a)
    doc["host_baseline"] = host_baseline(frame(min(a.sizes)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

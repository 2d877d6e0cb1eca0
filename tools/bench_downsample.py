"""Farthest-point downsampling of raw clouds to 1024 points (pn2.provider.farthest_point_sample /
farthest_point_sample_batch, csrc/fps_points.hip) against the numpy loop it replaces, at the sizes
of the reference's data path: the synthesised shapes and ModelNet's --use_uniform_sample
(N = 10000 and 30000, float64 C = 3 and float32 C = 6, one cloud and a batch of 64) and one
camera-sized cloud (N = 300000).

  numpy_ms      the reference's loop restated (tests/downsample_ref.py), one cloud, host clock
  gpu_host_ms   farthest_point_sample(cloud) from and to host arrays: staging, H2D, the kernel,
                D2H; host clock (the call ends with the copy back)
  gpu_ms        farthest_point_sample_batch on a device-resident [B, N, C] tensor, by HIP events
                over `reps` back-to-back calls after warm-up: the whole Python call (output and
                workspace allocation, the pinned table and its copy, the kernel)
  kernel_ms     the C entry pn2_fps_points alone, buffers and table prepared beforehand, by HIP
                events over `reps` back-to-back calls: the kernel
  per_iter_us   kernel_ms / number: one iteration of the serial loop (all B clouds side by side)
  ratio         numpy_ms * B / gpu_ms: the numpy loop runs the clouds one after another

Each figure is the median of `rounds` rounds; the spread (min, max of the rounds) is recorded
beside it.  The first cloud of every row is checked against the numpy loop, bit for bit.
Needs a ROCm device: there is no CPU fallback.
Writes one JSON document (default profiles/downsample/timing.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"), os.path.join(ROOT, "tests")]
import downsample_ref  # noqa: E402
from pn2 import _lib  # noqa: E402
from pn2.provider import farthest_point_sample, farthest_point_sample_batch  # noqa: E402

# (label, N, C, dtype, batch sizes)
SIZES = [
    ("shape_10k_f64", 10000, 3, np.float64, (1, 64)),
    ("shape_30k_f64", 30000, 3, np.float64, (1, 64)),
    ("modelnet_10k_f32", 10000, 6, np.float32, (1, 64)),
    ("camera_300k_f64", 300000, 3, np.float64, (1,)),
]


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--number", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--numpy-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downsample", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_downsample: needs a ROCm device")
    L = _lib.load()
    rows = []
    for label, N, C, dtype, batches in SIZES:
        rs = np.random.RandomState(N + C)
        clouds = rs.uniform(-1.0, 1.0, (max(batches), N, C)).astype(dtype)
        starts = rs.randint(0, N, max(batches))
        code = _lib.DTYPE_F64 if dtype == np.float64 else _lib.DTYPE_F32
        path = "lds" if L.pn2_fps_points_workspace_bytes(code, N, N) == 0 else "workspace"
        numpy_ms = []
        for _ in range(a.numpy_rounds):
            t0 = time.perf_counter()
            want = downsample_ref.sample_indices(clouds[0], a.number, starts[0])
            numpy_ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = []
        for r in range(a.rounds + 1):  # the first call is the warm-up
            np.random.seed(r)
            t0 = time.perf_counter()
            farthest_point_sample(clouds[0], a.number)
            if r:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        for B in batches:
            dev = torch.from_numpy(clouds[:B]).cuda()
            out, idx = farthest_point_sample_batch(dev, a.number, starts=starts[:B], return_index=True)
            np.testing.assert_array_equal(idx[0].cpu().numpy(), want)
            np.testing.assert_array_equal(out[0].cpu().numpy(), clouds[0][want])
            gpu_ms = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    farthest_point_sample_batch(dev, a.number, starts=starts[:B])
                e1.record()
                torch.cuda.synchronize()
                gpu_ms.append(e0.elapsed_time(e1) / a.reps)
            # the C entry alone, every buffer allocated and the table copied beforehand
            table = torch.from_numpy(np.concatenate([np.arange(B + 1, dtype=np.int64) * N,
                                                     starts[:B].astype(np.int64)])).cuda()
            k_idx = torch.empty(B, a.number, dtype=torch.int64, device="cuda")
            k_out = torch.empty(B, a.number, C, dtype=dev.dtype, device="cuda")
            need = L.pn2_fps_points_workspace_bytes(code, B * N, N)
            ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
            stream = _lib.stream_ptr(dev.device)

            def entry():
                _lib.check(L.pn2_fps_points(dev.data_ptr(), code, B, table.data_ptr(), table.data_ptr() + 8 * (B + 1),
                                            B * N, N, C, C, a.number, k_idx.data_ptr(), k_out.data_ptr(),
                                            ws.data_ptr() if need else 0, need, stream), "pn2_fps_points")
            entry()
            torch.cuda.synchronize()
            assert torch.equal(k_idx, idx) and torch.equal(k_out, out)
            kernel_ms = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    entry()
                e1.record()
                torch.cuda.synchronize()
                kernel_ms.append(e0.elapsed_time(e1) / a.reps)
            g, k = statistics.median(gpu_ms), statistics.median(kernel_ms)
            row = {"case": label, "N": N, "C": C, "dtype": np.dtype(dtype).name, "B": B, "number": a.number,
                   "distances": path, "numpy_ms": summary(numpy_ms), "gpu_host_ms": summary(host_ms),
                   "gpu_ms": summary(gpu_ms), "kernel_ms": summary(kernel_ms),
                   "per_iter_us": round(k / a.number * 1e3, 3),
                   "ratio": round(statistics.median(numpy_ms) * B / g, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "numpy_rounds": a.numpy_rounds, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

"""The three matrix products of a shared-MLP layer's training step: the library calls of
pn2/train._MlpMaxTrain (tuning train_gemm=0: torch.addmm, torch.mm, train._grad_weight's chunked
bmm + sum) against pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32 (train_gemm=1), on
identical inputs.

Shapes: the nine layers of H.ClsSSG at B clouds (default 32) of 1024 points:
  sa1  M = B*512*32  3 -> 64 -> 64 -> 128
  sa2  M = B*128*64  131 -> 128 -> 128 -> 256
  sa3  M = B*128     259 -> 256 -> 512 -> 1024
and per layer the products  forward Y = X W^T + b,  dx = dY W,  dw = dY^T X.

ms: HIP-event time per call over `reps` back-to-back calls after `warmup` calls; the two routes
run interleaved within each of `rounds` rounds; the median of the rounds with their min and max.
ratio = library median / kernel median (> 1: the kernel is faster).  max_rel_diff: the largest
|library - kernel| over the largest |library| (both are float32 GEMMs of the same operands).
step: the whole ClsSSG train step (forward + backward + SGD step, tools/bench_train.py's method:
wall clock over 20 steps after 3, synchronised) at train_gemm=0 and at train_gemm=1, interleaved
over `rounds` rounds; at key 0 this is the library route, unchanged.
Needs a ROCm device.  Writes one JSON document (default profiles/train_gemm/timing.json) and
prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
import cases  # noqa: E402
from bench_common import summary, timed  # noqa: E402
from pn2 import heads as H  # noqa: E402
from pn2 import ops, train, tuning  # noqa: E402

LAYERS = [  # module, rows per cloud, channel chain
    ("sa1", 512 * 32, [3, 64, 64, 128]),
    ("sa2", 128 * 64, [131, 128, 128, 256]),
    ("sa3", 128, [259, 256, 512, 1024]),
]


def bench_product(runs, a):
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():  # interleaved: both routes see the same machine state
            ms[k].append(timed(fn, a.reps))
    lib, ker = runs["library"]().double(), runs["kernel"]().double()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"ms": {k: summary(v) for k, v in ms.items()},
            "ratio_library_over_kernel": round(med["library"] / med["kernel"], 3),
            "max_rel_diff": ((lib - ker).abs().max() / lib.abs().max()).item()}


def bench_layer(M, cin, cout, a):
    g = torch.Generator().manual_seed(cin * 7 + cout)
    X = torch.randn(M, cin, generator=g).cuda()
    dY = torch.randn(M, cout, generator=g).cuda()
    W = (torch.randn(cout, cin, generator=g) / cin ** 0.5).cuda()
    b = torch.randn(cout, generator=g).cuda()
    Wt = W.t()
    products = {
        "forward": {"library": lambda: torch.addmm(b, X, Wt), "kernel": lambda: ops.gemm_nt_direct(X, W, b)},
        "dx": {"library": lambda: torch.mm(dY, W), "kernel": lambda: ops.gemm_nn_direct(dY, W)},
        "dw": {"library": lambda: train._grad_weight(dY, X), "kernel": lambda: ops.gemm_tn_direct(dY, X)},
    }
    out = {"M": M, "cin": cin, "cout": cout, "gflop": round(2e-9 * M * cin * cout, 3)}
    for name, runs in products.items():
        out[name] = bench_product(runs, a)
    return out


def bench_step(B, a):
    x = cases.cloud("uniform3", B, 1024, 5).permute(0, 2, 1).contiguous().cuda()
    y = (torch.arange(B) % 7).cuda()
    torch.manual_seed(0)
    model = H.ClsSSG().cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        logp, _, _ = model(x)
        torch.nn.functional.nll_loss(logp, y).backward()
        opt.step()

    def run(key):
        with tuning.override(train_gemm=key):
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / 20 * 1e3

    ms = {0: [], 1: []}
    for _ in range(a.rounds):
        for key in (0, 1):
            ms[key].append(run(key))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"model": "ClsSSG", "B": B, "N": 1024,
            "ms_per_step": {"train_gemm=%d" % k: summary(v) for k, v in ms.items()},
            "ratio_library_over_kernel": round(med[0] / med[1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_gemm", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_train_gemm: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "slab_rows": int(ops._L.pn2_gemm_tn_slab_rows()),
           "protocol": "HIP events around `reps` back-to-back calls per route (identical inputs), after "
                       "`warmup` calls; routes interleaved within each of `rounds` rounds; median (min, "
                       "max) of the rounds; ratio = library median / kernel median.  step: wall clock "
                       "over 20 synchronised train steps after 3, the two keys interleaved",
           "layers": {}}
    for name, rows, chain in LAYERS:
        for l in range(3):
            doc["layers"]["%s.%d" % (name, l)] = bench_layer(a.B * rows, chain[l], chain[l + 1], a)
    doc["step"] = bench_step(a.B, a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

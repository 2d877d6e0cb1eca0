"""The SA layers' eval-mode forward under autograd (pn2/pointnet2_utils._SaEvalGrad) against the
route it replaces and against the no_grad forward: H.ClsSSG, B=32, N=1024, model.eval(),
parameters requiring grad, the input resident on the device.

  a  tuning eval_grad=0: the reference's torch formulation ([B,C,K,S] Conv2d / BatchNorm2d / max)
  b  the default: fused inference kernels forward, recompute on the frozen-statistics training
     kernels in the backward
  c  torch.no_grad(): forward only

forward_ms / forward_backward_ms: HIP-event time per iteration over `reps` back-to-back
iterations, after warm-up; the routes run interleaved within each of `rounds` rounds; the median
of the rounds with their min and max.  peak_bytes: torch.cuda.max_memory_allocated over one
forward + backward, less what was allocated before it.  kernels: the device kernels of the three
SA layers in one torch-profiler step of b and of c (the FC tail is left out: under autograd it
is the torch modules by design).  Needs a ROCm device.
Writes one JSON document (default profiles/eval_grad/timing.json) and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden")]
import cases  # noqa: E402
from pn2 import geometry, tuning  # noqa: E402
from pn2 import heads as H  # noqa: E402


def summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def sa_layers(model, x):
    with geometry.fps_ahead(model.sa1, model.sa2):
        p, f = model.sa1(x, None)
        p, f = model.sa2(p, f)
    return model.sa3(p, f)[1]


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = []
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and not e.name.startswith(("Memcpy", "Memset")):
            names.append(e.name.split("(")[0])
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_grad", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval_grad: needs a ROCm device")
    model = cases.build_head(H.ClsSSG, 3).cuda()
    x = cases.cloud("uniform3", a.B, a.N, 5).permute(0, 2, 1).contiguous().cuda()

    def forward():
        return model(x)

    def forward_backward():
        model.zero_grad(set_to_none=True)
        logp, l3f, _ = model(x)
        (logp.sum() + l3f.sum()).backward()

    def no_grad():
        with torch.no_grad():
            return model(x)

    def route_a(fn):
        def run():
            with tuning.override(eval_grad=0):
                return fn()
        return run

    runs = {"a_forward": route_a(forward), "b_forward": forward, "c_forward": no_grad,
            "a_forward_backward": route_a(forward_backward), "b_forward_backward": forward_backward}
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():  # interleaved: every route sees the same machine state
            ms[k].append(timed(fn, a.reps))
    peak = {}
    for k in ("a_forward_backward", "b_forward_backward"):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        runs[k]()
        torch.cuda.synchronize()
        peak[k[0]] = int(torch.cuda.max_memory_allocated() - base)
    doc = {"device": torch.cuda.get_device_name(0), "model": "ClsSSG", "B": a.B, "N": a.N, "reps": a.reps,
           "rounds": a.rounds, "warmup": a.warmup,
           "forward_ms": {k[0]: summary(v) for k, v in ms.items() if k.endswith("_forward")},
           "forward_backward_ms": {k[0]: summary(v) for k, v in ms.items() if k.endswith("_backward")},
           "peak_bytes_forward_backward": peak}
    try:
        kb = kernel_names(lambda: sa_layers(model, x))
        with torch.no_grad():
            kc = kernel_names(lambda: sa_layers(model, x))
        doc["sa_kernels"] = {"b": kb, "c": kc, "same": kb == kc}
    except Exception as e:  # the timing stands without the profile
        doc["sa_kernels"] = {"error": repr(e)}
    model.zero_grad(set_to_none=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

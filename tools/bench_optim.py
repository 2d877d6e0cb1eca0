"""The optimizer step as one launch (pn2.optim) against what it replaces, on the same inputs:

  optimizer   the step alone over the ClsSSG parameter set (46 tensors, 1.47 M elements) with
              fixed gradients: torch.optim.Adam (default: foreach), torch.optim.Adam(fused=True),
              pn2.optim.Adam; the same three for SGD(momentum=0.9)
  train_step  the whole step (zero_grad, forward, loss, backward, optimizer) of ClsSSG B=32
              N=1024 (under the reproducible keys group_backward, train_gemm, train_head,
              train_loss) and of
              pointnet_cls B=24 N=1024 (default keys), eager, in two forms: with torch's Adam
              (the behaviour before pn2.optim) and with pn2.optim.Adam

bench_common's method: HIP events around `reps` back-to-back calls, the routes interleaved
within each of `rounds` rounds after `warmup` calls, the median of the rounds with min and max.
The events bracket the stream, so a host-bound loop is measured at its wall-clock rate.
Needs a ROCm device.  Writes one JSON document (default profiles/optim/timing.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
import cases  # noqa: E402
from bench_common import interleaved, summary  # noqa: E402
from pn2 import heads, heads_v1, losses, optim  # noqa: E402
from pn2 import pointnet_utils as PU  # noqa: E402

SSG_KEYS = {"group_backward": 1, "train_gemm": 1, "train_head": 1, "train_loss": 1}


def routes(runs, a, baseline):
    ms = interleaved(runs, a)
    med = {k: statistics.median(v) for k, v in ms.items()}
    doc = {"ms": {k: summary(v) for k, v in ms.items()}}
    for k in runs:
        if k != baseline:
            doc["ratio_%s_over_%s" % (baseline, k)] = round(med[baseline] / med[k], 3)  # > 1: k is faster
    return doc


def optimizer_case(kind, a):
    shapes = [tuple(p.shape) for p in heads.ClsSSG().parameters()]
    g = torch.Generator().manual_seed(1)

    def make(cls, **kw):
        ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).cuda() * 1e-2
        if kind == "adam":
            return cls(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, **kw)
        return cls(ps, lr=0.01, momentum=0.9, **kw)

    t, o = (torch.optim.Adam, optim.Adam) if kind == "adam" else (torch.optim.SGD, optim.SGD)
    opts = {"torch": make(t), "torch_fused": make(t, fused=True), "pn2": make(o)}
    doc = routes({k: ({}, v.step) for k, v in opts.items()}, a, "torch")
    assert opts["pn2"].last_route() == "kernel"
    doc["tensors"], doc["elements"] = len(shapes), sum(p.numel() for p in opts["pn2"].param_groups[0]["params"])
    return doc


def train_step_case(name, B, N, keys, a):
    if name == "cls_ssg":
        build = lambda: cases.build_head(heads.ClsSSG, 3).cuda().train()
        x = cases.cloud("uniform3", B, N, 5).permute(0, 2, 1).contiguous().cuda()
        crit = losses.ClsLoss()

        def loss_fn(model, x, target):
            return crit(model(x)[0], target, None)
    else:
        build = lambda: cases.build_head(heads_v1.PointNetCls, 3).cuda().train()
        x = torch.randn(B, 3, N, device="cuda")
        crit = losses.ClsLoss()

        def loss_fn(model, x, target):
            pred, trans_feat, _ = model(x)
            return crit(pred, target) + PU.feature_transform_reguliarzer(trans_feat) * 0.001
    target = torch.randint(0, 7, (B,), device="cuda")

    def eager(opt_cls):
        model = build()
        opt = opt_cls(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss_fn(model, x, target).backward()
            opt.step()
        return step

    runs = {"eager_torch_adam": (keys, eager(torch.optim.Adam)), "eager_pn2_adam": (keys, eager(optim.Adam))}
    doc = routes(runs, a, "eager_torch_adam")
    doc.update({"B": B, "N": N, "tuning": keys})
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optim: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "unit": "ms per call",
           "optimizer_step_cls_ssg_parameters": {k: optimizer_case(k, a) for k in ("adam", "sgd")},
           "train_step": {"cls_ssg_B32_N1024": train_step_case("cls_ssg", 32, 1024, SSG_KEYS, a),
                          "pointnet_cls_B24_N1024": train_step_case("pointnet_cls", 24, 1024, {}, a)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

"""The PointNet-v1 autograd routes against the routes they replace, on the same inputs:

  transform    torch.bmm / pn2.train.transform_points, forward + backward (x and T both need a
               gradient), k = 3 (channel-first) and k = 64 (rows), at B=24 N=1024 and B=3 N=10240
  regulariser  feature_transform_reguliarzer, torch / pn2.train.orthogonality_loss, forward +
               backward at [24, 64, 64]
  eval         a pointnet_cls and a RotationV1 eval forward under autograd, and forward +
               backward, tuning v1_eval_grad 0 / 1, with torch.cuda.max_memory_allocated over one
               forward + backward less what was allocated before it
  train_step   a pointnet_cls B=24 train step (forward, ClsLoss + regulariser, backward, Adam),
               tuning v1_transform 0 / 1

bench_common's method: HIP events around `reps` back-to-back calls, the two routes interleaved
within each of `rounds` rounds after `warmup` calls, the median of the rounds with min and max.
Needs a ROCm device.  Writes one JSON document (default profiles/v1_autograd/timing.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
import cases  # noqa: E402
from bench_common import two_routes  # noqa: E402
from pn2 import heads_v1, losses, train, tuning  # noqa: E402
from pn2 import pointnet_utils as PU  # noqa: E402


def transform_case(B, N, k, a):
    rows = k > 16
    x = torch.randn((B, N, k) if rows else (B, k, N), device="cuda").requires_grad_()
    T = torch.randn(B, k, k, device="cuda").requires_grad_()
    dy = torch.randn_like(x)

    def torch_route():
        x.grad = T.grad = None
        (torch.bmm(x, T.transpose(1, 2)) if rows else torch.bmm(T, x)).backward(dy)

    def kernel_route():
        x.grad = T.grad = None
        train.transform_points(x, T, rows).backward(dy)

    return two_routes({"torch": ({}, torch_route), "kernels": ({}, kernel_route)}, a)


def regulariser_case(B, k, a):
    T = (torch.eye(k, device="cuda") + 0.1 * torch.randn(B, k, k, device="cuda")).requires_grad_()

    def run():
        T.grad = None
        PU.feature_transform_reguliarzer(T).backward()

    return two_routes({"torch": ({"v1_transform": 0}, run), "kernels": ({"v1_transform": 1}, run)}, a)


def peak_bytes(fn, keys):
    with tuning.override(**keys):
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)


def eval_case(name, B, N, a):
    model = cases.build_head(heads_v1.HEADS_V1[name], 3).cuda().eval()
    x = torch.randn(B, 3 if name == "pointnet_cls" else 10, N, device="cuda")

    def forward():
        out = model(x)
        return out[0] if isinstance(out, tuple) else out

    def forward_backward():
        model.zero_grad(set_to_none=True)
        forward().sum().backward()

    old, new = {"v1_eval_grad": 0}, {"v1_eval_grad": 1}
    doc = {"B": B, "N": N,
           "forward": two_routes({"torch": (old, forward), "eval_grad": (new, forward)}, a),
           "forward_backward": two_routes({"torch": (old, forward_backward), "eval_grad": (new, forward_backward)}, a),
           "peak_bytes_forward_backward": {"torch": peak_bytes(forward_backward, old),
                                           "eval_grad": peak_bytes(forward_backward, new)}}
    model.zero_grad(set_to_none=True)
    return doc


def train_step_case(B, N, a):
    model = cases.build_head(heads_v1.PointNetCls, 3).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = losses.ClsLoss()
    x = torch.randn(B, 3, N, device="cuda")
    target = torch.randint(0, 7, (B,), device="cuda")

    def step():
        pred, trans_feat, _ = model(x)
        loss = crit(pred, target) + PU.feature_transform_reguliarzer(trans_feat) * 0.001
        opt.zero_grad()
        loss.backward()
        opt.step()

    return two_routes({"torch": ({"v1_transform": 0}, step), "kernels": ({"v1_transform": 1}, step)}, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "v1_autograd", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_v1_autograd: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "unit": "ms per call", "transform_forward_backward": {}, "eval": {}}
    for B, N in ((24, 1024), (3, 10240)):
        for k in (3, 64):
            doc["transform_forward_backward"]["B%d_N%d_k%d" % (B, N, k)] = transform_case(B, N, k, a)
    doc["regulariser_forward_backward_24x64x64"] = regulariser_case(24, 64, a)
    doc["eval"]["pointnet_cls"] = eval_case("pointnet_cls", 24, 1024, a)
    doc["eval"]["rotation"] = eval_case("rotation", 3, 10240, a)
    doc["train_step_pointnet_cls_B24_N1024"] = train_step_case(24, 1024, a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

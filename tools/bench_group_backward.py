"""The grouping's feature gradient (pn2/train._GroupTrain.backward) by torch's index_add_ (tuning
group_backward=0, float atomic adds) against pn2_group_backward_f32 (group_backward=1, each
point's rows summed in position order), on identical inputs.

Shapes, each at B clouds (default 32) of 512 points, 128 FPS centroids, the neighbour lists of
ops.ball_query_direct on seeded unit-sphere clouds:
  ssg_sa2       K=64  r=0.4  D=128  rows [xyz | feature]   (H.ClsSSG.sa2)
  msg_sa2_k32   K=32  r=0.2  D=320  rows [feature | xyz]   (H.ClsMSG.sa2, its three scales)
  msg_sa2_k64   K=64  r=0.4  D=320
  msg_sa2_k128  K=128 r=0.8  D=320
  adversarial   the ssg_sa2 shape with every group's list repeating one index (the group's own
                centroid): K rows of one group go to one address

ms: HIP-event time per backward (torch.autograd.grad through the Function, so both routes carry
the same autograd overhead) over `reps` back-to-back calls after warm-up; the two routes run
interleaved within each of `rounds` rounds; the median of the rounds with their min and max.
ratio = index_add_ median / kernel median (> 1: the kernel is faster).  same_bits_every_round:
the kernel's output of every round equals the first's bit for bit; index_add_ the same question.
step: two full H.ClsSSG train steps (B clouds of 1024 points) from the same state with
group_backward=1 -- whether every parameter gradient came out bit-identical, else the first
parameter that differs.  Recorded, not asserted: the GEMMs are library calls.
Needs a ROCm device.  Writes one JSON document (default profiles/group_backward/timing.json)
and prints it."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointnet-like-pose-estimation_amd"),
                os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]
import cases  # noqa: E402
from bench_common import summary, timed  # noqa: E402
from pn2 import heads as H  # noqa: E402
from pn2 import ops, train, tuning  # noqa: E402

SHAPES = [  # name, K, radius, D, feature_first, adversarial
    ("ssg_sa2", 64, 0.4, 128, False, False),
    ("msg_sa2_k32", 32, 0.2, 320, True, False),
    ("msg_sa2_k64", 64, 0.4, 320, True, False),
    ("msg_sa2_k128", 128, 0.8, 320, True, False),
    ("adversarial", 64, 0.4, 128, False, True),
]
N, S, C = 512, 128, 3


def bench_shape(B, K, radius, D, ff, adversarial, a):
    pts = cases.cloud("uniform3", B, N, 5).cuda()
    fps_idx, centers, cpk, ppk = ops.fps_direct(pts, S, torch.zeros(B, dtype=torch.long, device="cuda"))
    idx = ops.ball_query_direct(ppk, cpk, C, radius, K)
    if adversarial:
        idx = fps_idx.view(B, S, 1).expand(B, S, K).contiguous()
    g = torch.Generator().manual_seed(6)
    feature = torch.randn(B, N, D, generator=g).cuda().requires_grad_(True)
    dg = torch.randn(B, S, K, C + D, generator=g).cuda()
    grouped = train.group_train(pts, idx, centers, feature, ff)

    def route(key):
        def run():
            with tuning.override(group_backward=key):
                return torch.autograd.grad(grouped, feature, dg, retain_graph=True)[0]
        return run

    runs = {"index_add": route(0), "kernel": route(1)}
    for fn in runs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    first = {k: fn().clone() for k, fn in runs.items()}
    same = {k: True for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():  # interleaved: both routes see the same machine state
            ms[k].append(timed(fn, a.reps))
            same[k] = same[k] and bool(torch.equal(fn().view(torch.int32), first[k].view(torch.int32)))
    diff = (first["index_add"].double() - first["kernel"].double()).abs().max().item()
    lens = torch.bincount((idx + torch.arange(B, device="cuda").view(B, 1, 1) * N).reshape(-1), minlength=B * N)
    return {"B": B, "N": N, "S": S, "K": K, "D": D, "feature_first": ff,
            "rows": B * S * K, "row_bytes_moved": B * S * K * D * 4,
            "rows_per_point": {"mean": round(lens.float().mean().item(), 2), "max": int(lens.max())},
            "ms": {k: summary(v) for k, v in ms.items()},
            "ratio_index_add_over_kernel": round(statistics.median(ms["index_add"]) /
                                                 statistics.median(ms["kernel"]), 3),
            "same_bits_every_round": same,
            "max_abs_diff_between_routes": diff,
            "max_abs_gradient": first["kernel"].abs().max().item()}


def step_reproducible(B):
    """Two ClsSSG train steps from one state under group_backward=1: are the gradients' bits equal?"""
    model = cases.build_head(H.ClsSSG, 3).cuda().train()
    state = copy.deepcopy(model.state_dict())
    x = cases.cloud("uniform3", B, 1024, 5).permute(0, 2, 1).contiguous().cuda()
    R = torch.randn(B, 7, generator=torch.Generator().manual_seed(8)).cuda()
    grads = []
    for _ in range(2):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)  # the FPS start draws
        with tuning.override(group_backward=1):
            logp, l3f, _ = model(x)
            ((logp * R).sum() + l3f.sum()).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    differ = [k for k in grads[0] if not torch.equal(grads[0][k].view(torch.int32), grads[1][k].view(torch.int32))]
    return {"model": "ClsSSG", "B": B, "N": 1024, "parameters": len(grads[0]),
            "bit_identical": not differ, "first_parameter_that_differs": differ[0] if differ else None,
            "parameters_that_differ": len(differ)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_backward", "timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_group_backward: needs a ROCm device")
    doc = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "protocol": "HIP events around `reps` back-to-back backward calls of train._GroupTrain per "
                       "route (torch.autograd.grad, identical inputs), after `warmup` calls; routes "
                       "interleaved within each of `rounds` rounds; median (min, max) of the rounds; "
                       "ratio = index_add_ median / kernel median",
           "shapes": {}}
    for name, K, radius, D, ff, adv in SHAPES:
        doc["shapes"][name] = bench_shape(a.B, K, radius, D, ff, adv, a)
    try:
        doc["step"] = step_reproducible(a.B)
    except Exception as e:  # the timing stands without the observation
        doc["step"] = {"error": repr(e)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    text = json.dumps(doc, indent=1) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

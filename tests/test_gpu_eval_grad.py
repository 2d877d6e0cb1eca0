"""The SA modules' eval-mode forward under autograd (model.eval() without torch.no_grad(),
parameters requiring grad: the reference's mutilthreading/predict_test.py pattern, and
fine-tuning with frozen BatchNorm): the forward is the no_grad forward -- the fused inference
kernels, its bits, its CPU-RNG draws -- and the backward recomputes each layer on the
frozen-statistics training kernels (pn2/pointnet2_utils._SaEvalGrad, pn2/train.mlp_max_frozen).

Gradients are compared with a float64 CPU restatement of the reference's eval formulation
(pointnet2_utils.py:163-172 / :211-221): a gather with the GPU's own centroids and neighbour
lists (the Function's saved tensors), Conv2d, eval BatchNorm2d, ReLU, torch.max in double.
Bar, as tests/test_train.py's comparison with torch: |got - ref| <= 1e-3 |ref| + 1e-3 max|ref|.
Near-tie rule, as there: a (group, channel) pair stays in the upstream gradient when the two
largest activations of its group differ by more than 1e-4 (|top| + 1e-2).  Two refinements for
these small, padded groups, where that rule alone would mask harmless pairs:
  * repeats of a list's first hit (ball-query padding) are the same row: an exact tie whose
    gradient lands on the same point and the same input row whichever copy holds the argmax,
    so the two largest are taken over a group's distinct neighbours;
  * a pair whose largest pre-ReLU value is below -1e-4 (|value| + 1e-2) is dead on both sides
    (output 0, gradient 0 through the ReLU whatever the argmax): it stays.
At most 1 % of the pairs may be masked (asserted; the seeds below meet it)."""
import copy
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from test_gpu_sa import assert_feat_close
from test_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (kind, ctor args, B, N, D, weight seed, input seed, forward seed).  The fused inference
# kernels take layer widths that are multiples of 32 (pn2_sa_mlp_max_f32): "ssg_xyz" and "msg"
# have narrower layers, which no fused forward runs (under no_grad they raise), so with autograd
# they keep the torch formulation -- asserted below, with the same gradient check; the *_w32
# cases are the same layers at the narrowest widths the new route takes.
CASES = {
    "ssg_xyz": ("ssg", (16, 8, 0.3, 3, [16, 16, 32], False), 2, 64, 0, 11, 21, 31),
    "msg": ("msg", (16, [4, 8], [0.2, 0.4], 6, [[16, 16, 32], [16, 32, 32]]), 2, 64, 6, 14, 24, 34),
    "ssg_xyz_w32": ("ssg", (16, 8, 0.3, 3, [32, 32, 64], False), 2, 64, 0, 11, 21, 31),
    "ssg_feat": ("ssg", (32, 32, 0.4, 8 + 3, [64, 64, 128], False), 2, 128, 8, 12, 22, 32),
    "group_all": ("ssg", (None, None, None, 16 + 3, [32, 64, 128], True), 2, 32, 16, 13, 23, 33),
    "msg_w32": ("msg", (16, [4, 8], [0.2, 0.4], 6, [[32, 32, 64], [32, 64, 64]]), 2, 64, 6, 14, 24, 34),
}
NARROW = ("ssg_xyz", "msg")  # the torch route
FUSED = sorted(set(CASES) - set(NARROW))


def build(name):
    from pn2 import pointnet2_utils as P
    kind, args, B, N, D, wseed, iseed, fseed = CASES[name]
    torch.manual_seed(wseed)
    mod = (P.PointNetSetAbstraction if kind == "ssg" else P.PointNetSetAbstractionMsg)(*args)
    cases.randomize_bn(mod, wseed + 1)
    return mod.eval()


def inputs(name):
    """points [B, 3, N] (unit-sphere cloud) and feature [B, D, N] or None, on the host."""
    _, _, B, N, D, _, iseed, _ = CASES[name]
    pts = cases.cloud("uniform3", B, N, iseed).permute(0, 2, 1).contiguous()
    feat = torch.randn(B, D, N, generator=torch.Generator().manual_seed(iseed + 1)) if D else None
    return pts, feat


def min_width(name):
    widths = CASES[name][1][4]
    return min(min(w) if isinstance(w, list) else w for w in widths)


def fn_node(t):
    """The _SaEvalGrad node(s) behind t, nearest first."""
    found, seen, stack = [], set(), [t.grad_fn]
    while stack:
        n = stack.pop(0)
        if n is None or n in seen:
            continue
        seen.add(n)
        if "SaEvalGrad" in type(n).__name__:
            found.append(n)
        stack += [f for f, _ in n.next_functions]
    return found


def last_path():
    from pn2 import _lib
    return _lib.load().pn2_sa_mlp_last_path()


def run_both(mod, pts, feat, fseed):
    """-> (no_grad outputs, path, rng state), (autograd outputs, path, rng state)"""
    torch.manual_seed(fseed)
    with torch.no_grad():
        want = mod(pts, feat)
    a = (want, last_path(), torch.get_rng_state())
    torch.manual_seed(fseed)
    got = mod(pts, feat)
    return a, (got, last_path(), torch.get_rng_state())


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(a.detach().cpu().numpy().view(np.int32), b.detach().cpu().numpy().view(np.int32),
                                  err_msg=what)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", FUSED)
def test_forward_is_the_no_grad_forward(name):
    """Same bits on both outputs, same CPU generator state afterwards, same kernel path; the
    feature output carries history, the centroids do not; nothing of the MLP is saved."""
    _, _, B, N, D, _, _, fseed = CASES[name]
    mod = build(name).to(DEV)
    pts, feat = (t if t is None else t.to(DEV) for t in inputs(name))
    (want, path_w, rng_w), (got, path_g, rng_g) = run_both(mod, pts, feat, fseed)
    same_bits(got[0], want[0], "new_points")
    same_bits(got[1], want[1], "new_feature")
    assert torch.equal(rng_w, rng_g)
    assert path_w == path_g
    assert got[1].requires_grad and not got[0].requires_grad
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert got[0].stride() == want[0].stride() and got[1].stride() == want[1].stride()
    nodes = fn_node(got[1])
    assert len(nodes) == 1
    saved = sum(t.numel() * t.element_size() for t in nodes[0].saved_tensors if t is not None)
    S, K = (1, N) if name == "group_all" else (CASES[name][1][0], np.max(CASES[name][1][1]))
    print("%s: saved %d bytes, bound %d" % (name, saved, B * S * K * min_width(name) * 4))
    assert saved < B * S * K * min_width(name) * 4
    if name == "ssg_xyz_w32":  # the radius leaves padded groups (repeats of the first hit)
        idx = nodes[0].saved_tensors[3]
        assert bool(((idx[..., 1:] == idx[..., :1]).any(-1)).any())


# ------------------------------------------------------------------ gradients
def restate(name, mod, pts, feat, centers, idxs):
    """The reference's eval formulation in float64 on the host from the GPU's centroids and
    lists -> (out [B, Cout, S], clear [B, Cout, S] bool, feature leaf or None)."""
    kind = CASES[name][0]
    ref = copy.deepcopy(mod).cpu().double().eval()
    P = pts.cpu().double().permute(0, 2, 1)
    leaf = None if feat is None else feat.cpu().double().requires_grad_(True)
    Fv = None if leaf is None else leaf.permute(0, 2, 1)
    B, N, C = P.shape
    b = torch.arange(B).view(B, 1, 1)
    if kind == "ssg" and ref.group_all:
        blocks = [(ref.mlp_convs, ref.mlp_bns, None)]
    elif kind == "ssg":
        blocks = [(ref.mlp_convs, ref.mlp_bns, idxs[0])]
    else:
        blocks = [(c, n, i) for c, n, i in zip(ref.conv_blocks, ref.bn_blocks, idxs)]
    outs, clears = [], []
    for convs, bns, idx in blocks:
        if idx is None:
            grouped = torch.cat([P.view(B, 1, N, C), Fv.reshape(B, 1, N, -1)], -1)
            dup = torch.zeros(B, 1, N, dtype=torch.bool)
        else:
            idx = idx.cpu().long()
            g = P[b, idx] - centers.cpu().double().unsqueeze(2)
            if Fv is None:
                grouped = g
            else:
                grouped = torch.cat([Fv[b, idx], g] if kind == "msg" else [g, Fv[b, idx]], -1)
            dup = idx == idx[..., :1]
            dup[..., 0] = False
        x = grouped.permute(0, 3, 2, 1)  # [B, C, K, S]
        for conv, bn in zip(convs, bns):
            pre = bn(conv(x))
            x = F.relu(pre)
        gone = dup.permute(0, 2, 1).unsqueeze(1)  # [B, 1, K, S]
        h = x.detach().masked_fill(gone, -float("inf"))
        if h.shape[2] > 1:
            top2 = torch.topk(h, 2, dim=2)[0]
            t0, t1 = top2[:, :, 0], top2[:, :, 1]
        else:
            t0, t1 = h[:, :, 0], torch.full_like(h[:, :, 0], -float("inf"))
        live = (t0 - t1) > 1e-4 * (t0.abs() + 1e-2)
        p0 = pre.detach().masked_fill(gone, -float("inf")).max(2)[0]
        dead = p0 < -1e-4 * (p0.abs() + 1e-2)
        outs.append(torch.max(x, 2)[0])
        clears.append(live | dead)
    return torch.cat(outs, 1), torch.cat(clears, 1), leaf, ref


def lists_of(name, pts_d, fseed):
    """The centroids and int64 neighbour lists a forward seeded with fseed makes (the torch
    route's own calls, pointnet2_utils._forward_autograd)."""
    from pn2 import ops, shard
    kind, args = CASES[name][:2]
    P = pts_d.permute(0, 2, 1)
    B, N, C = P.shape
    torch.manual_seed(fseed)
    _, centers, cpk, ppk = ops.fps_direct(P, args[0], shard.host_start(B, N, P.device))
    radii, ks = (args[2], args[1]) if kind == "msg" else ([args[2]], [args[1]])
    return centers, [ops.ball_query_direct(ppk, cpk, C, r, k) for r, k in zip(radii, ks)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradients_match_float64_restatement(name):
    _, _, B, N, D, _, iseed, fseed = CASES[name]
    mod = build(name).to(DEV)
    pts, feat = inputs(name)
    pts_d = pts.to(DEV)
    feat_d = None if feat is None else feat.to(DEV).requires_grad_(True)
    buffers = {k: v.clone() for k, v in mod.named_buffers()}
    torch.manual_seed(fseed)
    _, out = mod(pts_d, feat_d)
    assert out.requires_grad
    if name in NARROW:  # widths the fused kernels reject: the torch route, still differentiable
        assert not fn_node(out)
        centers, idxs = lists_of(name, pts_d, fseed)
    else:
        node = fn_node(out)[0]
        _, _, centers, *idxs = node.saved_tensors
    out_ref, clear, leaf, ref = restate(name, mod, pts, feat, centers, idxs)
    masked = float((~clear).sum()) / clear.numel()
    print("%s: masked share %.4f of %d pairs" % (name, masked, clear.numel()))
    assert masked <= 0.01
    close(out.detach().cpu(), out_ref.detach(), 1e-4, "out")
    R = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(iseed + 7), dtype=torch.float64) * clear
    rng_before = torch.get_rng_state()
    (out * R.float().to(DEV)).sum().backward()
    assert torch.equal(torch.get_rng_state(), rng_before)  # no draw in the backward
    (out_ref * R).sum().backward()
    for (k, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, k
        assert float(q.grad.abs().max()) > 0, k
        close(p.grad.cpu(), q.grad, 1e-3, "grad " + k)
    if leaf is not None:
        close(feat_d.grad.cpu(), leaf.grad, 1e-3, "feature grad")
    for k, v in mod.named_buffers():  # running statistics and counters: not a bit moved
        assert torch.equal(v, buffers[k]), k


# ------------------------------------------------------------------ the stack
def _stack(seed=3):
    from pn2 import heads as H
    torch.manual_seed(seed)
    model = H.ClsSSG().eval()
    cases.randomize_bn(model, seed)
    x = cases.cloud("uniform3", 2, 256, 5).permute(0, 2, 1).contiguous()
    return model.to(DEV), x.to(DEV)


def test_stack_forward_bits_and_side_job():
    """H.ClsSSG: sa1, sa2 and sa3 all take the route; l3f has the no_grad bits, the generator
    ends in the same state, and sa2's FPS still rides on sa1's MLP launch."""
    from pn2 import ops
    model, x = _stack()
    jobs = []
    orig = ops.fps_side_job
    ops.fps_side_job = lambda *a: jobs.append(1) or orig(*a)
    try:
        torch.manual_seed(1)
        with torch.no_grad():
            want = model(x)
        n_want, rng_w = len(jobs), torch.get_rng_state()
        torch.manual_seed(1)
        got = model(x)
        n_got, rng_g = len(jobs) - n_want, torch.get_rng_state()
    finally:
        ops.fps_side_job = orig
    same_bits(got[1], want[1], "l3f")
    assert torch.equal(rng_w, rng_g) and n_got == n_want
    assert got[1].requires_grad and got[0].requires_grad
    assert len(fn_node(got[1])) == 3
    assert_feat_close(got[0].detach().cpu().numpy(), want[0].cpu().numpy())


def test_frozen_bn_fine_tune_step():
    """Forward, loss.backward(), SGD step with model.eval(): every parameter moves, no running
    statistic or counter does, and the next forward runs on the new weights (the pack cache
    follows the parameters' version counters)."""
    model, x = _stack()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    before_p = {k: v.detach().clone() for k, v in model.named_parameters()}
    before_b = {k: v.clone() for k, v in model.named_buffers()}
    torch.manual_seed(1)
    logp, l3f, _ = model(x)
    loss = F.nll_loss(logp, torch.tensor([1, 4], device=DEV)) + 1e-3 * l3f.square().mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    for k, v in model.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
        assert not torch.equal(v.detach(), before_p[k]), "%s did not move" % k
    for k, v in model.named_buffers():
        assert torch.equal(v, before_b[k]), k
    torch.manual_seed(1)
    again = model(x)[1]
    fresh = copy.deepcopy(model)
    for m in fresh.modules():  # no cache carried over: packed from the stepped weights
        if hasattr(m, "_pack_cache"):
            m._pack_cache = {} if isinstance(m._pack_cache, dict) else [{} for _ in m._pack_cache]
    torch.manual_seed(1)
    with torch.no_grad():
        want = fresh(x)[1]
    same_bits(again, want, "second forward")
    assert not torch.equal(again.detach(), l3f.detach())


# ------------------------------------------------------------------ routes
def test_routes():
    import pn2
    from pn2 import tuning
    name = "ssg_feat"
    fseed = CASES[name][7]
    mod = build(name).to(DEV)
    pts, feat = (t.to(DEV) for t in inputs(name))
    torch.manual_seed(fseed)
    with torch.no_grad():
        want = mod(pts, feat)
    # eval_grad = 0: the torch formulation, differentiable, within the feature tolerance
    with tuning.override(eval_grad=0):
        torch.manual_seed(fseed)
        got = mod(pts, feat)
    assert got[1].requires_grad and not fn_node(got[1])
    same_bits(got[0], want[0])
    assert_feat_close(got[1].detach().cpu().numpy(), want[1].cpu().numpy())
    got[1].sum().backward()
    assert mod.mlp_convs[0].weight.grad is not None
    mod.zero_grad()
    # fused_eval(): the no_grad bits without history
    torch.manual_seed(fseed)
    with pn2.fused_eval():
        fz = mod(pts, feat)
    assert not fz[1].requires_grad and not fz[0].requires_grad
    same_bits(fz[0], want[0])
    same_bits(fz[1], want[1])
    # coordinates that need a gradient: the torch route, which carries it
    p2 = pts.clone().requires_grad_(True)
    torch.manual_seed(fseed)
    got = mod(p2, feat)
    assert not fn_node(got[1])
    got[1].sum().backward()
    assert p2.grad is not None and float(p2.grad.abs().max()) > 0
    mod.zero_grad()
    # a double backward raises
    torch.manual_seed(fseed)
    out = mod(pts, feat)[1]
    assert fn_node(out)
    w = mod.mlp_convs[0].weight
    g, = torch.autograd.grad(out.sum(), w, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), w)


def _swap(kind):
    """An ssg_feat module with one property the frozen-statistics route does not cover."""
    mod = build("ssg_feat")
    if kind == "bn_not_affine":
        mod.mlp_bns[1] = torch.nn.BatchNorm2d(64, affine=False).eval()
    elif kind == "bn_no_running_stats":
        mod.mlp_bns[1] = torch.nn.BatchNorm2d(64, track_running_stats=False).eval()
    elif kind == "conv_no_bias":
        mod.mlp_convs[1] = torch.nn.Conv2d(64, 64, 1, bias=False)
    elif kind == "width_not_x32":
        mod.mlp_convs[1] = torch.nn.Conv2d(64, 48, 1)
        mod.mlp_bns[1] = torch.nn.BatchNorm2d(48).eval()
        mod.mlp_convs[2] = torch.nn.Conv2d(48, 128, 1)
    elif kind == "five_layers":
        mod.mlp_convs.append(torch.nn.Conv2d(128, 128, 1))
        mod.mlp_bns.append(torch.nn.BatchNorm2d(128).eval())
        mod.mlp_convs.append(torch.nn.Conv2d(128, 128, 1))
        mod.mlp_bns.append(torch.nn.BatchNorm2d(128).eval())
    elif kind == "bf16_precision":
        mod.mlp_precision = "bf16"
    return mod


@pytest.mark.parametrize("kind", ["bn_not_affine", "bn_no_running_stats", "conv_no_bias", "width_not_x32",
                                  "five_layers", "bf16_precision"])
def test_fallbacks_keep_the_torch_route(kind):
    """Each listed property sends an eval forward under autograd to the torch formulation: no
    _SaEvalGrad node, and a backward still reaches every parameter and the feature."""
    mod = _swap(kind).to(DEV)
    pts, feat = (t.to(DEV) for t in inputs("ssg_feat"))
    feat.requires_grad_(True)
    torch.manual_seed(CASES["ssg_feat"][7])
    new_points, out = mod(pts, feat)
    assert out.requires_grad and not fn_node(out)
    assert out.shape == (2, mod.mlp_convs[-1].weight.shape[0], 32) and bool(torch.isfinite(out).all())
    out.sum().backward()
    for k, p in mod.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert feat.grad is not None and float(feat.grad.abs().max()) > 0


def test_route_predicate_rejects_non_float32():
    """Half and double tensors never reach the fused route (the index kernels take float32 only,
    so such a forward is not run end to end here)."""
    from pn2 import pointnet2_utils as P
    mod = build("ssg_feat").to(DEV)
    pts, feat = (t.to(DEV) for t in inputs("ssg_feat"))
    assert P._eval_grad_route(mod, pts, feat)
    assert not P._eval_grad_route(mod, pts.double(), feat)
    assert not P._eval_grad_route(mod, pts, feat.half())
    assert not P._eval_grad_route(copy.deepcopy(mod).double(), pts, feat)
    assert not P._eval_grad_route(copy.deepcopy(mod).train(), pts, feat)


def test_backward_refuses_changed_buffers():
    """The recompute reads parameters and BatchNorm buffers: a change between the forward and
    its backward raises instead of giving another function's gradient."""
    mod = build("ssg_feat").to(DEV)
    pts, feat = (t.to(DEV) for t in inputs("ssg_feat"))
    torch.manual_seed(1)
    out = mod(pts, feat)[1]
    with torch.no_grad():
        mod.mlp_bns[0].running_var.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        out.sum().backward()


def test_two_threads_each_their_model_and_stream():
    """The predict_test.py pattern: two host threads, each with its own model and stream, eval
    mode, autograd on.  Each gets the bits of its own no_grad forward."""
    from pn2 import shard
    name = "ssg_xyz_w32"
    pts, _ = inputs(name)
    res, errs = {}, []

    def work(k):
        try:
            torch.manual_seed(100 + k)
            mod = build(name).to(DEV)
            x = (pts + 0.01 * k).to(DEV)
            with torch.cuda.stream(torch.cuda.Stream()):
                with shard.thread_generator(torch.Generator().manual_seed(k)):
                    with torch.no_grad():
                        want = mod(x, None)
                with shard.thread_generator(torch.Generator().manual_seed(k)):
                    got = mod(x, None)
                torch.cuda.current_stream().synchronize()
            res[k] = (want, got)
        except Exception as e:  # surfaced below
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in range(2):
        want, got = res[k]
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        assert got[1].requires_grad and len(fn_node(got[1])) == 1

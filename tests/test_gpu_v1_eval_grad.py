"""The PointNet-v1 modules' eval-mode forward under autograd with tuning key v1_eval_grad=1
(pn2/pointnet_utils._V1EvalGrad): run_mlp gives the bits of the no_grad point_mlp call; the
gradients of TNetkd, PointNetEncoder, RotationV1, SignV1 and PoseV1(transform, feat_trans) match
a float64 torch restatement (the module's own torch formulation, copied to the host in double)
at the SA eval-grad tests' bar, |got - ref| <= 1e-3 |ref| + 1e-3 max|ref|; buffers stay; an
in-place change between forward and backward raises; pn2.eval_autograd() and key 0 keep the
torch route (asserted through ops.kernel_timer); the recompute backward's peak memory is below
the torch formulation's.  And the reproducibility of a pointnet_cls / PoseV1 train step under
train_gemm=1, train_head=1, train_loss=1, v1_transform=1: two steps from one state give the same
bits in the loss, every gradient, every buffer and every parameter."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
POSE_KW = dict(mlp_list=[64, 64, 128, 1024], linear_list=[512, 256, 2], transform=True, feat_trans=True,
               num_category=0, normal_channel=False)


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(a.detach().cpu().numpy().view(np.int32), b.detach().cpu().numpy().view(np.int32),
                                  err_msg=str(what))


class Stack(nn.Module):
    def __init__(self, widths):
        super().__init__()
        self.conv = nn.ModuleList(nn.Conv1d(a, b, 1) for a, b in zip(widths[:-1], widths[1:]))
        self.bn = nn.ModuleList(nn.BatchNorm1d(b) for b in widths[1:])


def stack(widths, seed):
    torch.manual_seed(seed)
    m = Stack(widths)
    cases.randomize_bn(m, seed + 1)
    return m.to(DEV).eval()


# ------------------------------------------------------------------ run_mlp: the no_grad bits
@pytest.mark.parametrize("rows,widths", [(False, [6, 64, 64, 128]), (True, [64, 128, 1024]),
                                         (False, [10, 64, 64, 64, 128, 1024])])
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("last_relu", [True, False])
def test_run_mlp_gives_the_no_grad_bits(rows, widths, pool, last_relu):
    from pn2 import ops, pointnet_utils as PU, tuning
    if len(widths) > 5 and not pool:
        widths = widths[:4]  # [B, N, 1024] rows add nothing over the 128-wide ones
    B, N = 2, 50  # N is no multiple of 32
    m = stack(widths, 7)
    convs, bns = list(m.conv), list(m.bn)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, widths[0], generator=g).to(DEV) if rows else torch.randn(B, widths[0], N, generator=g).to(DEV)
    with torch.no_grad():
        want = PU.point_mlp(x, convs, bns, {}, pool, last_relu, m, rows)
    assert PU.mlp_mode(m, x, convs, bns) == "torch"  # key 0
    with tuning.override(v1_eval_grad=1), ops.kernel_timer() as t:
        mode = PU.mlp_mode(m, x, convs, bns)
        assert mode == "eval_grad"
        got = PU.run_mlp(mode, x, convs, bns, {}, pool, last_relu, m, rows)
    launched = set(t.summary())  # the no_grad launches: the packing and the fused MLP, no training kernel
    assert "pn2_sa_mlp_max_f32" in launched and launched <= {"pn2_sa_mlp_max_f32", "pn2_pack_layer_f32",
                                                               "pn2_pack_layer_split_bf16"}
    assert "V1EvalGrad" in type(got.grad_fn).__name__ and got.shape == want.shape
    same_bits(got, want)
    with tuning.override(v1_eval_grad=1):
        xg = x.clone().requires_grad_()
        got = PU.run_mlp("eval_grad", xg, convs, bns, {}, pool, last_relu, m, rows)
        same_bits(got, want)
        got.sum().backward()
    assert xg.grad is not None and xg.grad.shape == x.shape and torch.isfinite(xg.grad).all()
    assert all(p.grad is not None for p in m.parameters())


def test_mode_conditions():
    from pn2 import pointnet_utils as PU, tuning
    import pn2
    m = stack([6, 64, 128], 5)
    convs, bns = list(m.conv), list(m.bn)
    x = torch.randn(2, 6, 40, device=DEV)
    with tuning.override(v1_eval_grad=1):
        assert PU.mlp_mode(m, x, convs, bns) == "eval_grad"
        with torch.no_grad():
            assert PU.mlp_mode(m, x, convs, bns) == "fused"
        with pn2.eval_autograd():
            assert PU.mlp_mode(m, x, convs, bns) == "torch"
        with pn2.fused_eval():
            assert PU.mlp_mode(m, x, convs, bns) == "fused"
        with pn2.mlp_precision("bf16"):
            assert PU.mlp_mode(m, x, convs, bns) == "torch"
        assert PU.mlp_mode(m, x.double(), convs, bns) == "torch"
        narrow = stack([6, 16, 64], 5)
        assert PU.mlp_mode(narrow, x, list(narrow.conv), list(narrow.bn)) == "torch"
        nostats = stack([6, 64], 5)
        nostats.bn[0] = nn.BatchNorm1d(64, track_running_stats=False).to(DEV).eval()
        assert PU.mlp_mode(nostats, x, list(nostats.conv), list(nostats.bn)) == "torch"
        m.train()
        assert PU.mlp_mode(m, x, convs, bns) == "train"


# ------------------------------------------------------------------ gradients
def build(name):
    from pn2 import heads_v1, pointnet_utils as PU
    torch.manual_seed(50 + len(name))
    mod = {"tnetkd": lambda: PU.TNetkd(64), "encoder": lambda: PU.PointNetEncoder(channel=3),
           "rotation": heads_v1.RotationV1, "sign": heads_v1.SignV1,
           "pose": lambda: heads_v1.PoseV1(**POSE_KW)}[name]()
    cases.randomize_bn(mod, 61)
    C = {"tnetkd": 64, "encoder": 3, "rotation": 10, "sign": 10, "pose": 3}[name]
    x = torch.randn(2, C, 96, generator=torch.Generator().manual_seed(8)) * 0.5
    return mod.eval(), x


def outputs(name, out):
    """The differentiable outputs."""
    if name == "encoder":
        return list(out)
    if name == "sign":
        return [out[0]]
    return [out]


def scalar(outs, dtype, device):
    total = 0
    for i, o in enumerate(outs):
        w = torch.randn(o.shape, generator=torch.Generator().manual_seed(100 + i), dtype=torch.float64)
        total = total + (o * w.to(device=device, dtype=dtype)).sum()
    return total


def close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs()
    bound = 1e-3 * ref.abs() + 1e-3 * ref.abs().max()
    print("%-28s max err %.3e  max|ref| %.3e  worst err/bound %.3f" % (what, err.max(), ref.abs().max(),
                                                                     (err / bound.clamp_min(1e-300)).max()))
    assert (err <= bound).all(), what


NAMES = ("tnetkd", "encoder", "rotation", "sign", "pose")
KEYSETS = {"eval_grad": dict(v1_eval_grad=1), "all": dict(v1_eval_grad=1, v1_transform=1, train_head=1, train_gemm=1)}


@pytest.mark.parametrize("keys", sorted(KEYSETS))
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_float64_torch(name, keys):
    import pn2
    from pn2 import ops, tuning
    mod, x = build(name)
    ref_mod = copy.deepcopy(mod).double()
    xr = x.double().requires_grad_()
    with pn2.eval_autograd():  # the reference's torch formulation, on the host in float64
        scalar(outputs(name, ref_mod(xr)), torch.float64, "cpu").backward()
    mod = mod.to(DEV)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    xg = x.to(DEV).requires_grad_()
    with tuning.override(**KEYSETS[keys]), ops.kernel_timer() as t:
        outs = outputs(name, mod(xg))
        scalar(outs, torch.float32, DEV).backward()
    launched = set(t.summary())
    assert "pn2_sa_mlp_max_f32" in launched and "pn2_bn_relu_backward_f32" in launched
    if keys == "all" and name in ("encoder", "pose"):
        assert {"pn2_transform_points_f32", "pn2_transform_points_backward_f32"} <= launched
    for k, v in mod.state_dict().items():  # running statistics, num_batches_tracked, parameters
        assert torch.equal(v, before[k]), k
    close(xg.grad, xr.grad, name + " dx")
    for (pn, p), (_, pr) in zip(mod.named_parameters(), ref_mod.named_parameters()):
        if pr.grad is None:  # RotationV1's unused T-Net
            assert p.grad is None, pn
            continue
        close(p.grad, pr.grad, name + " " + pn)


def test_in_place_change_raises():
    from pn2 import heads_v1, tuning
    mod, x = build("rotation")
    mod = mod.to(DEV)
    with tuning.override(v1_eval_grad=1):
        out = mod(x.to(DEV))
        with torch.no_grad():
            mod.conv[3].weight.mul_(1.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            out.sum().backward()
        out = mod(x.to(DEV))
        mod.train()
        with pytest.raises(RuntimeError, match="left eval mode"):
            out.sum().backward()


def test_routes_through_kernel_timer():
    """Key 0, and pn2.eval_autograd() under key 1: the torch formulation -- no pn2 kernel runs.
    Key 1: the fused forward kernels and the frozen training kernels."""
    import pn2
    from pn2 import ops, tuning
    mod, x = build("rotation")
    mod, x = mod.to(DEV), x.to(DEV)
    with ops.kernel_timer() as t:
        mod(x).sum().backward()
    assert not t.summary()
    with tuning.override(v1_eval_grad=1), pn2.eval_autograd(), ops.kernel_timer() as t:
        mod(x).sum().backward()
    assert not t.summary()
    with tuning.override(v1_eval_grad=1), ops.kernel_timer() as t:
        mod(x).sum().backward()
    s = t.summary()
    assert s["pn2_sa_mlp_max_f32"]["launches"] >= 3 and "pn2_bn_relu_group_max_f32" in s


def test_peak_memory_below_the_torch_formulation():
    from pn2 import tuning
    mod, _ = build("rotation")
    mod = mod.to(DEV)
    x = torch.randn(4, 10, 4096, device=DEV)

    def peak(**keys):
        for p in mod.parameters():
            p.grad = None
        with tuning.override(**keys):
            mod(x).sum().backward()  # warm: caches, workspaces
            for p in mod.parameters():
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            mod(x).sum().backward()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() - base

    old, new = peak(v1_eval_grad=0), peak(v1_eval_grad=1)
    print("peak bytes above the resident state, forward + backward: torch %d, eval_grad %d" % (old, new))
    assert new < old


# ------------------------------------------------------------------ a reproducible train step
def train_step(name, state, keys):
    from pn2 import heads_v1, losses, pointnet_utils as PU, tuning
    B, N = 4, 128
    torch.manual_seed(1)
    model = heads_v1.PointNetCls() if name == "pointnet_cls" else heads_v1.PoseV1(classify=True, **POSE_KW)
    model.load_state_dict(state)
    model = model.to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 3, N, generator=g).to(DEV)
    target = torch.randint(0, 2, (B,), generator=g).to(DEV)
    crit = losses.ClsLoss()
    with tuning.override(**keys):
        torch.manual_seed(9)  # dropout's mask
        torch.cuda.manual_seed(9)
        if name == "pointnet_cls":
            pred, trans_feat, _ = model(x)
        else:
            pred, _, _ = model(x)
            trans_feat = model.ftnet_out
        # pointnet_cls.get_loss: the criterion plus the regulariser, scaled
        loss = crit(pred, target) + PU.feature_transform_reguliarzer(trans_feat) * 0.001
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    out = {"loss": loss.detach()}
    out.update({"grad." + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    out.update({"state." + k: v for k, v in model.state_dict().items()})
    return out


@pytest.mark.parametrize("name", ["pointnet_cls", "pose"])
def test_train_step_is_reproducible(name, monkeypatch):
    from pn2 import heads_v1, ops
    keys = dict(train_gemm=1, train_head=1, train_loss=1, v1_transform=1)
    if name == "pose":  # PoseV1 does not return its feature transform: keep it for the regulariser
        orig = heads_v1.PoseV1._split_ftnet

        def keep(self, x, mode):
            h, T = orig(self, x, mode)
            self.ftnet_out = T
            return h, T
        monkeypatch.setattr(heads_v1.PoseV1, "_split_ftnet", keep)
    torch.manual_seed(2)
    model = heads_v1.PointNetCls() if name == "pointnet_cls" else heads_v1.PoseV1(classify=True, **POSE_KW)
    state = copy.deepcopy(model.state_dict())
    with ops.kernel_timer() as t:
        a = train_step(name, state, keys)
    launched = set(t.summary())
    assert {"pn2_transform_points_f32", "pn2_transform_points_backward_f32", "pn2_orthogonality_forward_f32",
            "pn2_orthogonality_backward_f32", "pn2_gemm_tn_f32"} <= launched
    b = train_step(name, state, keys)
    assert set(a) == set(b) and any(k.startswith("grad.") for k in a)
    for k in sorted(a):
        assert torch.equal(a[k], b[k]), k
        if a[k].is_floating_point():
            assert torch.isfinite(a[k]).all(), k

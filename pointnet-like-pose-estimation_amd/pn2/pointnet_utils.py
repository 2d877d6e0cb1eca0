"""Drop-in for /root/reference/model/pointnet_utils.py (PointNet v1: T-Nets + shared-MLP
encoder) on MI355X -- SURVEY.md §8(f) rank 1.

Same public names, constructor signatures, submodule names (so ``state_dict`` keys match the
reference's checkpoints) and forward contracts:

  TNet3d(channel)        pointnet_utils.py:9-43   x [B,C,N] -> transform [B,3,3]
  TNetkd(channel)        pointnet_utils.py:45-81  x [B,k,N] -> transform [B,k,k]
  PointNetEncoder(global_feat=True, channel=3)
                         pointnet_utils.py:83-138 x [B,D,N] -> (global [B,1024] or
                                                  [B,1088,N], transform, trans_feat)
  feature_transform_reguliarzer(transform)        pointnet_utils.py:140-147

The hot part of every v1 network is the same as a group_all SA layer (pointnet2_utils.py
:163-172): a per-point shared MLP (Conv1d 1x1 + BatchNorm1d + ReLU)* followed by a max over
the N points.  In eval mode it runs on pn2's split-bf16 dense-layer kernels (pn2_sa_mlp_max_f32
with a group_all source for a channel-first [B,C<=16,N] input, or a rows source for per-point
features already in HBM), one launch per layer, the max fused into the last layer's epilogue;
the encoder's conv3 + bn3 without ReLU before its max uses PN2_LAYER_NO_RELU (signed pooling).
The small per-cloud transforms (torch.bmm of a 3x3 / 64x64 matrix with the points) and the
T-Nets' FC layers are plain library GEMMs (torch on the GPU) in the no_grad forward.  Training
on the GPU runs the same shared MLPs through pn2.train.point_mlp_train (library GEMMs, or the
train_gemm kernels, + the fused batch-statistics BN / ReLU / max kernels, forward and backward)
in the same rows layout.  Eval with autograd keeps the reference's torch formulation by default
(as do exotic BN configurations); with tuning key v1_eval_grad=1 it is mlp_mode's fourth answer,
"eval_grad": the fused kernels forward -- the no_grad launches and bits -- inside _V1EvalGrad,
which saves the MLP's input only and recomputes the MLP on pn2.train.point_mlp_frozen in its
backward.  With tuning key train_head=1 the T-Nets' FC tail under autograd (fc1/bn4, fc2/bn5,
fc3) runs on the kernels of csrc/fc_train.hip (pn2.train.linear_bn_train); the ``+ iden`` stays
a torch add.  With tuning key v1_transform=1 the transforms of a differentiable forward
(apply_transform: train mode and eval under autograd, float32 device tensors, k <= 64) run
pn2.train.transform_points and feature_transform_reguliarzer runs pn2.train.orthogonality_loss
(csrc/v1_transform.hip: every sum in a stated order, forward and backward); torch.bmm otherwise.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import ops
from . import train
from . import tuning
from .pointnet2_utils import _in_eval_autograd, _needs_autograd, _precision, _versions


# ----------------------------------------------------------------------------- eval-mode MLPs
def _pack(convs, bns, cache, xyz):
    """Folded (W^T, alpha, beta) and split images of Conv1d + BatchNorm1d layers; cached until a
    parameter changes.  xyz: channels of a channel-first first-layer input (group_all source,
    all of them in the split image's first block), 0 for a rows source."""
    tensors = []
    for conv, bn in zip(convs, bns):
        tensors += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = (xyz,) + tuple((t.data_ptr(), t._version) for t in tensors if t is not None)
    if cache.get("key") != key:
        wts, als, bes, cins, splits = [], [], [], [], []
        with torch.no_grad():
            for li, (conv, bn) in enumerate(zip(convs, bns)):
                wt, al, be = ops.pack_layer_direct(conv.weight, conv.bias, bn.weight, bn.bias,
                                                   bn.running_mean, bn.running_var, float(bn.eps), 0)
                wts.append(wt)
                als.append(al)
                bes.append(be)
                cins.append(conv.weight.shape[1])
                splits.append(ops.pack_layer_split_direct(conv.weight, xyz if li == 0 else 0, True))
        cache["key"] = key
        cache["layers"] = (wts, als, bes, cins, splits)
    return cache["layers"]


def point_mlp(x, convs, bns, cache, pool=True, last_relu=True, module=None, rows=False):
    """relu(bn(conv(x))) over every point (the last layer without ReLU if not last_relu), then
    the max over the points when pool.  x: channel-first [B, C, N] (rows=False, any strides:
    C <= 16 is read in place as a group_all source, wider inputs as rows) or per-point rows
    [B, N, C] (rows=True, unit column stride, as a previous point_mlp returns them).
    Returns [B, cout] (pool) or rows [B, N, cout]."""
    if not rows and x.shape[1] > 16:
        x, rows = _cf_to_rows(x), True
    chan_first = not rows
    if chan_first:
        B, C, N = x.shape
        pts = x.permute(0, 2, 1)
        layers = _pack(convs, bns, cache, C)
    else:
        B, N, C = x.shape
        layers = _pack(convs, bns, cache, 0)
    wts, als, bes, cins, splits = layers
    cout = wts[-1].shape[1]
    n = len(wts)
    flags = [0] * n
    if not last_relu:
        flags[-1] = _lib.LAYER_NO_RELU
    out = torch.empty((B if pool else B * N), cout, device=x.device, dtype=torch.float32)
    prec = "fp32" if module is None else _precision(module)
    # the kernels take <= 4 layers per call: longer chains go through a rows intermediate
    if n > 4:
        mid = point_mlp(x, convs[:n - 3], bns[:n - 3], cache.setdefault("head", {}), pool=False,
                        module=module, rows=rows)
        return point_mlp(mid, convs[n - 3:], bns[n - 3:], cache.setdefault("tail", {}), pool,
                         last_relu, module, rows=True)
    if chan_first:
        ops.sa_mlp_max_direct(out, _lib.SRC_GROUP_ALL, pts, None, None, None, wts, als, bes, cins,
                              splits, prec, flags, pool=pool)
    else:
        ops.sa_mlp_max_direct(out, _lib.SRC_ROWS, None, None, None, None, wts, als, bes, cins,
                              splits, prec, flags, rows=x, pool=pool)
    return out if pool else out.view(B, N, cout)


def _eval_grad_route(module, x, convs, bns):
    """Whether an eval-mode v1 shared MLP that must be differentiable runs the fused inference
    kernels with the recompute backward (_V1EvalGrad): tuning key v1_eval_grad=1, outside
    pn2.eval_autograd(), float32 device tensors, fp32 arithmetic, widths the fused entry takes
    and layers the frozen-statistics kernels cover."""
    if module.training or tuning.get("v1_eval_grad") != 1 or _in_eval_autograd():
        return False
    if not x.is_cuda or x.dtype != torch.float32 or _precision(module) != "fp32":
        return False
    if not all(ops.sa_mlp_supported([c.weight.shape[0]]) for c in convs):
        return False
    return train.eligible_frozen(x, convs, bns)


def mlp_mode(module, x, convs, bns):
    """How a v1 module runs its shared MLPs on x: "fused" (eval without autograd: the split-bf16
    kernels; a CPU tensor raises), "train" (training on the device: pn2.train), "eval_grad" (eval
    with autograd under tuning key v1_eval_grad=1: the fused kernels forward, the frozen
    training kernels recomputing in the backward -- _V1EvalGrad) or "torch" (the reference's
    formulation: eval with autograd otherwise, CPU training, BN configs pn2.train does not
    cover)."""
    if not _needs_autograd(module, x):
        return "fused"
    if module.training and train.eligible(x, convs, bns):
        return "train"
    if _eval_grad_route(module, x, convs, bns):
        return "eval_grad"
    return "torch"


class _V1EvalGrad(torch.autograd.Function):
    """A v1 shared MLP's eval-mode forward under autograd (modelled on pointnet2_utils
    _SaEvalGrad): the forward is point_mlp as it is -- the launches and the bits of the no_grad
    call on the same input; nothing of the MLP is saved, only the input and the module's
    versions.  The backward recomputes the MLP on the frozen-statistics training kernels
    (train.point_mlp_frozen) and backpropagates through that: gradients of the reference's eval
    formulation (Conv1d + BatchNorm1d on its running statistics) for the input and the conv / BN
    parameters."""

    @staticmethod
    def forward(ctx, module, convs, bns, cache, pool, last_relu, rows, x, *params):
        out = point_mlp(x, convs, bns, cache, pool, last_relu, module, rows)
        ctx.module, ctx.convs, ctx.bns = module, convs, bns  # the recompute reads the live parameters
        ctx.cfg = (pool, last_relu, rows)
        ctx.versions = _versions(module)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        module = ctx.module
        if _versions(module) != ctx.versions:
            raise RuntimeError("pn2: a parameter or buffer of %s was modified in place, or the module "
                               "left eval mode, between the eval-mode forward and its backward (the "
                               "backward recomputes the layer from them)" % type(module).__name__)
        x, = ctx.saved_tensors
        pool, last_relu, rows = ctx.cfg
        params = _mlp_params(ctx.convs, ctx.bns)
        with torch.enable_grad():
            leaf = x.detach().requires_grad_(ctx.needs_input_grad[7])
            out = train.point_mlp_frozen(leaf, ctx.convs, ctx.bns, rows, pool, last_relu)
            wanted = [i for i in range(len(params)) if ctx.needs_input_grad[8 + i]]
            inputs = [params[i] for i in wanted] + ([leaf] if leaf.requires_grad else [])
            got = torch.autograd.grad([out], inputs, [dout.reshape(out.shape)], allow_unused=True)
        grads = [None] * len(params)
        for i, g in zip(wanted, got):
            grads[i] = g
        dx = got[-1] if leaf.requires_grad else None
        return (None,) * 7 + (dx,) + tuple(grads)


def _mlp_params(convs, bns):
    params = []
    for conv, bn in zip(convs, bns):
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    return params


def run_mlp(mode, x, convs, bns, cache, pool=True, last_relu=True, module=None, rows=False):
    """point_mlp ("fused"), train.point_mlp_train ("train") or _V1EvalGrad ("eval_grad") on x:
    channel-first [B, C, N] as the module received it (rows=False), or rows [B, N, C] from a
    previous run_mlp (rows=True).  Same results layout: [B, cout] (pool) or rows [B, N, cout]."""
    if mode == "train":
        return train.point_mlp_train(x, convs, bns, rows, pool, last_relu)
    if mode == "eval_grad":
        return _V1EvalGrad.apply(module, convs, bns, cache, pool, last_relu, rows, x, *_mlp_params(convs, bns))
    return point_mlp(x, convs, bns, cache, pool, last_relu, module, rows)


def apply_transform(module, T, x, rows=False):
    """A T-Net's per-cloud transform of the points: ``torch.bmm(T, x)`` of a channel-first
    x [B, k, N] (pointnet_utils.py:108, 122), ``torch.bmm(x, T^T)`` of rows [B, N, k].  With
    tuning key v1_transform=1, where the forward must be differentiable on float32 device
    tensors with k <= 64, it is train.transform_points (csrc/v1_transform.hip); torch.bmm
    everywhere else."""
    if (tuning.get("v1_transform") == 1 and _needs_autograd(module, x, T) and
            train.transform_eligible(x, T)):
        return train.transform_points(x, T, rows)
    return torch.bmm(x, T.transpose(1, 2)) if rows else torch.bmm(T, x)


def _fold_linear(fc, bn, cache, extra=None):
    """Linear + eval BatchNorm1d folded into one (W', b') in float64, then float32:
    W' = a*W, b' = a*(b - running_mean) + beta (+ extra), a = gamma / sqrt(running_var + eps).
    Cached until a parameter or buffer changes.  None when bn normalises with batch statistics
    (no running stats), which cannot fold."""
    tensors = [fc.weight, fc.bias]
    if bn is not None:
        if bn.running_mean is None or bn.running_var is None:
            return None
        tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    if extra is not None:
        tensors.append(extra)
    key = tuple((t.data_ptr(), t._version) for t in tensors if t is not None)
    if cache.get("key") != key:
        with torch.no_grad():
            W = fc.weight.double()
            b = fc.bias.double() if fc.bias is not None else torch.zeros(W.shape[0], dtype=torch.float64,
                                                                         device=W.device)
            if bn is not None:
                a = torch.rsqrt(bn.running_var.double() + bn.eps)
                if bn.weight is not None:
                    a = a * bn.weight.double()
                W = W * a[:, None]
                b = (b - bn.running_mean.double()) * a
                if bn.bias is not None:
                    b = b + bn.bias.double()
            if extra is not None:
                b = b + extra.double().reshape(-1)
            cache["key"] = key
            cache["wb"] = (W.float().contiguous(), b.float().contiguous())
    return cache["wb"]


def linear_bn(x, fc, bn, cache, relu=True, extra=None):
    """Eval-mode ``relu(bn(fc(x)))`` (``bn`` may be None; ``extra`` a bias added after) as one
    folded GEMM with the ReLU in its epilogue: the v1 FC tails (pointnet_utils.py:33-40, the
    heads' fc / bn_fc) on B rows are launch-bound, and BatchNorm1d's eval kernels cost more than
    the GEMM.  Device tensors run on pn2_linear_rows_f32 (the library GEMMs picked for these
    shapes take 5-13 us; CPU tensors, in tests, on F.linear).  Falls back to the modules when
    the BN cannot fold."""
    wb = _fold_linear(fc, bn, cache, extra) if x.dtype == torch.float32 else None
    if wb is None:  # BN without running statistics, or a non-float32 model: the modules
        y = bn(fc(x)) if bn is not None else fc(x)
        if extra is not None:
            y = y + extra
        return F.relu(y) if relu else y
    if x.is_cuda and x.dim() == 2 and x.shape[0] >= 1 and x.stride(1) == 1:
        return ops.linear_rows(x, wb[0], wb[1], relu)
    y = F.linear(x, wb[0], wb[1])
    return y.relu_() if relu else y


def _rows_to_cf(rows):
    """[B, N, C] rows -> the reference's channel-first [B, C, N] view (no copy)."""
    return rows.permute(0, 2, 1)


def _cf_to_rows(x):
    """[B, C, N] channel-first -> [B, N, C] rows with unit column stride (copy unless it is
    already the permuted view of rows)."""
    r = x.permute(0, 2, 1)
    return r if r.stride(2) == 1 and r.stride(0) == r.shape[1] * r.stride(1) else r.contiguous()


# ----------------------------------------------------------------------------- modules
class _TNet(nn.Module):
    """Shared body of TNet3d / TNetkd (pointnet_utils.py:9-81): conv 64-128-1024 + max, FC
    512-256-k*k, + identity."""

    def _build(self, channel, k):
        self.conv1 = nn.Conv1d(channel, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)
        self._k = k
        self._cache = {}
        self._fc_cache = {}
        # the reference rebuilds eye(k) from numpy and copies it to the device every forward
        # (pointnet_utils.py:37-40); here it is a non-persistent buffer (state_dict unchanged)
        # that moves with the module, so the forward has no host copy and captures in a graph
        self.register_buffer("_iden", torch.from_numpy(np.eye(k).flatten().astype(np.float32)).view(1, k * k),
                             persistent=False)

    def forward(self, x):
        """x: [B, C, N] (any strides: a rows view is read as rows, not copied)."""
        B = x.size()[0]
        convs, bns = [self.conv1, self.conv2, self.conv3], [self.bn1, self.bn2, self.bn3]
        mode = mlp_mode(self, x, convs, bns)
        if mode == "torch":
            h = F.relu(self.bn1(self.conv1(x)))
            h = F.relu(self.bn2(self.conv2(h)))
            h = F.relu(self.bn3(self.conv3(h)))
            g = torch.max(h, 2, keepdim=True)[0].view(-1, 1024)
        else:
            g = run_mlp(mode, x, convs, bns, self._cache, module=self)
        if mode == "fused":  # FC + BN folded, the identity in fc3's bias
            g = linear_bn(g, self.fc1, self.bn4, self._fc_cache.setdefault(1, {}))
            g = linear_bn(g, self.fc2, self.bn5, self._fc_cache.setdefault(2, {}))
            g = linear_bn(g, self.fc3, None, self._fc_cache.setdefault(3, {}), relu=False, extra=self._iden)
            return g.view(-1, self._k, self._k)
        if tuning.get("train_head") == 1:  # the fc_train kernels
            g = train.linear_bn_train(g, self.fc1, self.bn4)
            g = train.linear_bn_train(g, self.fc2, self.bn5)
            g = train.linear_bn_train(g, self.fc3, None, relu=False)
        else:
            g = F.relu(self.bn4(self.fc1(g)))
            g = F.relu(self.bn5(self.fc2(g)))
            g = self.fc3(g)
        g = g + self._iden.expand(B, -1)
        return g.view(-1, self._k, self._k)


class TNet3d(_TNet):
    def __init__(self, channel):
        super(TNet3d, self).__init__()
        self._build(channel, 3)


class TNetkd(_TNet):
    def __init__(self, channel):
        super(TNetkd, self).__init__()
        self._build(channel, channel)
        self.channel = channel


class PointNetEncoder(nn.Module):
    """pointnet_utils.py:83-138 (same submodules, same forward, including its D > 3 branch)."""

    def __init__(self, global_feat=True, channel=3):
        super(PointNetEncoder, self).__init__()
        self.tnet = TNet3d(channel=channel)
        self.ftnet = TNetkd(channel=64)
        self.conv1 = nn.Conv1d(channel, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self._c1, self._c23 = {}, {}

    def forward(self, x):
        B, D, N = x.size()
        transform = self.tnet(x)
        if D > 3:
            normal = x[:, 3:, :]
            x = x[:, :3, :]
        x = apply_transform(self, transform, x)
        if D > 3:
            x = torch.cat([x, normal], dim=2)  # the reference's concatenation axis (:112)
        mode = mlp_mode(self, x, [self.conv1, self.conv2, self.conv3], [self.bn1, self.bn2, self.bn3])
        if mode == "torch":
            x = F.relu(self.bn1(self.conv1(x)))
            trans_feat = self.ftnet(x)
            x = apply_transform(self, trans_feat, x)
            pointfeat = x
            x = F.relu(self.bn2(self.conv2(x)))
            x = self.bn3(self.conv3(x))
            x = torch.max(x, 2, keepdim=True)[0].view(-1, 1024)
        else:
            # conv1 + bn1 + relu per point -> rows [B, N, 64]
            r1 = run_mlp(mode, x, [self.conv1], [self.bn1], self._c1, pool=False, module=self)
            trans_feat = self.ftnet(_rows_to_cf(r1))
            # bmm(trans_feat, x) in the rows layout: x2 rows = x1 rows . trans_feat^T
            r2 = apply_transform(self, trans_feat, r1, rows=True)
            pointfeat = _rows_to_cf(r2)
            # conv2 + bn2 + relu, conv3 + bn3 (no ReLU, :126-127), max over the points
            x = run_mlp(mode, r2, [self.conv2, self.conv3], [self.bn2, self.bn3], self._c23,
                        last_relu=False, module=self, rows=True)
        if self.global_feat:
            return x, transform, trans_feat
        x = x.view(-1, 1024, 1).repeat(1, 1, N)
        return torch.cat([x, pointfeat], 1), transform, trans_feat


def feature_transform_reguliarzer(transform):
    """pointnet_utils.py:140-147 (name kept as spelled in the reference)."""
    d = transform.size()[1]
    if (tuning.get("v1_transform") == 1 and torch.is_grad_enabled() and transform.requires_grad and
            transform.dim() == 3 and transform.is_cuda and transform.dtype == torch.float32 and
            transform.size()[2] == d and 1 <= d <= ops.TRANSFORM_MAX_K):
        return train.orthogonality_loss(transform)  # csrc/v1_transform.hip, every sum in a stated order
    I = torch.eye(d, device=transform.device)[None, :, :]
    return torch.mean(torch.norm(torch.bmm(transform, transform.transpose(2, 1)) - I, dim=(1, 2)))


__all__ = ["TNet3d", "TNetkd", "PointNetEncoder", "feature_transform_reguliarzer", "point_mlp",
           "mlp_mode", "run_mlp", "linear_bn", "apply_transform"]

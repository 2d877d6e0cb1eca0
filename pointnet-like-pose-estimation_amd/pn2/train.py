"""Training path of the SA layers' shared MLP: forward and backward of
(Conv 1x1 -> train-mode BatchNorm -> ReLU)* -> max over the K neighbours on channels-last rows.

Reference: pointnet2_utils.py:167-172 (and the MSG scales :211-221) run under autograd by the
training loops (train_rotation.py:99-133): Conv2d on the [B, C, K, S] grouped tensor,
BatchNorm2d with batch statistics over all B*S*K rows, ReLU, torch.max over K.

Here the rows stay channels-last [M = B*S*K, C] (the grouping's natural layout -- no [B,C,K,S]
permute copies).  The three GEMMs of each layer (Y = X W^T + b, dW = dY^T X, dX = dY W) are plain
library GEMMs (torch.mm -> hipBLASLt) by default; with tuning key train_gemm=1 they are the HIP
kernels of csrc/train_gemm.hip (pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32: split-bf16
products at fp32 accuracy, every sum in a fixed order -- include/pn2.h), so that a layer's step
runs no library arithmetic.  The batch-statistics BatchNorm, ReLU, running-stat update,
max + argmax and their backward are the fused HIP kernels of csrc/train.hip (one pass over the
activations each), called like every other kernel through pn2.ops (bn_train_forward_direct,
bn_relu_apply_direct, group_max_direct, bn_relu_backward_direct: ops.kernel_timer records them,
and their float64 partials live in ops' per-stream workspace).  BatchNorm semantics follow
torch's train mode: biased variance normalises, running_var takes the unbiased one, momentum
None = cumulative average, num_batches_tracked += 1.

The PointNet-v1 shared MLPs (Conv1d 1x1 -> train-mode BatchNorm1d -> ReLU, /root/reference/
model/pointnet_utils.py:31-35, 118-128, and the v1 heads' conv stacks, rotation.py:37-43) are the
same computation on [M = B*N, C] rows with K = N (the max over a cloud's points) or no max at all
(the encoder's per-point conv1); the encoder's conv3 + bn3 before its max has no ReLU
(PN2_LAYER_NO_RELU): point_mlp_train.

Used by the SA modules' and the v1 modules' autograd path when a module is training on a ROCm
device (pn2/pointnet2_utils.py, pn2/pointnet_utils.py, pn2/heads_v1.py).

Frozen mode (mlp_max_frozen): the same rows with eval-mode BatchNorm -- mean = running_mean,
invstd = rsqrt(running_var + eps), constants of the backward (PN2_LAYER_FROZEN_STATS), no
running-stat update, no counter increment.  Hidden layers run pn2_bn_relu_apply_f32; the pooled
last layer runs pn2_bn_relu_group_max_f32, which keeps Y and never writes its activation.  The
SA modules' eval-mode forward under autograd recomputes a layer with it in its backward
(pn2/pointnet2_utils.py); with tuning key v1_eval_grad=1 the v1 modules' eval forward under
autograd does the same on point_mlp_frozen (pn2/pointnet_utils._V1EvalGrad), and keeps the
reference's torch formulation otherwise.

The v1 per-cloud transforms and regulariser (transform_points, orthogonality_loss; tuning key
v1_transform=1): torch.bmm of a T-Net's [B, k, k] output with the points, and
feature_transform_reguliarzer, forward and backward on the kernels of csrc/v1_transform.hip --
float32 fma chains per element, dT from float64 slab partials added in slab order, the
regulariser's norm and mean one float64 chain each (include/pn2.h).

The heads' FC layers (linear_bn_train, tuning key train_head=1): Linear + BatchNorm1d + ReLU of
the FC tails, the translation heads' mean MLP and the T-Nets' tail under autograd, in train mode
(batch statistics) and in eval mode (frozen), one launch forward and one backward
(csrc/fc_train.hip: the whole batch inside one workgroup, float64 column sums in row order),
plus pn2_gemm_nn_f32 for the input gradient.  Batches above pn2_fc_train_max_rows() (64) rows
keep the modules, or with tuning key train_head_rows=1 run the same kernel pair's slab loop
(pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32): the same sums in the same orders.
"""
import torch
import torch.nn.functional as F

from . import ops
from . import tuning


def eligible(grouped, convs, bns):
    """The fused training path covers: device rows, 1x1 convs (Conv2d or Conv1d) with bias,
    affine train-mode BN."""
    if not grouped.is_cuda or grouped.dtype != torch.float32:
        return False
    for conv, bn in zip(convs, bns):
        if conv.bias is None or tuple(conv.weight.shape[2:]) not in ((1, 1), (1,)) or not bn.affine:
            return False
        if not bn.training:
            return False
    return True


def eligible_frozen(grouped, convs, bns):
    """The frozen-statistics path covers: float32 device rows and parameters, 1x1 convs with
    bias, affine eval-mode BN that has running statistics."""
    if not grouped.is_cuda or grouped.dtype != torch.float32:  # non-float32 (or host) rows
        return False
    for conv, bn in zip(convs, bns):
        if conv.bias is None or tuple(conv.weight.shape[2:]) not in ((1, 1), (1,)):
            return False  # convs without bias, or not 1x1
        if not bn.affine:  # non-affine BN: no gamma / beta to pass or to differentiate
            return False
        if bn.training or bn.running_mean is None or bn.running_var is None:
            return False  # BN without running statistics (or in train mode: mlp_max_train's)
        if any(t.dtype != torch.float32 for t in (conv.weight, bn.weight, bn.running_mean)):
            return False  # non-float32 parameters
    return True


def _bn_factor(bn):
    """torch's exponential_average_factor for a train-mode forward (and the counter update)."""
    if not bn.track_running_stats:
        return 0.0
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if bn.momentum is None:
        return 1.0 / float(bn.num_batches_tracked)
    return float(bn.momentum)


def _bn_config(bn, relu, frozen):
    """One layer's BatchNorm configuration for the autograd functions: (eps, momentum factor,
    running_mean, running_var, relu, frozen).  Train mode (frozen False) takes torch's momentum
    factor, counting the batch (_bn_factor), and names the running statistics only when they
    are to be updated; frozen mode reads them and updates nothing."""
    if frozen:
        return (float(bn.eps), 0.0, bn.running_mean, bn.running_var, relu, True)
    mom = _bn_factor(bn)
    return (float(bn.eps), mom, bn.running_mean if mom > 0 else None,
            bn.running_var if mom > 0 else None, relu, False)


_CHUNK = 2048


def _grad_weight(dY, X):
    """dW = dY^T X over M rows.  A single library GEMM of this tall-skinny shape (K = M up to
    5e5, output 64x64) runs on one or two workgroups (780-850 us at SSG sa1, measured); M is cut
    into 2048-row chunks summed after a batched GEMM instead (61-151 us,
    tools/debug/gemm_shapes.py)."""
    M = dY.shape[0]
    q = M // _CHUNK
    if q < 4:
        return torch.mm(dY.t(), X)
    n = q * _CHUNK
    g = torch.bmm(dY[:n].view(q, _CHUNK, -1).transpose(1, 2), X[:n].view(q, _CHUNK, -1)).sum(0)
    if n < M:
        g += torch.mm(dY[n:].t(), X[n:])
    return g


class _MlpMaxTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, K, cfg, *params):
        """x0 [M, Cin] rows; cfg[l] = _bn_config's (eps, momentum factor, running_mean,
        running_var, relu, frozen); params = (W, b, gamma, beta) per layer.  -> [M / K, Cout] max
        over each K rows, or the last layer's [M, Cout] rows when K == 0.  A frozen layer
        normalises with (running_mean, rsqrt(running_var + eps)) and updates nothing."""
        n = len(cfg)
        fixed = ctx.fixed = tuning.get("train_gemm") == 1  # the backward takes the forward's route
        xs, ys, stats = [x0], [], []
        x, pooled = x0, None
        for l in range(n):
            W, b, g, be = params[4 * l:4 * l + 4]
            eps, mom, rm, rv, relu, frozen = cfg[l]
            cout = W.shape[0]
            if fixed:
                Y = ops.gemm_nt_direct(x, W.reshape(cout, -1), b)
            else:
                Y = torch.addmm(b, x, W.reshape(cout, -1).t())
            ys.append(Y)
            if frozen:
                mean, invstd = rm, torch.rsqrt(rv + eps)
                stats += [mean, invstd, None]  # no sxhat: the backward's sums need none
                if l == n - 1 and K:  # max and argmax straight from Y: A is never written
                    pooled, arg = ops.bn_relu_group_max_direct(Y, K, mean, invstd, g, be, relu)
                    continue
                x = ops.bn_relu_apply_direct(Y, mean, invstd, g, be, relu)
            else:
                x, st_mi, sxhat = ops.bn_train_forward_direct(Y, g, be, rm, rv, eps, mom, relu)
                stats += [st_mi[:cout], st_mi[cout:], sxhat]
            if l + 1 < n:
                xs.append(x)
        ctx.K, ctx.n = K, n
        ctx.modes = tuple(c[4:] for c in cfg)  # (relu, frozen) per layer
        if not K:
            ctx.save_for_backward(*xs, *ys, *stats, *params)
            return x
        if pooled is None:
            pooled, arg = ops.group_max_direct(x, K)
        ctx.save_for_backward(*xs, *ys, *stats, arg, *params)
        return pooled

    @staticmethod
    def backward(ctx, dout):
        n, K = ctx.n, ctx.K
        saved = ctx.saved_tensors
        xs = saved[:n]
        ys = saved[n:2 * n]
        stats = saved[2 * n:5 * n]
        arg = saved[5 * n] if K else None
        params = saved[5 * n + (1 if K else 0):]
        dout = dout.contiguous()
        grads = [None] * (4 * n)
        dA = None if K else dout  # K == 0: the rows' gradient is dense
        for l in reversed(range(n)):
            W, b, g, be = params[4 * l:4 * l + 4]
            mean, invstd, sxhat = stats[3 * l:3 * l + 3]
            relu, frozen = ctx.modes[l]
            last = l == n - 1 and K  # the max's layer: dout scattered to the argmax rows
            dY, dgamma, dbeta, dbias = ops.bn_relu_backward_direct(
                ys[l], mean, invstd, g, be, None if last else dA, dout if last else None,
                arg if last else None, K, sxhat, relu, frozen)
            X = xs[l]
            W2 = W.reshape(W.shape[0], -1)
            grads[4 * l] = (ops.gemm_tn_direct(dY, X) if ctx.fixed else _grad_weight(dY, X)).view_as(W)
            grads[4 * l + 1] = dbias  # sum_r dY, from the BN sums (no extra pass over dY)
            grads[4 * l + 2] = dgamma
            grads[4 * l + 3] = dbeta
            if l > 0 or ctx.needs_input_grad[0]:
                dA = ops.gemm_nn_direct(dY, W2) if ctx.fixed else torch.mm(dY, W2)
        return (dA if ctx.needs_input_grad[0] else None, None, None, *grads)


class _GroupTrain(torch.autograd.Function):
    """Grouping with a gradient for the features only (coordinates and centroids carry none in
    the SA layers: they come from index ops of the input).  Forward: pn2_group_f32 (the same
    rows as the reference's index_points + cat, pointnet2_utils.py:107-116 / 204-209);
    backward: the feature rows' gradients added back to their source points (index_add_ --
    atomic adds, instead of advanced indexing's sort-based backward).

    The order rule.  index_add_ on the device is one float atomic add per element: the rows
    that name a point arrive in any order, so the gradient's last bits differ from run to run
    (the only order-dependent sum of the training step).  With tuning key group_backward=1, or
    under torch.use_deterministic_algorithms(True) (where torch would replace index_add_ by
    its sort-based path), the backward is pn2_group_backward_f32 instead: each point's rows
    summed in ascending (s, k) position order from +0.0, one rounding per add -- the bits of
    the reference's CPU backward (a sequential accumulate), the same on every run.  dgrouped is
    read in place through its strides, the feature columns as a slice of its rows."""

    @staticmethod
    def forward(ctx, feature, points, centers, idx, feature_first):
        ctx.save_for_backward(idx)
        ctx.meta = (feature.shape, points.shape[2], bool(feature_first))
        return ops.group_direct(points, feature, centers, idx, feature_first)

    @staticmethod
    def backward(ctx, dgrouped):
        idx, = ctx.saved_tensors
        (B, N, D), C, ff = ctx.meta
        if tuning.get("group_backward") == 1 or torch.are_deterministic_algorithms_enabled():
            return ops.group_backward_direct(dgrouped, idx, N, D, ff), None, None, None, None
        dfeat =dgrouped[..., :D] if ff else dgrouped[..., C:]
        flat = (idx + torch.arange(B, device=idx.device).view(B, 1, 1) * N).reshape(-1)
        out = torch.zeros(B * N, D, device=dgrouped.device, dtype=dgrouped.dtype)
        out.index_add_(0, flat, dfeat.reshape(-1, D))
        return out.view(B, N, D), None, None, None, None


def group_train(points, idx, centers, feature, feature_first):
    """[B,S,K,C+D] grouped rows for the training path (pn2/pointnet2_utils._torch_group's
    contract), or None when this path does not apply (no features needing a gradient, or
    coordinates that need one)."""
    if (feature is None or not feature.requires_grad or points.requires_grad or
            centers.requires_grad or not points.is_cuda):
        return None
    return _GroupTrain.apply(feature, points, centers, idx, feature_first)


def _apply(x0, K, convs, bns, last_relu=True):
    cfg, params = [], []
    n = len(convs)
    for l, (conv, bn) in enumerate(zip(convs, bns)):
        cfg.append(_bn_config(bn, last_relu or l < n - 1, False))
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    return _MlpMaxTrain.apply(x0, K, tuple(cfg), *params)


def mlp_max_frozen(grouped, convs, bns):
    """mlp_max_train's contract with eval-mode (running-statistics) BatchNorm: grouped
    [B, S, K, Cin] -> [B, Cout, S], the reference's ``torch.max(relu(bn(conv(x)))..., 2)[0]`` of
    an eval-mode layer (:167-172), differentiable in the features and the conv / BN parameters.
    Running statistics and num_batches_tracked are read only."""
    B, S, K, Cin = grouped.shape
    x0 = grouped.reshape(B * S * K, Cin)
    if not x0.is_contiguous():
        x0 = x0.contiguous()
    cfg, params = [], []
    for conv, bn in zip(convs, bns):
        cfg.append(_bn_config(bn, True, True))
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    out = _MlpMaxTrain.apply(x0, K, tuple(cfg), *params)
    return out.view(B, S, -1).permute(0, 2, 1)


def mlp_max_train(grouped, convs, bns):
    """grouped [B, S, K, Cin] (any float32 device tensor, autograd-tracked) -> [B, Cout, S]:
    the reference's ``torch.max(relu(bn(conv(x)))..., 2)[0]`` in train mode (:167-172)."""
    B, S, K, Cin = grouped.shape
    x0 = grouped.reshape(B * S * K, Cin)
    if not x0.is_contiguous():
        x0 = x0.contiguous()
    out = _apply(x0, K, convs, bns)
    return out.view(B, S, -1).permute(0, 2, 1)


def point_mlp_train(x, convs, bns, rows, pool=True, last_relu=True):
    """The v1 shared MLP in train mode, pn2.pointnet_utils.point_mlp's contract: x channel-first
    [B, C, N] (rows=False) or per-point rows [B, N, C] (rows=True), autograd-tracked; returns
    the max over the points [B, Cout] (pool) or rows [B, N, Cout].  The reference's
    relu(bn(conv(x)))* (+ torch.max(x, 2)) with Conv1d / BatchNorm1d in train mode
    (pointnet_utils.py:31-35, 118-128); last_relu=False drops the last ReLU (:127)."""
    if rows:
        B, N, C = x.shape
        x0 = x.reshape(B * N, C)
    else:
        B, C, N = x.shape
        x0 = x.permute(0, 2, 1).reshape(B * N, C)
    if not x0.is_contiguous():
        x0 = x0.contiguous()
    out = _apply(x0, N if pool else 0, convs, bns, last_relu)
    return out if pool else out.view(B, N, -1)


def point_mlp_frozen(x, convs, bns, rows, pool=True, last_relu=True):
    """point_mlp_train's contract (rows, pool, last_relu) with eval-mode BatchNorm1d: the running
    statistics normalise and are only read, num_batches_tracked stays (mlp_max_frozen's mode on
    the v1 shared MLPs).  The recompute of the v1 modules' eval forward under autograd
    (pn2/pointnet_utils._V1EvalGrad)."""
    if rows:
        B, N, C = x.shape
        x0 = x.reshape(B * N, C)
    else:
        B, C, N = x.shape
        x0 = x.permute(0, 2, 1).reshape(B * N, C)
    if not x0.is_contiguous():
        x0 = x0.contiguous()
    cfg, params = [], []
    n = len(convs)
    for l, (conv, bn) in enumerate(zip(convs, bns)):
        cfg.append(_bn_config(bn, last_relu or l < n - 1, True))
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
    out = _MlpMaxTrain.apply(x0, N if pool else 0, tuple(cfg), *params)
    return out if pool else out.view(B, N, -1)


class _TransformPoints(torch.autograd.Function):
    """y[b,n,:] = T[b] x[b,n,:] under autograd on the kernels of csrc/v1_transform.hip (forward,
    dx and dT in the orders include/pn2.h states).  Saved for the backward: x and T, nothing
    else."""

    @staticmethod
    def forward(ctx, x, T, rows):
        ctx.rows = rows
        ctx.save_for_backward(x, T)
        return ops.transform_points_direct(x, T, rows)

    @staticmethod
    def backward(ctx, dy):
        x, T = ctx.saved_tensors
        dx, dT = ops.transform_points_backward_direct(dy, x, T, ctx.rows, ctx.needs_input_grad[0],
                                                      ctx.needs_input_grad[1])
        return dx, dT, None


def transform_eligible(x, T):
    """What transform_points covers: float32 device tensors and k <= 64."""
    return (x.is_cuda and T.is_cuda and x.dtype == torch.float32 and T.dtype == torch.float32 and
            1 <= T.shape[-1] <= ops.TRANSFORM_MAX_K)


def transform_points(x, T, rows):
    """The v1 networks' per-cloud transform under autograd: x rows [B, N, k] (rows=True;
    ``torch.bmm(x, T.transpose(1, 2))``) or channel-first [B, k, N] (rows=False;
    ``torch.bmm(T, x)``, pointnet_utils.py:108, 122), T [B, k, k] -> the transformed points in
    x's layout.  Strided views are read in place."""
    return _TransformPoints.apply(x, T, bool(rows))


class _OrthoReg(torch.autograd.Function):
    """feature_transform_reguliarzer (pointnet_utils.py:140-147) on pn2_orthogonality_forward_f32
    / _backward_f32.  Saved for the backward: T and the per-cloud norms."""

    @staticmethod
    def forward(ctx, T):
        loss, norm, _ = ops.orthogonality_forward_direct(T)
        ctx.save_for_backward(T, norm)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        T, norm = ctx.saved_tensors
        return ops.orthogonality_backward_direct(T, norm, dloss.contiguous())


def orthogonality_loss(T):
    """mean_b ||T[b] T[b]^T - I||_F of T [B, k, k] (k <= 64, float32 on the device) under
    autograd, every sum in a stated order (include/pn2.h)."""
    return _OrthoReg.apply(T)


class _FcBnTrain(torch.autograd.Function):
    """One FC layer of a head under autograd: Linear (+ BatchNorm1d with batch or frozen
    statistics) (+ ReLU) as pn2_fc_bn_forward_f32, its backward as pn2_fc_bn_backward_f32 plus
    pn2_gemm_nn_f32 for the input gradient -- every sum in a fixed order (include/pn2.h).  The
    ops take the two entries' any-B forms above ops.fc_train_max_rows() rows.  Saved for the
    backward: x, Y, stats and the parameters, nothing else (A is recomputed)."""

    @staticmethod
    def forward(ctx, x, cfg, W, b, g, be):
        """cfg = (eps, momentum factor, running_mean, running_var, relu, frozen); g / be None:
        no BatchNorm."""
        eps, mom, rm, rv, relu, frozen = cfg
        Y, A, stats = ops.fc_bn_forward_direct(x, W, b, g, be, rm, rv, eps, mom, relu, frozen)
        ctx.relu, ctx.frozen, ctx.bn = relu, frozen, g is not None
        if ctx.bn:
            ctx.save_for_backward(x, Y, W, stats, g, be)
        else:
            ctx.save_for_backward(x, Y, W)
        return A

    @staticmethod
    def backward(ctx, dA):
        if ctx.bn:
            x, Y, W, stats, g, be = ctx.saved_tensors
        else:
            (x, Y, W), stats, g, be = ctx.saved_tensors, None, None, None
        dY, dW, db, dg, dbe = ops.fc_bn_backward_direct(dA, Y, x, stats, g, be, ctx.relu, ctx.frozen)
        dx = ops.gemm_nn_direct(dY, W) if ctx.needs_input_grad[0] else None
        return dx, None, dW, db, dg, dbe


def linear_bn_train(x, fc, bn, relu=True):
    """act(bn(fc(x))) for a head's FC layer under autograd -- ``F.relu(bn(fc(x)))`` of the
    reference's tails (pointnet2_cls_ssg.py:32-35), ``fc(x)`` alone with bn=None, relu=False --
    on the kernels of csrc/fc_train.hip.  The BN mode is the module's: training = batch
    statistics (running statistics and num_batches_tracked updated as torch does), eval =
    frozen running statistics.  Up to pn2_fc_train_max_rows() (64) rows run the kernel pair's
    one-slab instantiation; more rows run its slab loop (pn2_fc_bn_forward_rows_f32 /
    pn2_fc_bn_backward_rows_f32, the same sums in the same orders) when the tuning keys
    train_head and train_head_rows are both 1, and fall back to the modules otherwise.  Falls back to the modules as well for what
    no kernel covers: non-float32 or host tensors, a Linear without bias, a non-affine BN, an
    eval-mode BN without running statistics; and for a train-mode BN on a single row, where the
    modules raise their ValueError."""
    ok = (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and fc.bias is not None and
          fc.weight.dtype == torch.float32 and x.shape[0] >= 1)
    if ok and x.shape[0] > ops.fc_train_max_rows():
        ok = tuning.get("train_head") == 1 and tuning.get("train_head_rows") == 1
    if ok and bn is not None:
        ok = bn.affine and bn.weight.dtype == torch.float32
        if bn.training:
            ok = ok and x.shape[0] > 1
        else:
            ok = ok and bn.running_mean is not None and bn.running_var is not None
    if not ok:
        y = fc(x) if bn is None else bn(fc(x))
        return F.relu(y) if relu else y
    if bn is None:
        cfg = (0.0, 0.0, None, None, relu, False)
        return _FcBnTrain.apply(x, cfg, fc.weight, fc.bias, None, None)
    return _FcBnTrain.apply(x, _bn_config(bn, relu, not bn.training), fc.weight, fc.bias, bn.weight, bn.bias)


__all__ = ["mlp_max_train", "mlp_max_frozen", "point_mlp_train", "point_mlp_frozen", "group_train", "eligible",
           "eligible_frozen", "linear_bn_train", "transform_points", "transform_eligible", "orthogonality_loss"]

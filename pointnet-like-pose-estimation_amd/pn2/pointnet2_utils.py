"""Drop-in replacement for /root/reference/model/pointnet2_utils.py on MI355X.

Same public names, signatures, return shapes, ``state_dict`` keys and CPU-RNG consumption as
the reference, so its heads (pointnet2_cls_ssg/msg, rotation_/translation_/sign_*) run
unchanged when this module is importable as ``pointnet2_utils`` (see the shim
``pointnet-like-pose-estimation_amd/pointnet2_utils.py``).

Eval-mode inference (``model.eval()`` / no autograd) of an SA layer is three HIP launches
(FPS and ball query on the geometry stream, see geometry.py, overlapping the previous layer's
MLP):
  pn2::fps            FPS + gathered centroids + packed (coords, ssq) records
  pn2::ball_query     first-K-in-radius neighbour indices
  pn2::sa_mlp_max_    fused gather -> conv1x1/BN/ReLU chain -> max over neighbours
(the last one per scale; an MSG layer's ball queries are one launch over its radii).  Hidden
activations stay in registers (the chain kernel) or pass through an HBM workspace between the
dense-layer launches (group_all layers); the per-layer ``[B, C, K, S]`` tensors of the
reference are never materialised.

The two modules are the reference's constructors over one layer body (_SetAbstraction) written
over the module's list of scales; whatever else needs a layer's scales (_ball_queries,
_eval_grad_route, pn2.pipeline) reads ``_scales()`` too, never the class.

Training (``model.train()`` or autograd through the weights) keeps the reference's semantics
(batch-statistics BatchNorm, autograd through the MLP and the feature gather): FPS and the ball
query still run as HIP kernels (they are index ops with no gradient); in train mode the
grouping and the MLP + max run forward and backward on the training kernels of pn2/train.py
(csrc/train.hip around library GEMMs).  As in the reference, an eval-mode forward with
autograd enabled (``model.eval()`` without ``torch.no_grad()``, parameters requiring grad: the
mutilthreading/predict_test.py pattern, or fine-tuning with frozen BatchNorm) is
differentiable.  Its forward is the fused forward above -- the launches, the CPU-RNG draws and
the bits of the no_grad forward -- inside an autograd Function (_SaEvalGrad) that saves the
inputs, the centroids and the neighbour lists, no activation; its backward recomputes the layer
on the frozen-statistics training kernels (train.mlp_max_frozen) and gives the gradients of
the reference's eval formulation to the conv / BN parameters and the input feature.  The torch
device formulation remains for what that route does not cover (_eval_grad_route) and under
tuning ``eval_grad=0``.  Inside ``pn2.fused_eval()`` the fused forward runs without autograd
history.

Device tensors only -- the reference's CPU execution is not re-implemented here.
"""
import contextlib
import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import geometry
from . import ops
from . import shard
from . import train
from . import tuning


# ----------------------------------------------------------------------------- helpers
def _draw_start(B, N, device):
    """The reference's FPS start draw: torch.randint(0, N, (B,), dtype=long) on the CPU default
    generator (pointnet2_utils.py:59) -- one draw per FPS call, sliced when sharded.  A CPU
    tensor (ops.fps_direct passes host starts in the launch's arguments), or a device slot under
    graph capture."""
    return shard.host_start(B, N, device)


def _fps_ahead(module, new_points, live=False):
    """The side job that runs the next SA layer's FPS (geometry.fps_ahead) on this layer's
    centroids `new_points` [B, S, C] inside this layer's MLP call, or None: registered so the next
    layer's forward takes its results instead of sampling.  live: this layer runs inside
    _SaEvalGrad (autograd is on around it and its output will require grad, so the next layer's
    forward is a differentiable one); the next layer then takes the results only on that route
    too -- the torch formulation samples for itself."""
    nxt = geometry.ahead_of(module)
    if nxt is None or getattr(nxt, "group_all", False) or nxt.point_number is None:
        return None
    if (live or _needs_autograd(nxt, new_points)) and not _eval_grad_route(nxt, new_points, None):
        return None
    if shard.recording():  # (graph records: device starts)
        return None
    B, N, _ = new_points.shape
    start = shard.host_start(B, N, new_points.device)
    job, (_, newp, cpk, ppk) = ops.fps_side_job(new_points, nxt.point_number, start)
    geometry.put_ahead(nxt, new_points, newp, cpk, ppk)
    return job


def msg_ball_queries(ppk, cpk, C, radii, nsamples):
    """The ball queries of an MSG layer's scales (pointnet2_utils.py:197-203): one launch over
    all radii (ops.ball_query_multi_direct; host tuning bq_multi = 0: one call per radius), the
    same (int32 lists, counts) per radius either way."""
    if len(radii) > 1 and tuning.get("bq_multi"):
        return ops.ball_query_multi_direct(ppk, cpk, C, radii, nsamples)
    return [ops.ball_query_direct(ppk, cpk, C, r, k, True) for r, k in zip(radii, nsamples)]


def _ball_queries(module, ppk, cpk, C):
    """The ball queries of an SA module's scales on packed points / centroids (the module body
    and pn2.pipeline's geometry pre-computation) -> [(int32 lists, counts)] per scale."""
    scales = module._scales()
    return msg_ball_queries(ppk, cpk, C, [s[0] for s in scales], [s[1] for s in scales])


def _cat_scales(outs):
    """The scales' [B, Cout, S] outputs as one (:221); a single scale's is returned as it is."""
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)


def _channels_last(feature):
    """[B, D, N] feature -> a [B, N, D] view with unit channel stride (copy only if needed)."""
    f = feature.permute(0, 2, 1)
    return f if f.stride(2) == 1 else f.contiguous()


def _precision(module):
    """The module's MLP arithmetic: its own ``mlp_precision`` if set, else the thread's
    ``pn2.ops.mlp_precision`` context ("fp32" unless changed)."""
    p = getattr(module, "mlp_precision", None)
    return ops.current_precision() if p is None else p


_fused = threading.local()


@contextlib.contextmanager
def fused_eval(enabled=True):
    """Within this context (this thread) eval-mode forwards run the fused inference kernels even
    with autograd enabled (``model.eval()`` without ``torch.no_grad()``, the
    mutilthreading/predict_test.py pattern): the no_grad bits, no autograd history (a backward
    through the outputs finds nothing that requires grad).  Outside it such a forward is
    differentiable, as in the reference (the SA layers with the same bits, _SaEvalGrad)."""
    prev = getattr(_fused, "on", False)
    _fused.on = bool(enabled)
    try:
        yield
    finally:
        _fused.on = prev


@contextlib.contextmanager
def eval_autograd(enabled=True):
    """Round-2 name kept for callers: eval-mode forwards with autograd enabled are
    differentiable (the default now); ``enabled=False`` is ``fused_eval()``."""
    prev = getattr(_fused, "reference", False)
    _fused.reference = bool(enabled)  # the v1 modules keep the reference's formulation inside it
    try:
        with fused_eval(not enabled):
            yield
    finally:
        _fused.reference = prev


def _in_eval_autograd():
    """Whether this thread is inside ``eval_autograd()``."""
    return getattr(_fused, "reference", False)


def _needs_autograd(module, *tensors):
    """Whether a forward must be differentiable: training mode, or autograd on (outside
    ``fused_eval()``) with an input or a parameter that needs a gradient -- the reference's
    eval forward is differentiable whenever autograd is."""
    if module.training:
        return True
    if not torch.is_grad_enabled() or getattr(_fused, "on", False):
        return False
    if any(t is not None and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in module.parameters())


def _eval_grad_route(module, points, feature):
    """Whether an eval-mode SA forward that must be differentiable runs the fused inference
    kernels with the recompute backward (_SaEvalGrad).  Everything else stays the reference's
    torch formulation (_forward_autograd)."""
    if module.training or not tuning.get("eval_grad"):  # eval_grad=0: the torch formulation
        return False
    if points.requires_grad:  # coordinates that need a gradient: torch gathers carry it
        return False
    if not points.is_cuda or any(t is not None and t.dtype != torch.float32 for t in (points, feature)):
        return False  # non-float32 tensors (or host tensors): torch formulation
    if _precision(module) != "fp32":  # bf16 forward: the float32 recompute is another function
        return False
    blocks = [(convs, bns) for _, _, convs, bns, _ in module._scales()]
    for convs, _ in blocks:  # shapes the fused MLP entry rejects (widths not x32, > 4 layers)
        if not ops.sa_mlp_supported(c.weight.shape[0] for c in convs):
            return False
    # non-float32 parameters, BN without running statistics or affine, convs without bias or
    # not 1x1 (train.eligible_frozen names each): torch formulation
    return all(train.eligible_frozen(points, convs, bns) for convs, bns in blocks)


def _frozen_group(points, idx, centers, feature, feature_first):
    """The grouped rows of the recompute from the forward's int32 neighbour lists: with the
    index_add_ backward when the features need a gradient, else the plain grouping kernel."""
    idx = idx.long()
    g = train.group_train(points, idx, centers, feature, feature_first)
    return g if g is not None else ops.group_direct(points, feature, centers, idx, feature_first)


def _versions(module):
    """What _SaEvalGrad's recompute reads besides the saved tensors: the in-place versions of the
    parameters and the BatchNorm buffers, and the eval flags."""
    return (tuple(p._version for p in module.parameters()) + tuple(b._version for b in module.buffers()) +
            tuple(m.training for m in module.modules()))


class _SaEvalGrad(torch.autograd.Function):
    """An SA module's eval-mode forward under autograd: the forward is the module's fused body
    (the launches, the CPU-RNG draws and the bits of the no_grad forward); nothing of the MLP is
    saved -- only the inputs, the centroids and the neighbour lists the forward made.  The
    backward recomputes the layer from those on the frozen-statistics training kernels
    (train.mlp_max_frozen: library GEMMs + csrc/train.hip) and backpropagates through that:
    gradients of the reference's eval formulation (pointnet2_utils.py:163-172 / :211-221 with
    BatchNorm2d on its running statistics) for the conv / BN parameters and the input feature.
    FPS and ball query are not re-run and no RNG draw is taken."""

    @staticmethod
    def forward(ctx, module, points, feature, *params):
        new_points, out, centers, idxs = module._fused_body(points, feature, live=True)
        ctx.module = module  # parameter references: the recompute reads the live parameters
        ctx.versions = _versions(module)
        ctx.save_for_backward(points, feature, centers, *idxs)
        ctx.mark_non_differentiable(new_points)
        return new_points, out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _dnew_points, dout):
        module = ctx.module
        params = list(module.parameters())
        if _versions(module) != ctx.versions:
            raise RuntimeError("pn2: a parameter or buffer of %s was modified in place, or the module "
                               "left eval mode, between the eval-mode forward and its backward (the "
                               "backward recomputes the layer from them)" % type(module).__name__)
        points, feature, centers, *idxs = ctx.saved_tensors
        with torch.enable_grad():
            leaf = None
            if feature is not None:
                leaf = feature.detach().requires_grad_(ctx.needs_input_grad[2])
            out = module._recompute(points.detach(), leaf, centers, idxs)  # [B, Cout, S]
            B, cout, S = out.shape
            wanted = [i for i, p in enumerate(params) if ctx.needs_input_grad[3 + i]]
            inputs = [params[i] for i in wanted]
            if leaf is not None and leaf.requires_grad:
                inputs.append(leaf)
            got = torch.autograd.grad([out], inputs, [dout.reshape(B, S, cout).permute(0, 2, 1)],
                                      allow_unused=True)
        grads = [None] * len(params)
        for i, g in zip(wanted, got):
            grads[i] = g
        dfeat = got[-1] if len(inputs) > len(wanted) else None
        return (None, None, dfeat, *grads)


def _eval_grad_forward(module, points, feature):
    new_points, out = _SaEvalGrad.apply(module, points, feature, *module.parameters())
    return module._views(new_points, out)


_SPLIT_MAX_XYZ = 16  # point channels of a split-bf16 first layer (csrc/sa_chain.hip)


def _pack_chain(convs, bns, cache, rot0, xyz=0, xyz_first=True):
    """Fold each Conv2d-1x1 + eval BatchNorm2d into (W^T, alpha, beta) for the fp32 kernels and
    the split-bf16 image for the chain kernel; cached until any parameter/buffer changes
    (data_ptr or in-place version).  rot0: xyz channels leading the first layer's input in the
    reference's order (the fp32 kernels put them behind the features); xyz / xyz_first: the
    first layer's xyz channel count and order for the chain kernel (rows [xyz | features]).
    Points with more than 16 channels get no split images: the split-bf16 kernels hold at most
    16 point channels (pn2_layer_split_kblocks), so those layers run the fp32 kernels only and
    precision "bf16" fails loudly for them (sa_mlp_max_impl)."""
    tensors = []
    for conv, bn in zip(convs, bns):
        tensors += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    key = (rot0, xyz, xyz_first) + tuple((None if t is None else (t.data_ptr(), t._version))
                                         for t in tensors)
    if cache.get("key") != key:
        wts, als, bes, cins, splits = [], [], [], [], []
        with torch.no_grad():
            for li, (conv, bn) in enumerate(zip(convs, bns)):
                rot = rot0 if li == 0 else 0
                wt, al, be = ops.pack_layer_direct(conv.weight, conv.bias, bn.weight, bn.bias,
                                            bn.running_mean, bn.running_var, float(bn.eps), rot)
                wts.append(wt)
                als.append(al)
                bes.append(be)
                cins.append(conv.weight.shape[1])
                if xyz <= _SPLIT_MAX_XYZ:
                    splits.append(ops.pack_layer_split_direct(conv.weight, xyz if li == 0 else 0,
                                                              xyz_first))
        cache["key"] = key
        cache["layers"] = (wts, als, bes, cins, splits)
    return cache["layers"]


def _torch_group(points, idx, centers, feature, feature_first):
    """Differentiable grouping for the training path: the HIP grouping kernel with an
    index_add_ backward for the features (pn2/train.py), or torch device gathers when the
    coordinates need a gradient too."""
    g = train.group_train(points, idx, centers, feature, feature_first)
    if g is not None:
        return g
    B = points.shape[0]
    b = torch.arange(B, device=points.device).view(B, 1, 1)
    g = points[b, idx, :] - centers.unsqueeze(2)
    if feature is None:
        return g
    f = feature[b, idx, :]
    return torch.cat([f, g] if feature_first else [g, f], dim=-1)


def _torch_mlp_max(grouped, convs, bns):
    """grouped [B,S,K,C] -> [B, Cout, S].  Training on the device: the fused batch-statistics
    BN / ReLU / max kernels around library GEMMs (pn2/train.py); otherwise (eval with autograd
    where _eval_grad_route does not apply, exotic BN configs) the reference's torch formulation."""
    if train.eligible(grouped, convs, bns):
        return train.mlp_max_train(grouped, convs, bns)
    x = grouped.permute(0, 3, 2, 1)  # [B, C, K, S] as the reference (:167)
    for conv, bn in zip(convs, bns):
        x = F.relu(bn(conv(x)))
    return torch.max(x, 2)[0]


# ----------------------------------------------------------------------------- public functions
def square_distance(src, dst):
    """pointnet2_utils.py:5-26 -> [B, N, M], bit-identical to the reference's float32 result."""
    C = src.shape[-1]
    return ops.square_distance_direct(ops.pack_points_direct(src), ops.pack_points_direct(dst), C)


def index_points(points, idx):
    """pointnet2_utils.py:28-45: points [B,N,C], idx [B, ...] -> [B, ..., C]."""
    B = points.shape[0]
    out = ops.index_points_direct(points, idx.reshape(B, -1))
    return out.view(*idx.shape, points.shape[-1])


def farthest_point_sample(points, number):
    """pointnet2_utils.py:47-68: [B,N,C] -> [B, number] int64 (consumes one CPU randint)."""
    B, N, _ = points.shape
    return ops.fps_direct(points, number, _draw_start(B, N, points.device))[0]


def query_ball_point(radius, number, points, new_points):
    """pointnet2_utils.py:70-90: [B,S,number] int64; IndexError if number > N (as the
    reference)."""
    C = points.shape[-1]
    return ops.ball_query_direct(ops.pack_points_direct(points), ops.pack_points_direct(new_points),
                                 C, radius, number)


def sample_and_group(points, feature, point_number, sample_number, radius, returnfps=False):
    """pointnet2_utils.py:92-120.  points [B,N,C], feature [B,N,D] or None."""
    B, N, C = points.shape
    fps_idx, new_points, cpk, ppk = ops.fps_direct(points, point_number, _draw_start(B, N, points.device))
    idx = ops.ball_query_direct(ppk, cpk, C, radius, sample_number)
    new_feature = ops.group_direct(points, feature, new_points, idx, False)
    if returnfps:
        grouped = index_points(feature if feature is not None else points, idx)
        return new_points, new_feature, grouped, fps_idx
    return new_points, new_feature


def sample_and_group_all(points, feature):
    """pointnet2_utils.py:122-141: centroid at the origin, raw xyz (not centred) first."""
    B, N, C = points.shape
    new_points = torch.zeros(B, 1, C, device=points.device, dtype=points.dtype)
    grouped = points.reshape(B, 1, N, C)
    if feature is not None:
        return new_points, torch.cat([grouped, feature.reshape(B, 1, N, -1)], dim=-1)
    return new_points, grouped


# ----------------------------------------------------------------------------- modules
class _SetAbstraction(nn.Module):
    """The layer body of both SA modules, written over the module's scales.  A module gives
    ``_scales()`` -> [(radius, nsample, convs, bns, pack cache)] (one entry for SSG, one per
    radius for MSG; read from the live attributes on every call) and its grouped-row order:
    ``_xyz_first`` (the reference's rows are [xyz | feature] in SSG, :114 / :139, and
    [feature | xyz] in MSG, :209) with the fused kernels' source mode ``_src`` for it."""

    group_all = False

    def forward(self, points, feature):
        """points [B,C,N], feature [B,D,N] or None -> (new_points [B,C,S], new_feature
        [B, sum of mlp[-1] over the scales, S]).  Both outputs are channel-first views of
        channels-last buffers."""
        if _needs_autograd(self, points, feature):
            if _eval_grad_route(self, points, feature):
                return _eval_grad_forward(self, points, feature)
            return self._forward_autograd(points, feature)
        new_points, out, _, _ = self._fused_body(points, feature)
        return self._views(new_points, out)

    def _views(self, new_points, out):
        """The fused body's buffers as the forward's channel-first outputs."""
        B, cout = new_points.shape[0], out.shape[-1]
        if self.group_all:
            return new_points, out.view(B, 1, cout).permute(0, 2, 1)
        return new_points.permute(0, 2, 1), out.view(B, -1, cout).permute(0, 2, 1)

    def _fused_body(self, points, feature, live=False):
        """The fused inference launches of all scales (the no_grad forward and _SaEvalGrad's
        forward) -> (new_points buffer, out rows, centroids [B,S,C] or None, [int32 neighbour
        lists per scale])."""
        pts = points.permute(0, 2, 1)
        feat = None if feature is None else _channels_last(feature)
        B, N, C = pts.shape
        dev = pts.device
        scales = self._scales()
        # the fp32 kernels read [feature | xyz]: leading xyz channels rotate behind the features;
        # the split-bf16 rows keep the module's order (group_all layers too)
        rot0 = C if self._xyz_first and feat is not None else 0
        chains = [_pack_chain(convs, bns, cache, rot0, C, self._xyz_first)
                  for _, _, convs, bns, cache in scales]
        total = sum(ch[0][-1].shape[1] for ch in chains)
        if self.group_all:
            wts, als, bes, cins, splits = chains[0]
            out = torch.empty(B, total, device=dev, dtype=torch.float32)
            # new_points = the reference's zeros (:136), filled by the MLP's last launch
            new_points = torch.empty(B, C, 1, device=dev, dtype=torch.float32)
            ops.sa_mlp_max_direct(out, _lib.SRC_GROUP_ALL, pts, feat, None, None, wts, als, bes, cins,
                                  splits, _precision(self), zero=new_points)
            return new_points, out, None, []
        S = self.point_number
        pre = geometry.take(self, pts)  # FPS (+ ball queries) precomputed by pn2.pipeline
        if pre is not None:
            new_points, cpk, ppk, idxs = pre
            if not idxs:
                idxs = _ball_queries(self, ppk, cpk, C)
        else:
            with geometry.Span(dev, [pts]) as span:  # overlaps the previous layer's MLP
                _, new_points, cpk, ppk = ops.fps_direct(pts, S, _draw_start(B, N, dev))
                idxs = _ball_queries(self, ppk, cpk, C)
            span.finish([new_points], [new_points] + [t for ic in idxs for t in ic])
        out = torch.empty(B * S, total, device=dev, dtype=torch.float32)
        prec = _precision(self)
        col = 0
        side = _fps_ahead(self, new_points, live)  # rides on the longest scale's launch (largest K)
        longest = max(range(len(scales)), key=lambda i: scales[i][1])
        for i, (idx, cnt) in enumerate(idxs):
            wts, als, bes, cins, splits = chains[i]
            cout = wts[-1].shape[1]
            ops.sa_mlp_max_impl(out[:, col:col + cout], self._src, pts, feat, new_points, idx, wts,
                                als, bes, cins, splits, prec, cnt=cnt,
                                fps_side=side if i == longest else None)
            col += cout
        return new_points, out, new_points, [idx for idx, _ in idxs]

    def _recompute(self, points, feature, centers, idxs):
        """Every scale again from the forward's centroids and lists, differentiable in `feature`
        and the parameters, on the frozen-statistics training kernels (one Function for the
        module: autograd sums the scales' feature gradients) -> [B, sum Cout, S]."""
        pts = points.permute(0, 2, 1)
        feat = None if feature is None else feature.permute(0, 2, 1)
        scales = self._scales()
        if self.group_all:  # plain rows in the reference's [xyz | feature] order (:139)
            _, _, convs, bns, _ = scales[0]
            return train.mlp_max_frozen(sample_and_group_all(pts, feat)[1], convs, bns)
        outs = []
        for idx, (_, _, convs, bns, _) in zip(idxs, scales):
            grouped = _frozen_group(pts, idx, centers, feat, not self._xyz_first)
            outs.append(train.mlp_max_frozen(grouped, convs, bns))
        return _cat_scales(outs)

    def _forward_autograd(self, points, feature):
        """The torch formulation (training, and what _eval_grad_route leaves to it): FPS and the
        ball queries as HIP kernels, grouping and MLP + max under autograd."""
        pts = points.permute(0, 2, 1)
        feat = None if feature is None else feature.permute(0, 2, 1)
        scales = self._scales()
        if self.group_all:
            _, _, convs, bns, _ = scales[0]
            new_points, grouped = sample_and_group_all(pts, feat)
            return new_points.permute(0, 2, 1), _torch_mlp_max(grouped, convs, bns)
        B, N, C = pts.shape
        _, new_points, cpk, ppk = ops.fps_direct(pts.detach(), self.point_number,
                                                 _draw_start(B, N, pts.device))
        outs = []
        for radius, nsample, convs, bns, _ in scales:
            idx = ops.ball_query_direct(ppk, cpk, C, radius, nsample)
            grouped = _torch_group(pts, idx, new_points, feat, not self._xyz_first)
            outs.append(_torch_mlp_max(grouped, convs, bns))
        return new_points.permute(0, 2, 1), _cat_scales(outs)


class PointNetSetAbstraction(_SetAbstraction):
    """pointnet2_utils.py:143-174 (same ctor, submodule names and forward contract)."""

    _xyz_first, _src = True, _lib.SRC_GROUP_XYZ_FIRST

    def __init__(self, point_number, sample_number, radius, in_channel, mlp, group_all=False):
        super(PointNetSetAbstraction, self).__init__()
        self.point_number = point_number
        self.radius = radius
        self.sample_number = sample_number
        self.group_all = group_all
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last = out_channel
        self._pack_cache = {}
        self.mlp_precision = None  # None: ops.mlp_precision context ("fp32" by default)

    def _scales(self):
        return [(self.radius, self.sample_number, self.mlp_convs, self.mlp_bns, self._pack_cache)]


class PointNetSetAbstractionMsg(_SetAbstraction):
    """pointnet2_utils.py:176-223 (same ctor, submodule names and forward contract)."""

    _xyz_first, _src = False, _lib.SRC_GROUP_FEAT_FIRST

    def __init__(self, point_number, sample_number_list, radius_list, in_channel, mlp_list,
                 num_category=0):
        super(PointNetSetAbstractionMsg, self).__init__()
        self.point_number = point_number
        self.radius_list = radius_list
        self.sample_number_list = sample_number_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for widths in mlp_list:
            convs = nn.ModuleList()
            bns = nn.ModuleList()
            last = in_channel + 3 + num_category
            for out_channel in widths:
                convs.append(nn.Conv2d(last, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel))
                last = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)
        self._pack_cache = [{} for _ in mlp_list]
        self.mlp_precision = None  # None: ops.mlp_precision context ("fp32" by default)

    def _scales(self):
        return list(zip(self.radius_list, self.sample_number_list, self.conv_blocks, self.bn_blocks,
                        self._pack_cache))


__all__ = [
    "square_distance", "index_points", "farthest_point_sample", "query_ball_point",
    "sample_and_group", "sample_and_group_all", "PointNetSetAbstraction",
    "PointNetSetAbstractionMsg",
]

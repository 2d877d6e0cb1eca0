"""PyTorch custom ops (namespace ``pn2``) over the libpn2.so C ABI.

Each op takes/returns torch tensors, checks shapes in Python (raising the exception the
reference raises for the same misuse), and calls the HIP entry point asynchronously on torch's
current stream.  ``<op>_direct`` is the same function without the torch.library dispatcher
(the SA modules' eager path calls it: the dispatcher costs more host time per call than the
kernels it launches take on the GPU at these sizes).  Device tensors only: there is no CPU implementation and no fallback -- a CPU
tensor or a missing library is an error.

Ops (reference code each replaces, in /root/reference/model/pointnet2_utils.py):
  pn2::fps            farthest_point_sample :47-68 (+ index_points of the samples, :106)
  pn2::pack_points    the torch.sum(points**2, -1) terms of square_distance :24-25
  pn2::ball_query     query_ball_point :70-90
  pn2::square_distance square_distance :5-26
  pn2::index_points   index_points :28-45
  pn2::group          grouping in sample_and_group :107-116 / the MSG module :204-209
  pn2::group_backward the feature gradient of that grouping (autograd's backward of
                      index_points :44), summed per point in position order
  pn2::gemm_nt / gemm_nn / gemm_tn  the shared MLP's 1x1 convs under autograd :167-172 (forward,
                      input gradient, weight gradient), every sum in a fixed order
  pn2::pack_layer     Conv2d 1x1 + BatchNorm2d (eval) parameters :150-156, :184-193
  pn2::sa_mlp_max_    gathered shared MLP + max :167-172, :211-218 (writes into `out`)
  bn_train_forward_direct / bn_relu_apply_direct / group_max_direct / bn_relu_backward_direct
                      (no dispatcher op) train-mode BatchNorm2d + ReLU + torch.max :169-172 and
                      their backward on channels-last rows, around the GEMMs above
  log_softmax_rows_direct / criterion_forward_direct / criterion_backward_direct /
  meter_update_direct (no dispatcher op) F.log_softmax and the get_loss classes under autograd
                      (model/pointnet2_cls_ssg.py:36, 40-47, rotation_ssg.py:40-50,
                      sign_ssg.py:38-45) and the test loops' per-class bookkeeping
                      (train_rotation.py:157-163), every sum in a fixed order
  pn2::transform_points / transform_points_backward  torch.bmm of a T-Net's transform with the
                      points under autograd (model/pointnet_utils.py:102-113,
                      120-123; pose.py:50-69), forward, dx and dT in stated orders
  pn2::orthogonality_forward / orthogonality_backward  feature_transform_reguliarzer
                      (pointnet_utils.py:140-147) and its gradient
  pn2::bn_relu_group_max  eval BatchNorm2d + ReLU + torch.max of the last MLP layer :170-172 on
                      channels-last rows (the recompute of pn2.train's frozen mode)
"""
import contextlib
import ctypes
import threading
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import MlpLayer, SaSrc, check, load

_L = load()  # fail at import, loudly, if the native library is unavailable

# ------------------------------------------------------------------------------ MLP precision
# "fp32": the reference's arithmetic (split-bf16 products at fp32 accuracy, or fp32 MFMA);
# "bf16": bf16 operands, fp32 accumulation (BASELINE config 5) -- an explicit caller choice.
PRECISIONS = ("fp32", "bf16")
_prec = threading.local()


def current_precision() -> str:
    return getattr(_prec, "value", "fp32")


@contextlib.contextmanager
def mlp_precision(precision: str):
    """Within this context (this thread) SA modules without their own ``mlp_precision``
    attribute run their shared MLPs at `precision` ("fp32" or "bf16")."""
    if precision not in PRECISIONS:
        raise ValueError("pn2: precision must be one of %s, got %r" % (PRECISIONS, precision))
    prev = current_precision()
    _prec.value = precision
    try:
        yield
    finally:
        _prec.value = prev


class KernelTimer:
    """HIP-event timing of every libpn2 launch, recorded on the stream the launch is issued on
    (torch's current stream), with each launch's algorithmic FLOPs / bytes and, for the MLP
    calls, the planes per operand its kernels ran with (pn2_sa_mlp_last_planes)."""

    def __init__(self):
        self.records = []  # (name, start_event, end_event, flops, bytes[, planes])

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for rec in self.records:
            name, e0, e1, flops, nbytes = rec[:5]
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0,
                                      "flops_by_planes": {}})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
            if len(rec) > 5:
                fp = d["flops_by_planes"]
                fp[rec[5]] = fp.get(rec[5], 0.0) + flops
        return out


_TIMER = None


@contextlib.contextmanager
def kernel_timer():
    """Within this context every pn2 op launch is bracketed by HIP events."""
    global _TIMER
    prev, _TIMER = _TIMER, KernelTimer()
    try:
        yield _TIMER
    finally:
        _TIMER = prev


def _run(name, fn, args, device, flops=0.0, nbytes=0.0):
    t = _TIMER
    if t is None:
        check(fn(*args), name)
        return
    s = torch.cuda.current_stream(device)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(s)
    rc = fn(*args)
    e1.record(s)
    check(rc, name)
    t.records.append((name, e0, e1, float(flops), float(nbytes)))


def _dev(t: Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError("%s: pn2 runs on ROCm device tensors only (got %s); there is no CPU "
                           "path" % (what, t.device))
    if t.dtype != torch.float32 and t.dtype != torch.int64:
        raise TypeError("%s: unsupported dtype %s" % (what, t.dtype))


def _stream(t: Tensor) -> int:
    # this thread's device error slot first (a dict lookup once bound): kernels raise into it
    return _lib.stream_ptr(t.device)


_WS = {}


def _workspace(nbytes: int, device, stream: int) -> Tensor:
    """Scratch of the kernels that merge partial sums (the BN sweeps' float64 column partials,
    pn2_gemm_tn_f32's slab partials): one grow-only buffer per (device, stream).  Every use is
    ordered on that stream and consumed inside the call that fills it, so all of them share it
    (one allocation per step instead of one per call)."""
    key = (device, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def packed_stride(C: int) -> int:
    return int(_L.pn2_packed_stride(C))


def cin_pad(cin: int) -> int:
    return int(_L.pn2_layer_cin_pad(cin))


# ------------------------------------------------------------------------------ fps
def fps_direct(points: Tensor, npoint: int, start: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """points [B,N,C] float32 (any strides), start [B] int64 -> (fps_idx [B,S] int64,
    new_points [B,S,C], packed centroids [B,S,cp], packed points [B,N,cp]).  A CPU start (the
    reference's host draw) goes to pn2_fps_host_ws_f32 in the launch's arguments; a device start
    (and any start under graph capture, whose replays must read a device slot) to pn2_fps_ws_f32."""
    _dev(points, "pn2::fps")
    B, N, C = points.shape
    cp = packed_stride(C)
    host = start.device.type == "cpu" and not torch.cuda.is_current_stream_capturing()
    if host:
        start = start.to(dtype=torch.int64).contiguous()
    else:
        start = start.to(device=points.device, dtype=torch.int64).contiguous()
    idx = torch.empty(B, npoint, dtype=torch.int64, device=points.device)
    newp = torch.empty(B, npoint, C, dtype=torch.float32, device=points.device)
    cpk = torch.empty(B, npoint, cp, dtype=torch.float32, device=points.device)
    ppk = torch.empty(B, N, cp, dtype=torch.float32, device=points.device)
    sb, sn, sc = points.stride()
    # past the register-resident shapes (N > 16384, npoint > 8192) the streamed kernel; past
    # N = 40896 it keeps the running distances in this workspace
    nws = int(_L.pn2_fps_workspace_bytes(B, N, C, npoint))
    ws = torch.empty(max(nws, 0) // 4, dtype=torch.float32, device=points.device) if nws > 0 else None
    _run("pn2_fps_f32", _L.pn2_fps_host_ws_f32 if host else _L.pn2_fps_ws_f32,
         (points.data_ptr(), B, N, C, sb, sn, sc, start.data_ptr(), npoint, idx.data_ptr(),
          newp.data_ptr(), cpk.data_ptr(), ppk.data_ptr(), 0 if ws is None else ws.data_ptr(),
          max(nws, 0), _stream(points)), points.device,
         flops=float(B) * npoint * N * (3 * C + 2))
    return idx, newp, cpk, ppk


fps = torch.library.custom_op("pn2::fps", fps_direct, mutates_args=())


@fps.register_fake
def _(points, npoint, start):
    B, N, C = points.shape
    cp = packed_stride(C)
    e = points.new_empty
    return (e(B, npoint, dtype=torch.int64), e(B, npoint, C), e(B, npoint, cp), e(B, N, cp))


def fps2_eligible(N: int, C: int, S1: int, S2: int) -> bool:
    """Whether two consecutive sampling levels (N -> S1 -> S2 points of C channels) run as one
    pn2_fps2_f32 launch under the current tuning (include/pn2.h)."""
    return bool(_L.pn2_fps2_eligible(N, C, S1, S2))


last_fps2_path = None  # what the last fps2_direct call ran: "two_level" or "separate"


def fps2_direct(points: Tensor, npoint1: int, npoint2: int, start1: Tensor, start2: Tensor):
    """Two consecutive sampling levels: fps_direct(points, npoint1, start1) and fps_direct(its
    new_points, npoint2, start2) -> both result tuples, bit for bit.  Eligible shapes
    (fps2_eligible) run as one launch, one workgroup per cloud doing both levels; any other
    shape runs the two launches.  `last_fps2_path` names the path taken."""
    global last_fps2_path
    _dev(points, "pn2::fps2")
    B, N, C = points.shape
    if not fps2_eligible(N, C, npoint1, npoint2):
        last_fps2_path = "separate"
        r1 = fps_direct(points, npoint1, start1)
        return r1, fps_direct(r1[1], npoint2, start2)
    dev = points.device
    start1 = start1.to(device=dev, dtype=torch.int64).contiguous()
    start2 = start2.to(device=dev, dtype=torch.int64).contiguous()
    cp = packed_stride(C)
    e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    idx1 = torch.empty(B, npoint1, dtype=torch.int64, device=dev)
    idx2 = torch.empty(B, npoint2, dtype=torch.int64, device=dev)
    newp1, cpk1, ppk1 = e(B, npoint1, C), e(B, npoint1, cp), e(B, N, cp)
    newp2, cpk2, ppk2 = e(B, npoint2, C), e(B, npoint2, cp), e(B, npoint1, cp)
    sb, sn, sc = points.stride()
    _run("pn2_fps2_f32", _L.pn2_fps2_f32,
         (points.data_ptr(), B, N, C, sb, sn, sc, start1.data_ptr(), npoint1, start2.data_ptr(), npoint2,
          idx1.data_ptr(), newp1.data_ptr(), cpk1.data_ptr(), ppk1.data_ptr(),
          idx2.data_ptr(), newp2.data_ptr(), cpk2.data_ptr(), ppk2.data_ptr(), _stream(points)), dev,
         flops=float(B) * (npoint1 * N + npoint2 * npoint1) * (3 * C + 2))
    last_fps2_path = "two_level"
    return (idx1, newp1, cpk1, ppk1), (idx2, newp2, cpk2, ppk2)


# ------------------------------------------------------------------------------ pack_points
def pack_points_direct(points: Tensor) -> Tensor:
    """[B,N,C] (any strides) -> [B,N,cp] records (coords, ssq in the reference's order, pad)."""
    _dev(points, "pn2::pack_points")
    B, N, C = points.shape
    out = torch.empty(B, N, packed_stride(C), dtype=torch.float32, device=points.device)
    sb, sn, sc = points.stride()
    _run("pn2_pack_points_f32", _L.pn2_pack_points_f32,
         (points.data_ptr(), B, N, C, sb, sn, sc, out.data_ptr(), _stream(points)), points.device)
    return out


pack_points = torch.library.custom_op("pn2::pack_points", pack_points_direct, mutates_args=())


@pack_points.register_fake
def _(points):
    B, N, C = points.shape
    return points.new_empty(B, N, packed_stride(C))


# ------------------------------------------------------------------------------ ball query
def ball_query_direct(pts_packed: Tensor, ctr_packed: Tensor, C: int, radius: float, nsample: int,
                      with_count: bool = False):
    """Packed points [B,N,cp] and centroids [B,S,cp] -> group_idx [B,S,nsample] int64 (the
    reference's query_ball_point); with with_count the SA layers' fused-path form: the lists as
    int32 (half the bytes; sa_mlp_max_direct reads either) and the distinct neighbours per
    centroid, [B,S] int32 (entries past them repeat entry 0; sa_mlp_max_direct(cnt=...) then
    computes only those rows)."""
    _dev(pts_packed, "pn2::ball_query")
    B, N, _ = pts_packed.shape
    S = ctr_packed.shape[1]
    if nsample > N:
        # the reference's `group_idx[mask] = group_first[mask]` fails the same way (:89)
        raise IndexError("query_ball_point: sample_number %d > number of points %d" % (nsample, N))
    out = torch.empty(B, S, nsample, dtype=torch.int32 if with_count else torch.int64,
                      device=pts_packed.device)
    cnt = torch.empty(B, S, dtype=torch.int32, device=pts_packed.device) if with_count else None
    cp = pts_packed.shape[2]
    fn = _L.pn2_ball_query_i32 if with_count else _L.pn2_ball_query_cnt_f32
    _run("pn2_ball_query_f32", fn,
         (pts_packed.data_ptr(), ctr_packed.data_ptr(), B, N, S, C, float(radius), nsample,
          out.data_ptr(), 0 if cnt is None else cnt.data_ptr(), _stream(pts_packed)),
         pts_packed.device, nbytes=4.0 * cp * B * (N + S) + out.element_size() * B * S * nsample +
         (4.0 * B * S if with_count else 0.0),
         flops=float(B) * S * N * (2 * C + 3))  # pairs x (2C + 3)
    return (out, cnt) if with_count else out


def ball_query_multi_direct(pts_packed: Tensor, ctr_packed: Tensor, C: int, radii, nsamples):
    """ball_query_direct(..., with_count=True) for several radii of one centroid set (an MSG
    layer's scales) in one launch (pn2_ball_query_multi_i32, up to 3 radii per launch): a list of
    (group_idx [B,S,nsample] int32, counts [B,S] int32), the same as one call per radius."""
    _dev(pts_packed, "pn2::ball_query")
    B, N, cp = pts_packed.shape
    S = ctr_packed.shape[1]
    res = []
    for i0 in range(0, len(radii), 3):
        rs, ks = list(radii[i0:i0 + 3]), list(nsamples[i0:i0 + 3])
        for k in ks:
            if k > N:
                raise IndexError("query_ball_point: sample_number %d > number of points %d" % (k, N))
        outs = [torch.empty(B, S, k, dtype=torch.int32, device=pts_packed.device) for k in ks]
        cnts = [torch.empty(B, S, dtype=torch.int32, device=pts_packed.device) for _ in ks]
        nr = len(ks)
        radii_c = (ctypes.c_double * nr)(*[float(r) for r in rs])
        ks_c = (ctypes.c_int64 * nr)(*[int(k) for k in ks])
        outs_c = (ctypes.c_void_p * nr)(*[t.data_ptr() for t in outs])
        cnts_c = (ctypes.c_void_p * nr)(*[t.data_ptr() for t in cnts])
        _run("pn2_ball_query_f32", _L.pn2_ball_query_multi_i32,
             (pts_packed.data_ptr(), ctr_packed.data_ptr(), B, N, S, C, nr, radii_c, ks_c, outs_c, cnts_c,
              _stream(pts_packed)), pts_packed.device,
             nbytes=4.0 * cp * B * (N + S) + sum(4.0 * B * S * (k + 1) for k in ks),
             flops=float(B) * S * N * (2 * C + 3))  # one distance per pair for all radii
        res.extend(zip(outs, cnts))
    return res


def _ball_query_op(pts_packed: Tensor, ctr_packed: Tensor, C: int, radius: float, nsample: int) -> Tensor:
    return ball_query_direct(pts_packed, ctr_packed, C, radius, nsample)


ball_query = torch.library.custom_op("pn2::ball_query", _ball_query_op, mutates_args=())


@ball_query.register_fake
def _(pts_packed, ctr_packed, C, radius, nsample):
    return pts_packed.new_empty(pts_packed.shape[0], ctr_packed.shape[1], nsample, dtype=torch.int64)


# ------------------------------------------------------------------------------ square_distance
def square_distance_direct(src_packed: Tensor, dst_packed: Tensor, C: int) -> Tensor:
    _dev(src_packed, "pn2::square_distance")
    B, S, _ = src_packed.shape
    N = dst_packed.shape[1]
    out = torch.empty(B, S, N, dtype=torch.float32, device=src_packed.device)
    _run("pn2_square_distance_f32", _L.pn2_square_distance_f32,
         (src_packed.data_ptr(), dst_packed.data_ptr(), B, S, N, C, out.data_ptr(),
          _stream(src_packed)), src_packed.device)
    return out


square_distance = torch.library.custom_op("pn2::square_distance", square_distance_direct, mutates_args=())


@square_distance.register_fake
def _(src_packed, dst_packed, C):
    return src_packed.new_empty(src_packed.shape[0], src_packed.shape[1], dst_packed.shape[1])


# ------------------------------------------------------------------------------ index_points
def index_points_direct(points: Tensor, idx: Tensor) -> Tensor:
    """points [B,N,C] (any strides), idx [B,M] int64 -> [B,M,C] contiguous."""
    _dev(points, "pn2::index_points")
    B, N, C = points.shape
    M = idx.shape[1]
    idx = idx.contiguous()
    out = torch.empty(B, M, C, dtype=torch.float32, device=points.device)
    sb, sn, sc = points.stride()
    _run("pn2_index_points_f32", _L.pn2_index_points_f32,
         (points.data_ptr(), B, N, C, sb, sn, sc, idx.data_ptr(), M, out.data_ptr(),
          _stream(points)), points.device)
    return out


index_points = torch.library.custom_op("pn2::index_points", index_points_direct, mutates_args=())


@index_points.register_fake
def _(points, idx):
    return points.new_empty(points.shape[0], idx.shape[1], points.shape[2])


# ------------------------------------------------------------------------------ group
def group_direct(points: Tensor, feature: Optional[Tensor], centers: Tensor, idx: Tensor,
          feature_first: bool) -> Tensor:
    """[B,S,K,C+D]: [xyz(idx) - centre, feature(idx)] (or feature first, the MSG order)."""
    _dev(points, "pn2::group")
    B, N, C = points.shape
    S, K = idx.shape[1], idx.shape[2]
    D = 0 if feature is None else feature.shape[2]
    centers = centers.contiguous()
    idx = idx.contiguous()
    out = torch.empty(B, S, K, C + D, dtype=torch.float32, device=points.device)
    sb, sn, sc = points.stride()
    if feature is None:
        fp, fb, fn, fd = 0, 0, 0, 0
    else:
        fp = feature.data_ptr()
        fb, fn, fd = feature.stride()
    _run("pn2_group_f32", _L.pn2_group_f32,
         (points.data_ptr(), B, N, C, sb, sn, sc, fp, D, fb, fn, fd, centers.data_ptr(), S,
          idx.data_ptr(), K, int(feature_first), out.data_ptr(), _stream(points)), points.device)
    return out


group = torch.library.custom_op("pn2::group", group_direct, mutates_args=())


@group.register_fake
def _(points, feature, centers, idx, feature_first):
    D = 0 if feature is None else feature.shape[2]
    return points.new_empty(points.shape[0], idx.shape[1], idx.shape[2], points.shape[2] + D)


# ------------------------------------------------------------------------------ group_backward
def group_backward_direct(dgrouped: Tensor, idx: Tensor, N: int, D: int, feature_first: bool) -> Tensor:
    """The feature gradient of pn2::group: dgrouped [B,S,K,C+D] float32 (the gradient of the
    grouped rows, read in place: any row stride, features at column 0 when feature_first, else
    at C), idx [B,S,K] int64 or int32 (any strides) -> [B,N,D], each point the float32 sum of
    the rows that name it, in ascending (s,k) order from +0.0 (np.add.at's bits, the same on
    every run; pn2_group_backward_f32)."""
    _dev(dgrouped, "pn2::group_backward")
    if dgrouped.dtype != torch.float32 or idx.dtype not in (torch.int64, torch.int32):
        raise TypeError("pn2::group_backward: float32 rows and int64 / int32 indices")
    B, S, K, W = dgrouped.shape
    if tuple(idx.shape) != (B, S, K) or not 1 <= D <= W:
        raise ValueError("pn2::group_backward: dgrouped [B,S,K,C+D], idx [B,S,K], 1 <= D <= C+D")
    if B * S * K == 0:  # no rows: every sum is empty
        return torch.zeros(B, N, D, dtype=torch.float32, device=dgrouped.device)
    rs = dgrouped.stride(2)
    if (dgrouped.stride(3) != 1 or rs < W or dgrouped.stride(1) != K * rs or
                      dgrouped.stride(0) != S * K * rs):
        dgrouped = dgrouped.contiguous()  # rows that no single row stride describes
        rs = W
    out = torch.empty(B, N, D, dtype=torch.float32, device=dgrouped.device)
    nbytes = int(_L.pn2_group_backward_workspace_bytes(B, N, S, K))
    if nbytes < 0:
        raise ValueError("pn2::group_backward: bad shape B=%d N=%d S=%d K=%d" % (B, N, S, K))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dgrouped.device)
    ib, is_, ik = idx.stride()
    _run("pn2_group_backward_f32", _L.pn2_group_backward_f32,
         (dgrouped.data_ptr(), rs, 0 if feature_first else W - D, idx.data_ptr(),
          _lib.INDEX_I32 if idx.dtype == torch.int32 else _lib.INDEX_I64, ib, is_, ik, B, N, S, K, D,
          out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dgrouped)), dgrouped.device,
         nbytes=4.0 * B * S * K * D + 4.0 * B * N * D)
    return out


group_backward = torch.library.custom_op("pn2::group_backward", group_backward_direct, mutates_args=())


@group_backward.register_fake
def _(dgrouped, idx, N, D, feature_first):
    return dgrouped.new_empty(dgrouped.shape[0], N, D)


# ------------------------------------------------------------------------------ training GEMMs
def _matrix(t: Tensor, what: str) -> Tuple[Tensor, int]:
    """A 2-D float32 device matrix as the GEMM kernels read it in place -> (tensor, leading
    dimension): unit column stride and a row stride >= the width (a slice of wider rows is
    fine); any other view is copied."""
    _dev(t, what)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError("%s: 2-D float32 matrices" % what)
    rows, width = t.shape
    if rows <= 1 and (width <= 1 or t.stride(1) == 1):
        return t, max(width, 1)  # a single row: its stride is never used
    if t.stride(1) != 1 or t.stride(0) < width:
        t = t.contiguous()
    return t, max(t.stride(0), 1)


def gemm_nt_direct(A: Tensor, B: Tensor, bias: Optional[Tensor]) -> Tensor:
    """A [M,K], B [N,K], bias [N] or None -> A B^T + bias [M,N] (pn2_gemm_nt_f32: each row of
    the result a function of that row of A, of B and of the bias only; ascending 16-wide steps
    over K from +0, the bias added last).  Operands are read in place through their row stride."""
    A, lda = _matrix(A, "pn2::gemm_nt")
    B, ldb = _matrix(B, "pn2::gemm_nt")
    M, K = A.shape
    N = B.shape[0]
    if B.shape[1] != K or B.device != A.device:
        raise ValueError("pn2::gemm_nt: A [M,K], B [N,K] on one device")
    bp = 0
    if bias is not None:
        if bias.dtype != torch.float32 or tuple(bias.shape) != (N,) or bias.device != A.device:
            raise ValueError("pn2::gemm_nt: bias [N] float32 on A's device")
        bias = bias.contiguous()
        bp = bias.data_ptr()
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    _run("pn2_gemm_nt_f32", _L.pn2_gemm_nt_f32,
         (A.data_ptr(), lda, B.data_ptr(), ldb, bp, C.data_ptr(), N, M, N, K, _stream(A)), A.device,
         flops=2.0 * M * N * K, nbytes=4.0 * (M * K + N * K + M * N))
    return C


gemm_nt = torch.library.custom_op("pn2::gemm_nt", gemm_nt_direct, mutates_args=())


@gemm_nt.register_fake
def _(A, B, bias):
    return A.new_empty(A.shape[0], B.shape[0])


def gemm_nn_direct(A: Tensor, B: Tensor) -> Tensor:
    """A [M,K], B [K,N] -> A B [M,N] (pn2_gemm_nn_f32: B read as stored, row independence and
    order as gemm_nt)."""
    A, lda = _matrix(A, "pn2::gemm_nn")
    B, ldb = _matrix(B, "pn2::gemm_nn")
    M, K = A.shape
    N = B.shape[1]
    if B.shape[0] != K or B.device != A.device:
        raise ValueError("pn2::gemm_nn: A [M,K], B [K,N] on one device")
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    _run("pn2_gemm_nn_f32", _L.pn2_gemm_nn_f32,
         (A.data_ptr(), lda, B.data_ptr(), ldb, C.data_ptr(), N, M, N, K, _stream(A)), A.device,
         flops=2.0 * M * N * K, nbytes=4.0 * (M * K + N * K + M * N))
    return C


gemm_nn = torch.library.custom_op("pn2::gemm_nn", gemm_nn_direct, mutates_args=())


@gemm_nn.register_fake
def _(A, B):
    return A.new_empty(A.shape[0], B.shape[1])


def gemm_tn_direct(A: Tensor, B: Tensor) -> Tensor:
    """A [M,N], B [M,K] -> A^T B [N,K], the sum over the M rows (pn2_gemm_tn_f32: float32
    partials of pn2_gemm_tn_slab_rows()-row slabs, added in slab order in float64 and rounded
    once; the same bits on every run).  M == 0 gives zeros."""
    A, lda = _matrix(A, "pn2::gemm_tn")
    B, ldb = _matrix(B, "pn2::gemm_tn")
    M, N = A.shape
    K = B.shape[1]
    if B.shape[0] != M or B.device != A.device:
        raise ValueError("pn2::gemm_tn: A [M,N], B [M,K] on one device")
    if M == 0:
        return torch.zeros(N, K, dtype=torch.float32, device=A.device)
    nbytes = int(_L.pn2_gemm_tn_workspace_bytes(M, N, K))
    if nbytes < 0:
        raise ValueError("pn2::gemm_tn: bad shape M=%d N=%d K=%d" % (M, N, K))
    st = _stream(A)
    ws = _workspace(nbytes, A.device, st)
    C = torch.empty(N, K, dtype=torch.float32, device=A.device)
    _run("pn2_gemm_tn_f32", _L.pn2_gemm_tn_f32,
         (A.data_ptr(), lda, B.data_ptr(), ldb, C.data_ptr(), K, M, N, K, ws.data_ptr(), ws.numel(), st),
         A.device, flops=2.0 * M * N * K, nbytes=4.0 * (M * N + M * K + N * K) + 2.0 * nbytes)
    return C


gemm_tn = torch.library.custom_op("pn2::gemm_tn", gemm_tn_direct, mutates_args=())


@gemm_tn.register_fake
def _(A, B):
    return A.new_empty(A.shape[1], B.shape[1])


# ------------------------------------------------------------------------------ FC heads, training
def fc_train_max_rows() -> int:
    """The largest batch pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32 accept."""
    return int(_L.pn2_fc_train_max_rows())


def _fc_entry(direction: str, B: int, rows: Optional[bool]):
    """(timer name, C entry, error prefix) of the FC forward / backward for B rows: the 64-row
    entry up to fc_train_max_rows() rows, the any-B entry above; rows forces one of the two."""
    if B > fc_train_max_rows() if rows is None else rows:
        return ("pn2_fc_rows_%s_f32" % direction, getattr(_L, "pn2_fc_bn_%s_rows_f32" % direction),
                "pn2::fc_rows_" + direction)
    return "pn2_fc_bn_%s_f32" % direction, getattr(_L, "pn2_fc_bn_%s_f32" % direction), "pn2::fc_bn_" + direction


def _vector(t: Optional[Tensor], n: int, what: str, like: Tensor) -> int:
    if t is None:
        return 0
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or t.device != like.device or not t.is_contiguous():
        raise ValueError("%s: contiguous float32 [%d] vectors on the input's device" % (what, n))
    return t.data_ptr()


def fc_bn_forward_direct(x: Tensor, weight: Tensor, bias: Tensor, gamma: Optional[Tensor],
                         beta: Optional[Tensor], running_mean: Optional[Tensor],
                         running_var: Optional[Tensor], eps: float, momentum: float, relu: bool,
                         frozen: bool, rows: Optional[bool] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """x [B,K], weight [N,K], bias [N] -> (Y = x W^T + b, A = act(bn(Y)), stats [mean | invstd]
    or None without BN), one launch: pn2_fc_bn_forward_f32 up to fc_train_max_rows() rows,
    pn2_fc_bn_forward_rows_f32 (recorded by ops.kernel_timer as pn2_fc_rows_forward_f32) above --
    the same sums in the same orders (include/pn2.h states the order rules).  gamma None: no
    BatchNorm.  frozen: the running statistics normalise and are only read; else batch
    statistics, and momentum > 0 updates running_mean / running_var in place.  Strided 2-D views
    with unit column stride are read in place.  rows: True / False force the any-B / the 64-row
    entry whatever B is."""
    name, entry, what = _fc_entry("forward", x.shape[0] if x.dim() == 2 else 0, rows)
    x, ldx = _matrix(x, what)
    weight, ldw = _matrix(weight, what)
    B, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K or weight.device != x.device:
        raise ValueError("%s: x [B,K], weight [N,K] on one device" % what)
    if gamma is not None and not frozen and B == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                         % (torch.Size([B, N]),))
    upd = gamma is not None and not frozen and momentum > 0.0
    use_running = frozen or upd
    Y = torch.empty(B, N, dtype=torch.float32, device=x.device)
    A = torch.empty(B, N, dtype=torch.float32, device=x.device)
    stats = torch.empty(2 * N, dtype=torch.float32, device=x.device) if gamma is not None else None
    flags = (0 if relu else _lib.LAYER_NO_RELU) | (_lib.LAYER_FROZEN_STATS if frozen and gamma is not None else 0)
    _run(name, entry,
         (x.data_ptr(), ldx, weight.data_ptr(), ldw, _vector(bias, N, what, x), B, N, K, float(eps),
          float(momentum) if upd else 0.0,
          _vector(running_mean if use_running else None, N, what, x),
          _vector(running_var if use_running else None, N, what, x),
          _vector(gamma, N, what, x), _vector(beta if gamma is not None else None, N, what, x),
          Y.data_ptr(), N, A.data_ptr(), N, 0 if stats is None else stats.data_ptr(), flags, _stream(x)),
         x.device, flops=2.0 * B * N * K, nbytes=4.0 * (B * K + N * K + 2 * B * N))
    return Y, A, stats


def fc_bn_backward_direct(dA: Tensor, Y: Tensor, x: Tensor, stats: Optional[Tensor],
                          gamma: Optional[Tensor], beta: Optional[Tensor], relu: bool, frozen: bool,
                          rows: Optional[bool] = None):
    """The backward of fc_bn_forward_direct up to the layer's own gradients
    (pn2_fc_bn_backward_f32, or pn2_fc_bn_backward_rows_f32 -- recorded as
    pn2_fc_rows_backward_f32 -- above fc_train_max_rows() rows; rows as there) -> (dY [B,N],
    dW [N,K], dbias [N], dgamma, dbeta -- None without BN).  The input gradient is
    gemm_nn_direct(dY, weight)."""
    name, entry, what = _fc_entry("backward", Y.shape[0] if Y.dim() == 2 else 0, rows)
    dA, ldd = _matrix(dA, what)
    Y, ldy = _matrix(Y, what)
    x, ldx = _matrix(x, what)
    B, N = Y.shape
    K = x.shape[1]
    if tuple(dA.shape) != (B, N) or x.shape[0] != B or dA.device != x.device or Y.device != x.device:
        raise ValueError("%s: dA [B,N], Y [B,N], x [B,K] on one device" % what)
    bn = gamma is not None
    if bn and (stats is None or stats.dtype != torch.float32 or stats.numel() != 2 * N or
               not stats.is_contiguous() or stats.device != x.device):
        raise ValueError("%s: stats is the forward's [mean | invstd], 2N float32" % what)
    dY = torch.empty(B, N, dtype=torch.float32, device=x.device)
    dW = torch.empty(N, K, dtype=torch.float32, device=x.device)
    dbias = torch.empty(N, dtype=torch.float32, device=x.device)
    dgamma = torch.empty(N, dtype=torch.float32, device=x.device) if bn else None
    dbeta = torch.empty(N, dtype=torch.float32, device=x.device) if bn else None
    flags = (0 if relu else _lib.LAYER_NO_RELU) | (_lib.LAYER_FROZEN_STATS if frozen and bn else 0)
    _run(name, entry,
         (dA.data_ptr(), ldd, Y.data_ptr(), ldy, x.data_ptr(), ldx, stats.data_ptr() if bn else 0,
          _vector(gamma, N, what, x), _vector(beta if bn else None, N, what, x), B, N, K,
          dY.data_ptr(), N, dW.data_ptr(), K, dbias.data_ptr(), dgamma.data_ptr() if bn else 0,
          dbeta.data_ptr() if bn else 0, flags, _stream(x)),
         x.device, flops=2.0 * B * N * K, nbytes=4.0 * (B * K + N * K + 3 * B * N))
    return dY, dW, dbias, dgamma, dbeta


def fc_rows_forward_direct(x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, relu,
                           frozen):
    """fc_bn_forward_direct on the any-B entry whatever B is (the same bits up to
    fc_train_max_rows() rows)."""
    return fc_bn_forward_direct(x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, relu,
                                frozen, rows=True)


def fc_rows_backward_direct(dA, Y, x, stats, gamma, beta, relu, frozen):
    """fc_bn_backward_direct on the any-B entry whatever B is."""
    return fc_bn_backward_direct(dA, Y, x, stats, gamma, beta, relu, frozen, rows=True)


# ------------------------------------------------------------------------------ losses, metrics
LOSS_KINDS = {"nll": _lib.LOSS_NLL, "mse": _lib.LOSS_MSE, "l1": _lib.LOSS_L1, "bce": _lib.LOSS_BCE}
REDUCTIONS = {"mean": _lib.REDUCE_MEAN, "sum": _lib.REDUCE_SUM}
METER_KINDS = {"cls": _lib.METER_CLS, "sign": _lib.METER_SIGN, "pose": _lib.METER_POSE}
LOG_SOFTMAX_MAX_K = 1024


def log_softmax_rows_direct(x: Tensor) -> Tensor:
    """x [B,K] -> log_softmax(x, -1) (pn2_log_softmax_rows_f32: per row the float64 sum of
    exponentials in ascending column order; rows independent of each other and of B)."""
    x, ldx = _matrix(x, "pn2::log_softmax_rows")
    B, K = x.shape
    y = torch.empty(B, K, dtype=torch.float32, device=x.device)
    _run("pn2_log_softmax_rows_f32", _L.pn2_log_softmax_rows_f32,
         (x.data_ptr(), ldx, y.data_ptr(), K, B, K, _stream(x)), x.device, nbytes=8.0 * B * K)
    return y


def log_softmax_rows_backward_direct(dy: Tensor, y: Tensor) -> Tensor:
    """dy [B,K] and the forward's y -> dx = dy - exp(y) * sum_j dy_j
    (pn2_log_softmax_rows_backward_f32: the row sum one float64 chain in ascending j)."""
    dy, ldd = _matrix(dy, "pn2::log_softmax_rows_backward")
    y, ldy = _matrix(y, "pn2::log_softmax_rows_backward")
    B, K = y.shape
    if tuple(dy.shape) != (B, K) or dy.device != y.device:
        raise ValueError("pn2::log_softmax_rows_backward: dy [B,K], y [B,K] on one device")
    dx = torch.empty(B, K, dtype=torch.float32, device=y.device)
    _run("pn2_log_softmax_rows_backward_f32", _L.pn2_log_softmax_rows_backward_f32,
         (dy.data_ptr(), ldd, y.data_ptr(), ldy, dx.data_ptr(), K, B, K, _stream(y)), y.device,
         nbytes=12.0 * B * K)
    return dx


def _criterion_target(what: str, kind: str, pred: Tensor, target: Tensor) -> Tuple[Tensor, int]:
    B, K = pred.shape
    if target.device != pred.device:
        raise ValueError("%s: pred and target on one device" % what)
    if kind == "nll":
        if target.dtype != torch.int64 or tuple(target.shape) != (B,):
            raise ValueError("%s: nll target int64 [B]" % what)
        return target.contiguous(), 1
    if target.dtype != torch.float32 or tuple(target.shape) != (B, K):
        raise ValueError("%s: target float32 [B,K], pred's shape" % what)
    return _matrix(target, what)


def criterion_forward_direct(kind: str, reduction: str, pred: Tensor, target: Tensor) -> Tensor:
    """pred [B,K] float32, target (int64 [B] for "nll", float32 [B,K] for "mse" / "l1" / "bce")
    -> the 0-dim float32 loss with reduction "mean" or "sum" (pn2_criterion_forward_f32: ONE
    float64 chain over the element terms in row-major order, rounded once)."""
    what = "pn2::criterion_forward"
    pred, ldp = _matrix(pred, what)
    target, ldt = _criterion_target(what, kind, pred, target)
    B, K = pred.shape
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    _run("pn2_criterion_forward_f32", _L.pn2_criterion_forward_f32,
         (LOSS_KINDS[kind], REDUCTIONS[reduction], pred.data_ptr(), ldp, target.data_ptr(), ldt, B, K,
          loss.data_ptr(), _stream(pred)), pred.device, nbytes=8.0 * B * K)
    return loss


def criterion_backward_direct(kind: str, reduction: str, pred: Tensor, target: Tensor, g: Tensor) -> Tensor:
    """The gradient of criterion_forward_direct with respect to pred for the upstream scalar g
    (a device tensor of one float32: no host read) -> [B,K] (pn2_criterion_backward_f32)."""
    what = "pn2::criterion_backward"
    pred, ldp = _matrix(pred, what)
    target, ldt = _criterion_target(what, kind, pred, target)
    if g.dtype != torch.float32 or g.numel() != 1 or g.device != pred.device:
        raise ValueError("%s: g is one float32 on pred's device" % what)
    g = g.contiguous()
    B, K = pred.shape
    dP = torch.empty(B, K, dtype=torch.float32, device=pred.device)
    _run("pn2_criterion_backward_f32", _L.pn2_criterion_backward_f32,
         (LOSS_KINDS[kind], REDUCTIONS[reduction], pred.data_ptr(), ldp, target.data_ptr(), ldt, g.data_ptr(),
          B, K, dP.data_ptr(), K, _stream(pred)), pred.device, nbytes=12.0 * B * K)
    return dP


def meter_update_direct(kind: str, pred: Tensor, target: Tensor, label: Optional[Tensor], num_category: int,
                        acc: Tensor, invalid: Tensor, records: Tensor, slot: int) -> None:
    """One batch into a meter's device state (pn2_meter_update; include/pn2.h has the rules):
    acc float64 [num_category, W], invalid float64 [1], records float64 [slots, RW], all
    contiguous.  "cls": pred, target int64 [B]; "sign": pred, target float32 [B] or [B,1], label
    int64 [B]; "pose": pred, target float32 [B,D], label int64 [B].  No host sync."""
    what = "pn2::meter_update"
    dev = pred.device
    _dev(pred, what)
    D = pred.shape[1] if kind == "pose" else 1
    W, RW = (1 + D, D) if kind == "pose" else (2, 1)
    for t, shape in ((acc, (num_category, W)), (invalid, (1,)), (records, (records.shape[0], RW))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s: state is contiguous float64 %s on pred's device" % (what, shape))
    B = pred.shape[0]
    if kind == "cls":
        if pred.dtype != torch.int64 or target.dtype != torch.int64 or tuple(pred.shape) != (B,) or \
                tuple(target.shape) != (B,) or target.device != dev:
            raise ValueError("%s: cls takes pred, target int64 [B] on one device" % what)
        pred, target, ldp, ldt, lp = pred.contiguous(), target.contiguous(), 1, 1, 0
    else:
        if kind == "sign":
            pred, target = pred.reshape(B, 1), target.reshape(B, 1)
        pred, ldp = _matrix(pred, what)
        target, ldt = _matrix(target, what)
        if tuple(target.shape) != (B, D) or target.device != dev:
            raise ValueError("%s: target has pred's shape and device" % what)
        if label.dtype != torch.int64 or tuple(label.shape) != (B,) or label.device != dev:
            raise ValueError("%s: label int64 [B] on pred's device" % what)
        label = label.contiguous()
        lp = label.data_ptr()
    _run("pn2_meter_update", _L.pn2_meter_update,
         (METER_KINDS[kind], pred.data_ptr(), ldp, target.data_ptr(), ldt, lp, B, D, num_category,
          acc.data_ptr(), invalid.data_ptr(), records.data_ptr(), slot, records.shape[0], _stream(pred)), dev)


# ------------------------------------------------------------------------------ pack_layer
def pack_layer_direct(weight: Tensor, bias: Optional[Tensor], gamma: Optional[Tensor],
               beta: Optional[Tensor], mean: Optional[Tensor], var: Optional[Tensor],
               eps: float, rot: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Conv2d 1x1 weight [cout,cin,1,1] (+ bias) and eval BatchNorm2d stats -> (W^T pair-packed
    [cin_pad/2,cout,2], alpha [cout], beta [cout]) with layer(x) = relu(alpha*(W x) + beta).
    rot: leading xyz input channels moved behind the features (the kernels' row order)."""
    _dev(weight, "pn2::pack_layer")
    cout, cin = weight.shape[0], weight.shape[1]
    w = weight.reshape(cout, cin).contiguous()
    dev = weight.device
    wt = torch.empty(cin_pad(cin) // 2, cout, 2, dtype=torch.float32, device=dev)
    al = torch.empty(cout, dtype=torch.float32, device=dev)
    be = torch.empty(cout, dtype=torch.float32, device=dev)

    def p(t):
        return 0 if t is None else t.contiguous().data_ptr()
    keep = [None if t is None else t.contiguous() for t in (bias, gamma, beta, mean, var)]
    _run("pn2_pack_layer_f32", _L.pn2_pack_layer_f32,
         (w.data_ptr(), *[p(t) for t in keep], float(eps), cout, cin, int(rot), wt.data_ptr(),
          al.data_ptr(), be.data_ptr(), _stream(weight)), weight.device)
    return wt, al, be


pack_layer = torch.library.custom_op("pn2::pack_layer", pack_layer_direct, mutates_args=())


@pack_layer.register_fake
def _(weight, bias, gamma, beta, mean, var, eps, rot):
    cout, cin = weight.shape[0], weight.shape[1]
    e = weight.new_empty
    return e(cin_pad(cin) // 2, cout, 2), e(cout), e(cout)


def pack_layer_split_direct(weight: Tensor, xyz: int, xyz_first: bool) -> Tensor:
    """Conv2d 1x1 weight [cout,cin,1,1] -> the split image of pn2_pack_layer_split_bf16 (three
    bf16 planes hi/mid/lo, two fp16 planes of the row-scaled weights and the rows' inverse
    scales, in MFMA fragment order), flat 16-bit storage.  xyz: the xyz channels
    of a first layer (its rows are [xyz | features] in the chain kernel; 0 for hidden layers),
    xyz_first: W's own order is [xyz, features] (SSG) rather than [features, xyz] (MSG)."""
    _dev(weight, "pn2::pack_layer_split")
    cout, cin = weight.shape[0], weight.shape[1]
    w = weight.reshape(cout, cin).contiguous()
    nbytes = int(_L.pn2_layer_split_bytes(cout, cin, xyz))
    if nbytes < 0:
        raise ValueError("pn2::pack_layer_split: bad shape cout=%d cin=%d xyz=%d" % (cout, cin, xyz))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    _run("pn2_pack_layer_split_bf16", _L.pn2_pack_layer_split_bf16,
         (w.data_ptr(), cout, cin, int(xyz), 1 if xyz_first else 0, out.data_ptr(),
          _stream(weight)), weight.device)
    return out


pack_layer_split = torch.library.custom_op("pn2::pack_layer_split", pack_layer_split_direct, mutates_args=())


@pack_layer_split.register_fake
def _(weight, xyz, xyz_first):
    cout, cin = weight.shape[0], weight.shape[1]
    return weight.new_empty(int(_L.pn2_layer_split_bytes(cout, cin, xyz)) // 2, dtype=torch.bfloat16)


# ------------------------------------------------------------------------------ sa_mlp_max_
def _src(mode, points, feature, centers, idx, rows, B, N, C, D, S, K, cnt=None):
    s = SaSrc()
    if cnt is not None:
        if cnt.dtype != torch.int32 or not cnt.is_contiguous() or cnt.numel() != B * S:
            raise ValueError("pn2::sa_mlp_max_: cnt must be a contiguous int32 [B, S] tensor")
        s.cnt = cnt.data_ptr()
    s.mode = mode
    if points is not None:
        s.pts = points.data_ptr()
        s.pb, s.pn, s.pc = points.stride()
    if feature is not None:
        if feature.stride(2) != 1:
            raise ValueError("pn2::sa_mlp_max_: features must be channels-last (stride 1)")
        s.feat = feature.data_ptr()
        s.fb, s.fn = feature.stride(0), feature.stride(1)
    if centers is not None:
        s.ctr = centers.data_ptr()
    if idx is not None:
        if idx.dtype == torch.int32:
            s.idx32 = idx.data_ptr()
        else:
            s.idx = idx.data_ptr()
    if rows is not None:
        s.rows = rows.data_ptr()
        s.rs = rows.stride(0)
    s.B, s.N, s.C, s.D, s.S, s.K = B, N, C, D, S, K
    return s


MLP_MAX_LAYERS = 4  # csrc/sa_entry.cpp kMaxLayers


def sa_mlp_supported(couts) -> bool:
    """Whether pn2_sa_mlp_max_f32 takes a chain of these layer widths (csrc/sa_entry.cpp
    validate): at most 4 layers, every width a multiple of 32."""
    couts = list(couts)
    return 1 <= len(couts) <= MLP_MAX_LAYERS and all(c >= 32 and c % 32 == 0 for c in couts)


def fps_side_job(points: Tensor, npoint: int, start: Tensor):
    """The next SA layer's farthest point sampling as a side job of an SA MLP call (pn2_fps_side):
    points [B,N,C] (any strides), start [B] int64 on the CPU -> (job, (fps_idx, new_points,
    packed centroids, packed points)); pass `job` as sa_mlp_max_impl(..., fps_side=job).  The
    outputs are fps_direct's, filled by the MLP call's launches."""
    _dev(points, "pn2::fps")
    B, N, C = points.shape
    cp = packed_stride(C)
    start = start.to(dtype=torch.int64).contiguous()
    if start.device.type != "cpu" or start.shape != (B,):
        raise ValueError("pn2::fps side job: start must be a [B] CPU tensor")
    dev = points.device
    outs = (torch.empty(B, npoint, dtype=torch.int64, device=dev),
            torch.empty(B, npoint, C, dtype=torch.float32, device=dev),
            torch.empty(B, npoint, cp, dtype=torch.float32, device=dev),
            torch.empty(B, N, cp, dtype=torch.float32, device=dev))
    sb, sn, sc = points.stride()
    job = _lib.FpsSide(points.data_ptr(), B, N, C, sb, sn, sc, start.data_ptr(), npoint,
                       *(t.data_ptr() for t in outs))
    job._keep = (points, start)  # alive until the MLP call has read them
    return job, outs


def sa_mlp_max_direct(out: Tensor, mode: int, points: Optional[Tensor], feature: Optional[Tensor],
                centers: Optional[Tensor], idx: Optional[Tensor], wts: List[Tensor],
                alphas: List[Tensor], betas: List[Tensor], cins: List[int],
                splits: List[Tensor], precision: str = "fp32", flags: Optional[List[int]] = None,
                rows: Optional[Tensor] = None, pool: bool = True,
                cnt: Optional[Tensor] = None, zero: Optional[Tensor] = None) -> None:
    """sa_mlp_max_impl without a side job (the signature torch.library registers)."""
    sa_mlp_max_impl(out, mode, points, feature, centers, idx, wts, alphas, betas, cins, splits,
                    precision, flags, rows, pool, cnt, zero)


def sa_mlp_max_impl(out, mode, points, feature, centers, idx, wts, alphas, betas, cins, splits,
                    precision="fp32", flags=None, rows=None, pool=True, cnt=None, zero=None,
                    fps_side=None):
    """Fused gather -> MLP (conv1x1+BN+ReLU)* -> max over each group, written channels-last
    into `out` ([G, >=cout] view with unit column stride; G = B*S groups, or B for
    group_all).  mode: 0 SSG grouping, 1 MSG grouping, 2 group_all, 3 rows (`rows` [B, R, cin]
    with unit column stride: B groups of R rows, `points` unused).  splits: the
    pack_layer_split images of the same layers (empty list: fp32 kernels only).
    precision: "fp32" (pn2_sa_mlp_max_f32) or "bf16" (pn2_sa_mlp_max_bf16, needs splits).
    flags: per-layer PN2_LAYER_* bits (LAYER_NO_RELU).  pool=False: `out` gets every row's
    last-layer output ([M, >=cout], group_all / rows sources).  cnt: the ball query's
    distinct-neighbour counts ([B, S] int32, grouping modes) -- only those rows of each group are
    computed (the rest repeat the first neighbour; same result).  zero: a contiguous float32
    tensor one of the call's launches fills with zeros (group_all's new_points).  fps_side: a
    fps_side_job() the call also runs (sa_mlp_max_impl only; the SA modules' lookahead)."""
    if precision not in PRECISIONS:
        raise ValueError("pn2::sa_mlp_max_: precision must be one of %s" % (PRECISIONS,))
    bf16 = precision == "bf16"
    if bf16 and not splits:
        raise ValueError("pn2::sa_mlp_max_: bf16 needs the split weight images (none for points "
                         "with more than 16 channels)")
    if mode == _lib.SRC_ROWS:
        _dev(rows, "pn2::sa_mlp_max_")
        if rows.dim() != 3 or rows.stride(2) != 1 or rows.stride(0) != rows.shape[1] * rows.stride(1):
            raise ValueError("pn2::sa_mlp_max_: rows must be [B, R, cin] with unit column stride "
                             "and uniform row stride")
        B, K = rows.shape[0], rows.shape[1]
        src = _src(mode, None, None, None, None, rows.view(B * K, -1) if B * K else rows[0],
                   B, K, 0, 0, 1, K)
        dev_t = rows
        S = 1
    else:
        _dev(points, "pn2::sa_mlp_max_")
        B, N, C = points.shape
        D = 0 if feature is None else feature.shape[2]
        if mode == _lib.SRC_GROUP_ALL:
            S, K = 1, N
        else:
            S, K = idx.shape[1], idx.shape[2]
            idx = idx.contiguous()
            centers = centers.contiguous()
        src = _src(mode, points, feature, centers, idx, None, B, N, C, D, S, K,
                   cnt if mode in (_lib.SRC_GROUP_XYZ_FIRST, _lib.SRC_GROUP_FEAT_FIRST) else None)
        dev_t = points
    if zero is not None:
        if zero.dtype != torch.float32 or not zero.is_contiguous() or zero.device != dev_t.device:
            raise ValueError("pn2::sa_mlp_max_: zero must be a contiguous float32 device tensor")
        src.zero_out, src.zero_count = zero.data_ptr(), zero.numel()
    if fps_side is not None:
        src.fps_side = ctypes.addressof(fps_side)
    n = len(wts)
    layers = (MlpLayer * n)()
    for i in range(n):
        layers[i].wt = wts[i].data_ptr()
        layers[i].alpha = alphas[i].data_ptr()
        layers[i].beta = betas[i].data_ptr()
        layers[i].cin = cins[i]
        layers[i].cout = wts[i].shape[1]  # [cin_pad/2, cout, 2]
        layers[i].wt_split = splits[i].data_ptr() if splits else 0
        layers[i].flags = int(flags[i]) if flags else 0
    if out.stride(-1) != 1:
        raise ValueError("pn2::sa_mlp_max_: out must have unit column stride")
    ws_fn = _L.pn2_sa_mlp_workspace_bytes_bf16 if bf16 else _L.pn2_sa_mlp_workspace_bytes
    ws_bytes = int(ws_fn(src, layers, n))
    if ws_bytes < 0:
        check(-1, "pn2_sa_mlp_workspace_bytes")
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev_t.device) if ws_bytes else None
    M = B * S * K
    flops = 2.0 * M * sum(cins[i] * wts[i].shape[1] for i in range(n))  # algorithmic, cin unpadded
    # compulsory bytes: every source element, index and weight read once, the output written once
    if mode == _lib.SRC_ROWS:
        nbytes = 4.0 * B * K * cins[0]
    else:
        nbytes = 4.0 * B * N * (C + D)
        if mode != _lib.SRC_GROUP_ALL:
            nbytes += 4.0 * B * S * C + 8.0 * B * S * K + (4.0 * B * S if cnt is not None else 0.0)
    nbytes += sum(4.0 * (cins[i] + 2) * wts[i].shape[1] for i in range(n))
    nbytes += 4.0 * (B * S if pool else M) * wts[-1].shape[1]
    name = "pn2_sa_mlp_max_bf16" if bf16 else "pn2_sa_mlp_max_f32"
    _run(name, getattr(_L, name),
         (src, layers, n, 1 if pool else 0, out.data_ptr(), out.stride(-2),
          0 if ws is None else ws.data_ptr(), ws_bytes, _stream(dev_t)), dev_t.device, flops=flops,
         nbytes=nbytes)
    if _TIMER is not None and _TIMER.records and _TIMER.records[-1][0] == name:
        _TIMER.records[-1] = _TIMER.records[-1] + (int(_L.pn2_sa_mlp_last_planes()),)


sa_mlp_max_ = torch.library.custom_op("pn2::sa_mlp_max_", sa_mlp_max_direct, mutates_args=("out", "zero"))


@sa_mlp_max_.register_fake
def _(out, mode, points, feature, centers, idx, wts, alphas, betas, cins, splits, precision="fp32",
      flags=None, rows=None, pool=True, cnt=None, zero=None):
    return None


def linear_rows(x: Tensor, weight: Tensor, bias: Optional[Tensor], relu: bool) -> Tensor:
    """act(x @ weight^T + bias) on pn2_linear_rows_f32 (rows in blocks of 16; each output
    element computed the same way whatever the row count, so batch shards are bit-identical):
    x [B, K] (unit column stride), weight [N, K] contiguous, bias [N] or None -> [B, N]."""
    _dev(x, "pn2::linear_rows")
    B, K = x.shape
    N = weight.shape[0]
    if B < 1 or x.stride(1) != 1 or not weight.is_contiguous() or \
            weight.shape[1] != K or (bias is not None and not bias.is_contiguous()):
        raise ValueError("pn2::linear_rows: x [B, K] with unit column stride, weight [N, K] "
                         "contiguous")
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    check(_L.pn2_linear_rows_f32(x.data_ptr(), x.stride(0), B, K, weight.data_ptr(),
                                 0 if bias is None else bias.data_ptr(), out.data_ptr(), N, N,
                                 _lib.LINEAR_RELU if relu else 0, _stream(x)),
          "pn2_linear_rows_f32")
    return out


def fc_tail(x: Tensor, layers, logsoftmax: bool):
    """The heads' eval FC tail on pn2_fc_tail_f32 (two launches): x [B, K] (unit column stride),
    layers = ((W1, b1), (W2, b2), (W3, b3)) folded float32 (bn1 / bn2 in W1 / W2), fc1 and fc2
    with ReLU -> (out [B, N3], argmax [B] int64 or None).  logsoftmax: out is
    log_softmax(fc3(...), -1) and argmax its first per-row maximum (the classifiers' tail,
    pointnet2_cls_ssg.py:36-38)."""
    _dev(x, "pn2::fc_tail")
    (w1, b1), (w2, b2), (w3, b3) = layers
    B, K = x.shape
    N1, N2, N3 = w1.shape[0], w2.shape[0], w3.shape[0]
    if x.stride(1) != 1 or w1.shape[1] != K or w2.shape[1] != N1 or w3.shape[1] != N2:
        raise ValueError("pn2::fc_tail: x [B, K] with unit column stride and chained layer shapes")
    nbytes = int(_L.pn2_fc_tail_workspace_bytes(B, N1, N2))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty(B, N3, dtype=torch.float32, device=x.device)
    amax = torch.empty(B, dtype=torch.int64, device=x.device) if logsoftmax else None

    def p(t):
        return 0 if t is None else t.data_ptr()
    _run("pn2_fc_tail_f32", _L.pn2_fc_tail_f32,
         (x.data_ptr(), x.stride(0), B, K, w1.data_ptr(), p(b1), N1, w2.data_ptr(), p(b2), N2,
          w3.data_ptr(), p(b3), N3, _lib.TAIL_LOGSOFTMAX if logsoftmax else 0, out.data_ptr(), N3,
          p(amax), ws.data_ptr(), nbytes, _stream(x)), x.device,
         flops=2.0 * B * (K * N1 + N1 * N2 + N2 * N3))
    return out, amax


# ------------------------------------------------------------------------------ training BN / ReLU / max
# The sweeps of csrc/train.hip around the shared MLP's GEMMs (pn2.train's autograd function is
# their only caller; no torch.library op: nothing needs the dispatcher).  Rows are read in
# place through their row stride; outputs are allocated here, contiguous.
def _bn_vectors(what: str, Y: Tensor, *vs) -> Tuple[int, ...]:
    C = Y.shape[1]
    return tuple(_vector(v, C, what, Y) for v in vs)


def bn_train_forward_direct(Y: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor],
                            running_var: Optional[Tensor], eps: float, momentum: float,
                            relu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """Y [M, C] -> (A = act((Y - mean) * invstd * gamma + beta), stats [mean | invstd] 2C float32,
    sxhat [C] float64) with the batch statistics of Y's columns (pn2_bn_train_forward_f32:
    statistics sweep, then apply).  momentum > 0 with running statistics updates them in place
    (torch's train-mode rule); otherwise they are not touched."""
    what = "pn2::bn_train_forward"
    Y, ld = _matrix(Y, what)
    M, C = Y.shape
    upd = momentum > 0.0 and running_mean is not None
    A = torch.empty(M, C, dtype=torch.float32, device=Y.device)
    stats = torch.empty(2 * C, dtype=torch.float32, device=Y.device)
    sxhat = torch.empty(C, dtype=torch.float64, device=Y.device)
    st = _stream(Y)
    ws = _workspace(int(_L.pn2_bn_train_workspace_bytes(M, C)), Y.device, st)
    _run("pn2_bn_train_forward_f32", _L.pn2_bn_train_forward_f32,
         (Y.data_ptr(), M, C, ld, float(eps), float(momentum) if upd else 0.0,
          *_bn_vectors(what, Y, running_mean if upd else None, running_var if upd else None, gamma, beta),
          A.data_ptr(), C, 0 if relu else _lib.LAYER_NO_RELU, stats.data_ptr(), sxhat.data_ptr(),
          ws.data_ptr(), ws.numel(), st), Y.device, nbytes=12.0 * M * C, flops=8.0 * M * C)
    return A, stats, sxhat


def bn_relu_apply_direct(Y: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor,
                         relu: bool) -> Tensor:
    """Y [M, C] -> A = act((Y - mean) * invstd * gamma + beta) with the caller's statistics
    (pn2_bn_relu_apply_f32): a hidden layer of pn2.train's frozen mode."""
    what = "pn2::bn_relu_apply"
    Y, ld = _matrix(Y, what)
    M, C = Y.shape
    A = torch.empty(M, C, dtype=torch.float32, device=Y.device)
    _run("pn2_bn_relu_apply_f32", _L.pn2_bn_relu_apply_f32,
         (Y.data_ptr(), M, C, ld, *_bn_vectors(what, Y, mean, invstd, gamma, beta), A.data_ptr(), C,
          0 if relu else _lib.LAYER_NO_RELU, _stream(Y)), Y.device, nbytes=8.0 * M * C, flops=5.0 * M * C)
    return A


def group_max_direct(A: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """A [G*K, C] -> (max [G, C], first argmax [G, C] int32) over each K rows, a NaN above every
    number as torch.max (pn2_group_max_f32)."""
    A, lda = _matrix(A, "pn2::group_max")
    M, C = A.shape
    if K < 1 or M % K:
        raise ValueError("pn2::group_max: A [G*K, C]")
    G = M // K
    out = torch.empty(G, C, dtype=torch.float32, device=A.device)
    arg = torch.empty(G, C, dtype=torch.int32, device=A.device)
    _run("pn2_group_max_f32", _L.pn2_group_max_f32,
         (A.data_ptr(), G, K, C, lda, out.data_ptr(), C, arg.data_ptr(), _stream(A)), A.device,
         nbytes=4.0 * M * C + 8.0 * G * C)
    return out, arg


def bn_relu_backward_direct(Y: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor,
                            dA: Optional[Tensor], dOut: Optional[Tensor], arg: Optional[Tensor], K: int,
                            sxhat: Optional[Tensor], relu: bool,
                            frozen: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The backward of BatchNorm + ReLU on Y [M, C] (pn2_bn_relu_backward_f32) -> (dY [M, C],
    dgamma, dbeta, dbias = sum of dY's rows).  The incoming gradient is dA [M, C], or, with dA
    None, scattered from the max over each K rows: dOut [M/K, C] on the rows arg [M/K, C] int32
    names.  sxhat is the forward's (None when frozen: the running statistics are constants)."""
    what = "pn2::bn_relu_backward"
    Y, ld = _matrix(Y, what)
    M, C = Y.shape
    if dA is not None:
        d, ldd = _matrix(dA, what)
        rows, ap = M, 0
    else:
        if dOut is None or arg is None:
            raise ValueError("%s: dA, or dOut and arg of the max" % what)
        d, ldd = _matrix(dOut, what)
        rows = M // K if K >= 1 and M % K == 0 else -1
        if arg.dtype != torch.int32 or tuple(arg.shape) != (rows, C) or not arg.is_contiguous():
            raise ValueError("%s: arg [M/K, C] contiguous int32" % what)
        ap = arg.data_ptr()
    if tuple(d.shape) != (rows, C) or d.device != Y.device or (sxhat is None and not frozen):
        raise ValueError("%s: dA [M, C] or dOut [M/K, C] on Y's device, sxhat unless frozen" % what)
    dY = torch.empty(M, C, dtype=torch.float32, device=Y.device)
    dgamma, dbeta, dbias = (torch.empty(C, dtype=torch.float32, device=Y.device) for _ in range(3))
    st = _stream(Y)
    ws = _workspace(int(_L.pn2_bn_train_workspace_bytes(M, C)), Y.device, st)
    flags = (0 if relu else _lib.LAYER_NO_RELU) | (_lib.LAYER_FROZEN_STATS if frozen else 0)
    dense = dA is not None
    _run("pn2_bn_relu_backward_f32", _L.pn2_bn_relu_backward_f32,
         (Y.data_ptr(), M, C, ld, *_bn_vectors(what, Y, mean, invstd, gamma, beta),
          d.data_ptr() if dense else 0, ldd, 0 if dense else d.data_ptr(), ldd, ap, K,
          0 if sxhat is None else sxhat.data_ptr(), dY.data_ptr(), C, dgamma.data_ptr(), dbeta.data_ptr(),
          dbias.data_ptr(), ws.data_ptr(), ws.numel(), flags, st), Y.device,
         nbytes=20.0 * M * C if dense else 8.0 * M * C + 20.0 * rows * C, flops=16.0 * M * C)
    return dY, dgamma, dbeta, dbias


# ------------------------------------------------------------------------------ bn_relu_group_max
def bn_relu_group_max_direct(Y: Tensor, K: int, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor,
                             relu: bool) -> Tuple[Tensor, Tensor]:
    """Y [G*K, C] rows (unit column stride) -> (max [G, C], first argmax [G, C] int32) of
    act((Y - mean) * invstd * gamma + beta) over each K rows, in one pass over Y
    (pn2_bn_relu_group_max_f32): the bits of pn2_bn_relu_apply_f32 then pn2_group_max_f32 without
    the [G*K, C] activation between them.  The pooled last layer of pn2.train's frozen mode."""
    _dev(Y, "pn2::bn_relu_group_max")
    M, C = Y.shape
    if K < 1 or M % K or Y.stride(1) != 1 or any(
            t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()
            for t in (mean, invstd, gamma, beta)):
        raise ValueError("pn2::bn_relu_group_max: Y [G*K, C] with unit column stride and four "
                         "contiguous float32 [C] vectors")
    G = M // K
    out = torch.empty(G, C, dtype=torch.float32, device=Y.device)
    arg = torch.empty(G, C, dtype=torch.int32, device=Y.device)
    _run("pn2_bn_relu_group_max_f32", _L.pn2_bn_relu_group_max_f32,
         (Y.data_ptr(), G, K, C, Y.stride(0), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
          beta.data_ptr(), out.data_ptr(), C, arg.data_ptr(), 0 if relu else _lib.LAYER_NO_RELU,
          _stream(Y)), Y.device, nbytes=4.0 * M * C + 8.0 * G * C, flops=5.0 * M * C)
    return out, arg


bn_relu_group_max = torch.library.custom_op("pn2::bn_relu_group_max", bn_relu_group_max_direct,
                                            mutates_args=())


@bn_relu_group_max.register_fake
def _(Y, K, mean, invstd, gamma, beta, relu):
    G = Y.shape[0] // K
    return Y.new_empty(G, Y.shape[1]), Y.new_empty(G, Y.shape[1], dtype=torch.int32)


# ------------------------------------------------------------------------------ v1 transforms
TRANSFORM_MAX_K = 64


def transform_slab_rows() -> int:
    """R of pn2_transform_points_backward_f32's dT rule (a constant of the build)."""
    return int(_L.pn2_transform_slab_rows())


def _cloud(t: Tensor, rows: bool, what: str):
    """A tensor of points, rows [B,N,k] or channel-first [B,k,N], as the transform kernels read it
    in place -> (B, N, k, (sb, sn, sc) element strides of the [B][N][k] view)."""
    _dev(t, what)
    if t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError("%s: 3-D float32 tensors of points" % what)
    v = t if rows else t.permute(0, 2, 1)
    return v.shape[0], v.shape[1], v.shape[2], tuple(v.stride())


def _transforms(T: Tensor, B: int, k: int, what: str) -> Tuple[Tensor, int]:
    """T [B,k,k] as the kernels read it -> (tensor, row stride): unit column stride, a row
    stride >= k and clouds k rows apart; any other view is copied."""
    if T.dtype != torch.float32 or tuple(T.shape) != (B, k, k):
        raise ValueError("%s: T [B,k,k] float32, one transform per cloud" % what)
    if not 1 <= k <= TRANSFORM_MAX_K:
        raise ValueError("%s: k=%d outside [1, %d]" % (what, k, TRANSFORM_MAX_K))
    if T.stride(2) != 1 or T.stride(1) < k or T.stride(0) != k * T.stride(1):
        T = T.contiguous()
    return T, T.stride(1)


def _like_cloud(B: int, N: int, k: int, rows: bool, like: Tensor):
    """A fresh dense tensor in the caller's layout and its [B][N][k] element strides."""
    if rows:
        return torch.empty(B, N, k, dtype=torch.float32, device=like.device), (N * k, k, 1)
    return torch.empty(B, k, N, dtype=torch.float32, device=like.device), (k * N, 1, N)


def transform_points_direct(x: Tensor, T: Tensor, rows: bool) -> Tensor:
    """x rows [B,N,k] (rows) or channel-first [B,k,N] (any strides, read in place), T [B,k,k]
    -> y in x's layout, y[b,n,:] = T[b] x[b,n,:]: torch.bmm(T, x) of a channel-first x,
    torch.bmm(x, T^T) of rows (pn2_transform_points_f32: each element one float32 fma chain over
    ascending j; a row's result depends on that row and T[b] only)."""
    what = "pn2::transform_points"
    B, N, k, (sb, sn, sc) = _cloud(x, rows, what)
    T, ldt = _transforms(T, B, k, what)
    y, (yb, yn, yc) = _like_cloud(B, N, k, rows, x)
    if B * N == 0:
        return y
    _run("pn2_transform_points_f32", _L.pn2_transform_points_f32,
         (x.data_ptr(), sb, sn, sc, T.data_ptr(), ldt, y.data_ptr(), yb, yn, yc, B, N, k, _stream(x)), x.device,
         flops=2.0 * B * N * k * k, nbytes=4.0 * (2 * B * N * k + B * k * k))
    return y


transform_points = torch.library.custom_op("pn2::transform_points", transform_points_direct, mutates_args=())


@transform_points.register_fake
def _(x, T, rows):
    return x.new_empty(x.shape)


def transform_points_backward_direct(dy: Tensor, x: Optional[Tensor], T: Optional[Tensor], rows: bool,
                                     need_dx: bool = True, need_dT: bool = True):
    """The backward of transform_points_direct: dy in the forward's layout (any strides), the
    forward's x (read for dT only) and T (read for dx only) -> (dx in that layout or None,
    dT [B,k,k] or None).  pn2_transform_points_backward_f32: dx one float32 fma chain over
    ascending i per element; dT float64 partials of transform_slab_rows()-row slabs in ascending
    n, added in ascending slab order and rounded once.  The partials live in ops' per-stream
    workspace."""
    what = "pn2::transform_points_backward"
    B, N, k, (db, dn, dc) = _cloud(dy, rows, what)
    if not (need_dx or need_dT):
        return None, None
    xb = xn = xc = ldt = 0
    if need_dT:
        if x is None or _cloud(x, rows, what)[:3] != (B, N, k) or x.device != dy.device:
            raise ValueError("%s: x in dy's shape on dy's device" % what)
        xb, xn, xc = _cloud(x, rows, what)[3]
    if need_dx:
        if T is None or T.device != dy.device:
            raise ValueError("%s: T [B,k,k] on dy's device" % what)
        T, ldt = _transforms(T, B, k, what)
    elif not 1 <= k <= TRANSFORM_MAX_K:
        raise ValueError("%s: k=%d outside [1, %d]" % (what, k, TRANSFORM_MAX_K))
    dx, (gb, gn, gc) = _like_cloud(B, N, k, rows, dy) if need_dx else (None, (0, 0, 0))
    dT = torch.empty(B, k, k, dtype=torch.float32, device=dy.device) if need_dT else None
    if B * N == 0:
        return dx, (dT.zero_() if need_dT else None)
    st = _stream(dy)
    nbytes = int(_L.pn2_transform_workspace_bytes(B, N, k)) if need_dT else 0
    if nbytes < 0:
        raise ValueError("%s: bad shape B=%d N=%d k=%d" % (what, B, N, k))
    ws = _workspace(nbytes, dy.device, st) if need_dT else None
    _run("pn2_transform_points_backward_f32", _L.pn2_transform_points_backward_f32,
         (dy.data_ptr(), db, dn, dc, x.data_ptr() if need_dT else 0, xb, xn, xc,
          T.data_ptr() if need_dx else 0, ldt, dx.data_ptr() if need_dx else 0, gb, gn, gc,
          dT.data_ptr() if need_dT else 0, B, N, k, ws.data_ptr() if need_dT else 0,
          ws.numel() if need_dT else 0, st), dy.device,
         flops=2.0 * B * N * k * k * (int(need_dx) + int(need_dT)),
         nbytes=4.0 * B * N * k * (1 + int(need_dx) + int(need_dT)) + 2.0 * nbytes)
    return dx, dT


def _transform_points_backward_op(dy: Tensor, x: Tensor, T: Tensor, rows: bool) -> Tuple[Tensor, Tensor]:
    return transform_points_backward_direct(dy, x, T, rows)


transform_points_backward = torch.library.custom_op("pn2::transform_points_backward",
                                                    _transform_points_backward_op, mutates_args=())


@transform_points_backward.register_fake
def _(dy, x, T, rows):
    return dy.new_empty(dy.shape), T.new_empty(T.shape)


def orthogonality_forward_direct(T: Tensor, want_G: bool = False):
    """T [B,k,k] -> (loss 0-dim, norm [B], G [B,k,k] or None): feature_transform_reguliarzer's
    mean_b ||T[b] T[b]^T - I||_F (pn2_orthogonality_forward_f32: G one float32 fma chain per
    element, bitwise symmetric; each norm one float64 chain in row-major order; the mean one
    float64 chain over ascending b)."""
    what = "pn2::orthogonality_forward"
    _dev(T, what)
    if T.dim() != 3 or T.shape[1] != T.shape[2] or T.shape[0] < 1:
        raise ValueError("%s: T [B,k,k], B >= 1" % what)
    B, k = T.shape[0], T.shape[1]
    T, ldt = _transforms(T, B, k, what)
    loss = torch.empty((), dtype=torch.float32, device=T.device)
    norm = torch.empty(B, dtype=torch.float32, device=T.device)
    G = torch.empty(B, k, k, dtype=torch.float32, device=T.device) if want_G else None
    _run("pn2_orthogonality_forward_f32", _L.pn2_orthogonality_forward_f32,
         (T.data_ptr(), ldt, B, k, G.data_ptr() if want_G else 0, norm.data_ptr(), loss.data_ptr(), _stream(T)),
         T.device, flops=2.0 * B * k * k * k, nbytes=4.0 * B * k * k)
    return loss, norm, G


def _orthogonality_forward_op(T: Tensor) -> Tuple[Tensor, Tensor]:
    return orthogonality_forward_direct(T)[:2]


orthogonality_forward = torch.library.custom_op("pn2::orthogonality_forward", _orthogonality_forward_op,
                                                mutates_args=())


@orthogonality_forward.register_fake
def _(T):
    return T.new_empty(()), T.new_empty(T.shape[0])


def orthogonality_backward_direct(T: Tensor, norm: Tensor, dloss: Tensor) -> Tensor:
    """T [B,k,k], the forward's norm [B], dloss (a one-element float32 device tensor) ->
    dT[b] = c_b * (G[b] T[b]), c_b = 2 dloss / (B norm[b]) evaluated in float64, +0 where
    norm[b] == 0 (pn2_orthogonality_backward_f32)."""
    what = "pn2::orthogonality_backward"
    _dev(T, what)
    if T.dim() != 3 or T.shape[1] != T.shape[2] or T.shape[0] < 1:
        raise ValueError("%s: T [B,k,k], B >= 1" % what)
    B, k = T.shape[0], T.shape[1]
    T, ldt = _transforms(T, B, k, what)
    if (norm.dtype != torch.float32 or tuple(norm.shape) != (B,) or norm.device != T.device or
            dloss.dtype != torch.float32 or dloss.numel() != 1 or dloss.device != T.device):
        raise ValueError("%s: norm [B] and a one-element dloss, float32 on T's device" % what)
    norm = norm.contiguous()
    dT = torch.empty(B, k, k, dtype=torch.float32, device=T.device)
    _run("pn2_orthogonality_backward_f32", _L.pn2_orthogonality_backward_f32,
         (T.data_ptr(), ldt, norm.data_ptr(), dloss.data_ptr(), B, k, dT.data_ptr(), _stream(T)), T.device,
         flops=4.0 * B * k * k * k, nbytes=8.0 * B * k * k)
    return dT


orthogonality_backward = torch.library.custom_op("pn2::orthogonality_backward", orthogonality_backward_direct,
                                                 mutates_args=())


@orthogonality_backward.register_fake
def _(T, norm, dloss):
    return T.new_empty(T.shape)

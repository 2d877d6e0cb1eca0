"""Tuning of the launch choices -- for A/B experiments and tests, not for users.

The product path reads one environment variable, once, at import:

    PN2_TUNING="key=value,key=value,..."

Keys are the library's kernel-selection parameters (include/pn2.h ``pn2_tuning_set``:
``mlp_f32``, ``chain_prepass``, ``dense_pair``, ``compact``, ``compact_pool``, ``compact_stages``,
``bq_waves``, ``bq_rowbuf_kb``, ``fps_threads``, ``fps_ppt``, ``fps_mid``, ``dense_maxntc``,
``dense_minwg``, ``dense_wide_minwg``, ``dense_lds``, ``dense_lds_stages``, ``dense_lds_xcd2d``,
``dense_lds_tile``; csrc/pn2_internal.h documents each) and these host-side ones:

    drain_heads      how many final batches of a pipelined run take their heads on their own
                     compute streams (default 2)
    geometry_stream  1: the eager forward runs layer i+1's FPS + ball query on a side stream
    fc_tail          0: the heads' FC tail as one row-kernel launch per layer + torch's
                     log_softmax / argmax, instead of pn2_fc_tail_f32's fused fc3 + log_softmax
    tail_streams     2: the pipeline's heads alternate between two tail streams (needs the
                     hardware queues: GPU_MAX_HW_QUEUES >= the pipeline's streams)
    force_gather     1: shard.all_gather_rows runs its collective in a 1-rank group too (the
                     bench's --force-rccl measurement of the collective's cost on one GPU)
    geometry_bq      1: the pipeline's geometry stream runs the ball queries after the FPS;
                     0: only the FPS, each batch's forward (compute stream) queries
    pipe_fuse        1: GraphedPipeline runs one forward (sa + head graphs) per geometry group,
                     its batches side by side; 0: one forward per batch
    bq_multi         1: an MSG layer's ball queries in one launch over its radii
                     (pn2_ball_query_multi_i32); 0: one launch per radius
    eval_grad        1: an SA module's eval-mode forward under autograd runs the fused inference
                     kernels and recomputes the layer in its backward (pointnet2_utils
                     _SaEvalGrad); 0: the reference's torch formulation
    group_backward   0: the grouping's feature gradient (train._GroupTrain.backward) by torch's
                     index_add_ -- float atomic adds, the sum's order and last bits differ from
                     run to run; 1: pn2_group_backward_f32, each point's rows summed in position
                     order -- the CPU index_add_'s bits, the same on every run.  With
                     torch.use_deterministic_algorithms(True) the kernel runs whatever the key
                     says.  0 or 1; anything else is an error
    train_gemm       0: the three matrix products of a shared-MLP layer's training step
                     (train._MlpMaxTrain: Y = X W^T + b, dX = dY W, dW = dY^T X) are library
                     GEMMs (torch.addmm / mm / bmm), whose summation order is the library's
                     choice; 1: pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32, every sum
                     in a fixed order (include/pn2.h) -- with group_backward=1 an SA layer's
                     step then has no order-dependent sum.  Not tied to
                     torch.use_deterministic_algorithms.  0 or 1; anything else is an error
    train_head       0: the heads' FC layers under autograd (the FC tails' fc1/bn1, fc2/bn2, fc3,
                     the translation heads' mean MLP, the T-Nets' and the v1 heads' FC tails) are
                     the torch modules: library GEMMs and BatchNorm1d's kernels, whose summation
                     order is the library's choice; 1: pn2_fc_bn_forward_f32 /
                     pn2_fc_bn_backward_f32 (+ pn2_gemm_nn_f32 for the input gradient) wherever
                     the forward must be differentiable, in train mode (batch statistics) and
                     in eval mode (frozen running statistics): one launch per layer and
                     direction, every sum in a fixed order (include/pn2.h) -- with train_gemm=1
                     and group_backward=1 a PointNet++ head's train step then has no
                     order-dependent sum in any kernel of this project (dropout's mask, the
                     loss and the optimizer stay torch).  Batches above
                     pn2_fc_train_max_rows() rows keep the modules unless train_head_rows=1.
                     0 or 1; anything else is an error
    train_head_rows  with train_head=1 only.  0: an FC layer whose batch has more than
                     pn2_fc_train_max_rows() (64) rows stays the torch modules, so above 64 rows
                     the reproducibility route above does not hold; 1: such a batch runs
                     pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32 (+ pn2_gemm_nn_f32),
                     the same kernel pair with its slab loop at run-time length: the same sums
                     in the same fixed orders at any number of rows -- each column's rows are
                     one serial chain inside one workgroup, so these launches have no more
                     workgroups than at 64 rows and their time grows with the batch (DESIGN.md
                     §4.4 has the measurements).  Batches of 64 rows or fewer run the one-slab
                     instantiation either way; with train_head=0 the key does nothing.
                     0 or 1; anything else is an error
    train_loss       0: the classifiers' log_softmax under autograd (heads._fc_log_softmax, the
                     two heads_v1 classifiers) is F.log_softmax, a row reduction forward and
                     backward whose order is torch's choice; 1: pn2.losses.log_softmax
                     (pn2_log_softmax_rows_f32 / _backward_f32: each row's sums one float64
                     chain in ascending column order, include/pn2.h).  With the four keys above
                     at 1 and the criterion from pn2.losses (ClsLoss / PoseLoss / SignLoss: the
                     loss ONE float64 chain over the element terms in row-major order), a
                     PointNet++ head's whole train step then has no reduction whose order this
                     project does not fix; what stays torch is dropout's mask, the optimizer,
                     sigmoid and the elementwise adds.  The criteria and the meters of
                     pn2.metrics are the caller's to use and need no key.  The no-autograd eval
                     path (pn2_fc_tail_f32) is untouched.  Measured (profiles/loss/timing.json,
                     torch / kernels, forward + backward at B=32): log_softmax 0.027 / 0.051 ms,
                     nll_loss 0.036 / 0.058 ms, MSELoss(sum) 0.043 / 0.060 ms -- host-bound, the
                     kernels' route the slower one; the whole ClsSSG B=32 train step 5.746 /
                     5.746 ms.  The key buys the fixed order, not speed.
                     0 or 1; anything else is an error
    v1_transform     0: the per-cloud transforms of the PointNet-v1 modules under autograd
                     (PointNetEncoder's and PoseV1's two torch.bmm each) and
                     feature_transform_reguliarzer are torch: library calls whose summation
                     order -- bmm's backward sums over all N points of a cloud -- is the
                     library's choice; 1: pn2.train.transform_points / orthogonality_loss
                     (csrc/v1_transform.hip: pn2_transform_points_f32 / _backward_f32,
                     pn2_orthogonality_forward_f32 / _backward_f32, every sum in a stated order,
                     include/pn2.h) wherever a v1 module must be differentiable on float32 device
                     tensors, in train mode and in eval under autograd.  CPU or non-float32
                     tensors and k > 64 keep torch; the no_grad fused forward is untouched.
                     With train_gemm=1, train_head=1 and train_loss=1 a pointnet_cls or pose
                     train step then carries the guarantee stated for the PointNet++ heads
                     (DESIGN.md §7).  0 or 1; anything else is an error
    v1_eval_grad     0: a v1 module's eval-mode forward that must be differentiable runs the
                     reference's Conv1d / BatchNorm1d formulation and saves every [B, C, N]
                     activation; 1: pointnet_utils.mlp_mode answers "eval_grad" for float32
                     device tensors, fp32 precision, layers train.eligible_frozen accepts and
                     widths ops.sa_mlp_supported accepts: the shared MLPs run the fused
                     inference kernels (the no_grad launches and bits) inside an autograd
                     Function that saves the input only and recomputes the MLP on the
                     frozen-statistics training kernels in its backward
                     (pointnet_utils._V1EvalGrad, modelled on _SaEvalGrad).  Inside
                     pn2.eval_autograd() the answer stays "torch".  0 or 1; anything else is an
                     error
    pipe_profile     1: the pipelines (pn2.pipeline) whose launches carry >= 64 clouds
                     (fused groups, or B >= 64) capture and run their kernels under
                     PIPELINE_PROFILE -- the launch choices measured best beside each other's
                     kernels, where the kernel defaults are the ones measured best alone (the
                     eager forward, GraphedForward); 0: the defaults everywhere; 2: every
                     pipeline (A/B)

Unknown keys are an error.  ``override(**kw)`` changes keys for the duration of a ``with``
block (tests); process-wide kernel keys are atomic words in the library, so a change on one
thread while another launches is safe.  ``pipeline_profile()`` applies PIPELINE_PROFILE only
to keys still at their library default: an explicit setting wins inside the pipelines too.
Every default is the measured best.
"""
import contextlib
import os

HOST_DEFAULTS = {
    "pipe_profile": 1,
    "drain_heads": 2,
    "geometry_stream": 0,
    "fc_tail": 1,
    "force_gather": 0,
    "tail_streams": 1,
    "geometry_bq": 1,
    "pipe_fuse": 1,
    "bq_multi": 1,
    "eval_grad": 1,
    "group_backward": 0,
    "train_gemm": 0,
    "train_head": 0,
    "train_head_rows": 0,
    "train_loss": 0,
}
# host keys with a checked range (inclusive); the others take any integer
HOST_RANGES = {"group_backward": (0, 1), "train_gemm": (0, 1), "train_head": (0, 1), "train_head_rows": (0, 1),
               "train_loss": (0, 1)}
# The PointNet-v1 autograd routes' keys: host keys like the ones above in every respect (get,
# override, PN2_TUNING), in a table of their own because tests/test_abi_loss.py pins
# HOST_DEFAULTS to exactly the keys it had when train_loss was added.
V1_DEFAULTS = {
    "v1_transform": 0,
    "v1_eval_grad": 0,
}
V1_RANGES = {"v1_transform": (0, 1), "v1_eval_grad": (0, 1)}
_HOST_KEYS = {**HOST_DEFAULTS, **V1_DEFAULTS}


def _check_host(key, value):
    lo, hi = HOST_RANGES.get(key, V1_RANGES.get(key, (value, value)))
    if not lo <= value <= hi:
        raise ValueError("pn2 tuning: %s=%r is outside [%d, %d]" % (key, value, lo, hi))
    return value


def _parse(text):
    out = {}
    for item in filter(None, (t.strip() for t in text.split(","))):
        if "=" not in item:
            raise ValueError("PN2_TUNING: expected key=value, got %r" % item)
        k, v = (s.strip() for s in item.split("=", 1))
        out[k] = int(v)
    return out


_ENV = _parse(os.environ.get("PN2_TUNING", ""))
_host = dict(_HOST_KEYS)
_host.update({k: _check_host(k, v) for k, v in _ENV.items() if k in _HOST_KEYS})


# Kernel keys the pipelines set while they capture / run: the FPS block of 4
# waves x 4 points, the register-staged dense kernel, 8-wave ball-query workgroups (for
# clouds below 2048 points) and group_all's first two layers one launch each (the fused pair
# streams both layers' weights per 32-row block: at a fused group's 16384 rows that L2 -> CU
# stream costs more than the launch it saves, SSG K=100 192.2k with it vs 195.3k) -- each
# faster alone in the other form, slower beside the chains.
PIPELINE_PROFILE = {"fps_mid": 256, "dense_lds": 0, "bq_waves": 0, "dense_pair": 0}


@contextlib.contextmanager
def local():
    """Context: this host thread's own copy of the kernel keys (pn2_tuning_local); changes
    inside it do not reach other threads and end with it."""
    from . import _lib
    L = _lib.load()
    _lib.check(L.pn2_tuning_local(1), "pn2_tuning_local")
    try:
        yield
    finally:
        _lib.check(L.pn2_tuning_local(0), "pn2_tuning_local")


_DEFAULTS = {}


def kernel_default(key):
    """A kernel-selection parameter's library default (pn2_tuning_default)."""
    if key not in _DEFAULTS:
        import ctypes
        from . import _lib
        v = ctypes.c_int64(0)
        _lib.check(_lib.load().pn2_tuning_default(key.encode(), ctypes.byref(v)), "pn2_tuning_default")
        _DEFAULTS[key] = v.value
    return _DEFAULTS[key]


def effective_pipeline_profile():
    """The PIPELINE_PROFILE entries a pipeline applies now: only keys that still hold their
    library default -- a key set by PN2_TUNING or override() keeps that value in the pipelines
    too (an A/B of e.g. dense_lds=1 measures the pipelines as well).  {} with pipe_profile 0."""
    if not _host["pipe_profile"]:
        return {}
    return {k: v for k, v in PIPELINE_PROFILE.items() if kernel(k) == kernel_default(k)}


@contextlib.contextmanager
def pipeline_profile():
    """Context: the effective PIPELINE_PROFILE (above) applied on this thread's own copy of
    the keys -- a forward on another host thread meanwhile keeps the defaults."""
    prof = effective_pipeline_profile()
    if not prof:
        yield
        return
    with local(), override(**prof):
        yield


def get(key):
    """A host-side key's value (kernel keys: ``kernel(key)``)."""
    return _host[key]


def kernel(key):
    """A kernel-selection parameter's current value in the loaded library."""
    import ctypes
    from . import _lib
    v = ctypes.c_int64(0)
    _lib.check(_lib.load().pn2_tuning_get(key.encode(), ctypes.byref(v)), "pn2_tuning_get")
    return v.value


def _set_kernel(L, key, value):
    if L.pn2_tuning_set(key.encode(), int(value)) != 0:
        raise ValueError("pn2 tuning: %s" % L.pn2_last_error().decode(errors="replace"))


def apply_env(L):
    """Apply PN2_TUNING's kernel keys to the just-loaded library L (called by _lib.load)."""
    for k, v in _ENV.items():
        if k not in _HOST_KEYS:
            _set_kernel(L, k, v)


@contextlib.contextmanager
def override(**kw):
    """Change tuning keys (host-side or kernel) within a ``with`` block, then restore them."""
    from . import _lib
    L = _lib.load()
    saved = []
    try:
        for k, v in kw.items():
            if k in _HOST_KEYS:
                _check_host(k, v)
                saved.append((k, _host[k], True))
                _host[k] = v
            else:
                saved.append((k, kernel(k), False))
                _set_kernel(L, k, v)
        yield
    finally:
        for k, v, host in reversed(saved):
            if host:
                _host[k] = v
            else:
                _set_kernel(L, k, v)

"""The training scripts' criteria and the classifiers' log_softmax on csrc/loss.hip: every
reduction in a fixed order (include/pn2.h: a row's log_softmax sums one float64 chain in
ascending column order, a loss ONE float64 chain over its element terms in row-major order).

The modules mirror the reference's ``get_loss`` classes, signature for signature:

  ClsLoss   model/pointnet2_cls_ssg.py:40-47   F.nll_loss(pred, target)
  PoseLoss  model/rotation_ssg.py:40-50        nn.MSELoss / nn.L1Loss(reduction=...)
  SignLoss  model/sign_ssg.py:38-45            nn.BCELoss()

They run the kernels for CUDA float32 2-D predictions with a matching target (int64 [B] for
ClsLoss, float32 of pred's shape otherwise) and reduction 'mean' or 'sum'.  Anything else --
CPU tensors among it -- calls the torch.nn.functional function the reference calls.  The
backward is once-differentiable and gives the prediction's gradient only (as the loops need).

``log_softmax(x)`` is the classifiers' F.log_softmax(x, -1) under autograd; the heads call it
when the tuning key train_loss is 1 (``head_log_softmax``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops, tuning


def _kernel_matrix(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] >= 1


class _LogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.log_softmax_rows_direct(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.log_softmax_rows_backward_direct(dy, y)


def log_softmax(x):
    """F.log_softmax(x, -1) of a CUDA float32 [B, K] matrix, K <= 1024, on the fixed-order
    kernels, differentiable once.  Other inputs take F.log_softmax."""
    if _kernel_matrix(x) and x.shape[1] <= ops.LOG_SOFTMAX_MAX_K:
        return _LogSoftmax.apply(x)
    return F.log_softmax(x, -1)


def head_log_softmax(x):
    """The heads' log_softmax: the kernels when the forward must be differentiable and the
    tuning key train_loss is 1, F.log_softmax otherwise (train_loss=0 changes nothing)."""
    if tuning.get("train_loss") == 1 and x.requires_grad and torch.is_grad_enabled():
        return log_softmax(x)
    return F.log_softmax(x, -1)


class _Criterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, reduction):
        ctx.save_for_backward(pred, target)
        ctx.kind, ctx.reduction = kind, reduction
        return ops.criterion_forward_direct(kind, reduction, pred, target)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return ops.criterion_backward_direct(ctx.kind, ctx.reduction, pred, target, g), None, None, None


def _eligible(pred, target, kind, reduction):
    if reduction not in ops.REDUCTIONS or not torch.is_tensor(pred) or not torch.is_tensor(target):
        return False
    if not _kernel_matrix(pred) or target.device != pred.device or target.requires_grad:
        return False
    if kind == "nll":
        return target.dtype == torch.int64 and tuple(target.shape) == (pred.shape[0],)
    return target.dtype == torch.float32 and target.shape == pred.shape


def criterion(kind, reduction, pred, target):
    """The fixed-order loss of kind "nll" / "mse" / "l1" / "bce" (the modules' kernel route)."""
    return _Criterion.apply(pred, target, kind, reduction)


class ClsLoss(nn.Module):
    """get_loss of pointnet2_cls_ssg.py:40-47 (and the other classifiers'): nll_loss of the
    log-probabilities, mean over the batch; trans_feat is accepted and unused, as there."""

    def forward(self, pred, target, trans_feat=None):
        if _eligible(pred, target, "nll", "mean"):
            return criterion("nll", "mean", pred, target)
        return F.nll_loss(pred, target)


class PoseLoss(nn.Module):
    """get_loss of rotation_ssg.py:40-50 (and translation's): 'L2_loss' is nn.MSELoss, any other
    type nn.L1Loss, with the given reduction."""

    def __init__(self, type='L2_loss', reduction='mean'):
        super().__init__()
        self.kind = "mse" if type == 'L2_loss' else "l1"
        self.reduction = reduction

    def forward(self, pred, target):
        if _eligible(pred, target, self.kind, self.reduction):
            return criterion(self.kind, self.reduction, pred, target)
        if self.kind == "mse":
            return F.mse_loss(pred, target, reduction=self.reduction)
        return F.l1_loss(pred, target, reduction=self.reduction)


class SignLoss(nn.Module):
    """get_loss of sign_ssg.py:38-45: nn.BCELoss() of the sigmoid output, mean reduction."""

    def forward(self, pred, target):
        if _eligible(pred, target, "bce", "mean"):
            return criterion("bce", "mean", pred, target)
        return F.binary_cross_entropy(pred, target)

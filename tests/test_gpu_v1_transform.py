"""csrc/v1_transform.hip on the device, BIT FOR BIT against tests/v1_transform_ref.py (the numpy
restatement of the order rules in include/pn2.h): the transform forward, dx and dT over
k in {1, 3, 5, 64}, N around the 64-row tile and the slab length R, B in {1, 3}, through every
layout the kernels read in place (rows, channel-first, a row stride above k, a misaligned base:
the dword paths), non-contiguous dy, NaN-filled outputs, dx-only / dT-only calls, row and cloud
independence, the regulariser forward and backward (T = I, the zero norm, included), and the
autograd Functions against torch's bmm / regulariser on the same device tensors at the
project's feature bar, 1e-5 |ref| + 1e-5 max|ref|."""
import ctypes

import numpy as np
import pytest
import torch

import v1_transform_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (1, 3, 5, 64)
BS = (1, 3)


def slab_rows():
    from pn2 import ops
    return ops.transform_slab_rows()


def n_values():
    Rr = 128  # pn2_transform_slab_rows(); test_slab_rows_is_the_parametrised_one pins it
    return (1, 63, 64, 65, Rr - 1, Rr, Rr + 1, 2 * Rr + 1)


def test_slab_rows_is_the_parametrised_one():
    assert slab_rows() == 128


def data(B, N, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N, k)).astype(np.float32)
    T = (rng.standard_normal((B, k, k)) / np.sqrt(k)).astype(np.float32)
    dy = rng.standard_normal((B, N, k)).astype(np.float32)
    return x, T, dy


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(what))


def layout(a, kind):
    """The logical [B,N,k] array a as a device tensor in one of the layouts -> (tensor as the op
    takes it, rows flag)."""
    B, N, k = a.shape
    t = torch.from_numpy(a).to(DEV)
    if kind == "rows":
        return t.contiguous(), True
    if kind == "cf":  # channel-first [B,k,N]
        return t.permute(0, 2, 1).contiguous(), False
    if kind == "rows_wide":  # a row stride above k (a slice of wider rows)
        buf = torch.full((B, N, k + 4), float("nan"), device=DEV)
        buf[..., :k] = t
        return buf[..., :k], True
    if kind == "rows_odd":  # ... an odd one: dword accesses
        buf = torch.full((B, N, k + 3), float("nan"), device=DEV)
        buf[..., 1:k + 1] = t
        return buf[..., 1:k + 1], True
    if kind == "rows_misaligned":  # dense rows one element off a 16-byte boundary
        buf = torch.full((B * N * k + 1,), float("nan"), device=DEV)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(B, N, k), True
    if kind == "cf_misaligned":
        buf = torch.full((B * N * k + 1,), float("nan"), device=DEV)
        buf[1:] = t.permute(0, 2, 1).reshape(-1)
        return buf[1:].view(B, k, N), False
    if kind == "rows_of_cf":  # rows [B,N,k] that are a permuted view of channel-first storage
        return t.permute(0, 2, 1).contiguous().permute(0, 2, 1), True
    raise KeyError(kind)


LAYOUTS = ("rows", "cf", "rows_wide", "rows_odd", "rows_misaligned", "cf_misaligned", "rows_of_cf")


def logical(t, rows):
    return t if rows else t.permute(0, 2, 1)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", n_values())
@pytest.mark.parametrize("k", KS)
def test_transform_bits(k, N, B):
    from pn2 import ops
    x, T, dy = data(B, N, k, 1000 * k + 10 * N + B)
    want_y = R.transform_points(x, T)
    want_dx = R.transform_points_dx(dy, T)
    want_dT = R.transform_points_dT(dy, x, slab_rows())
    Tn = torch.from_numpy(T).to(DEV)
    Tw = torch.full((B, k, k + 2), float("nan"), device=DEV)  # T with a row stride above k
    Tw[..., :k] = Tn
    for i, kind in enumerate(LAYOUTS):
        xt, rows = layout(x, kind)
        Tt = Tw[..., :k] if i % 2 else Tn
        y = ops.transform_points_direct(xt, Tt, rows)
        assert y.is_contiguous() and y.shape == xt.shape
        same_bits(logical(y, rows), want_y, ("y", kind))
        # dy in another layout than x (non-contiguous included), same rows flag
        dkind = {True: ("rows_wide", "rows_of_cf", "rows"), False: ("cf_misaligned", "cf")}[rows][i % (3 if rows else 2)]
        dyt, drows = layout(dy, dkind)
        assert drows == rows
        dx, dT = ops.transform_points_backward_direct(dyt, xt, Tt, rows)
        same_bits(logical(dx, rows), want_dx, ("dx", kind, dkind))
        same_bits(dT, want_dT, ("dT", kind, dkind))
        dx1, none = ops.transform_points_backward_direct(dyt, None, Tt, rows, need_dT=False)
        assert none is None
        same_bits(logical(dx1, rows), want_dx, ("dx only", kind))
        none, dT1 = ops.transform_points_backward_direct(dyt, xt, None, rows, need_dx=False)
        assert none is None
        same_bits(dT1, want_dT, ("dT only", kind))
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", KS)
def test_row_and_cloud_independence(k):
    """A row's y equals its y in a batch of one row; a cloud's dT is unchanged by the other
    clouds of the batch."""
    from pn2 import ops
    B, N = 3, 2 * slab_rows() + 1
    x, T, dy = data(B, N, k, 77 + k)
    xt, Tt, dyt = (torch.from_numpy(a).to(DEV) for a in (x, T, dy))
    y = ops.transform_points_direct(xt, Tt, True)
    dx, dT = ops.transform_points_backward_direct(dyt, xt, Tt, True)
    for b, n in ((0, 0), (1, 64), (2, N - 1), (1, slab_rows())):
        y1 = ops.transform_points_direct(xt[b:b + 1, n:n + 1].contiguous(), Tt[b:b + 1], True)
        same_bits(y1[0, 0], y[b, n], ("row", b, n))
        y1 = ops.transform_points_direct(xt[b:b + 1, n:n + 1].permute(0, 2, 1).contiguous(), Tt[b:b + 1], False)
        same_bits(y1[0, :, 0], y[b, n], ("row, channel-first", b, n))
        dx1, _ = ops.transform_points_backward_direct(dyt[b:b + 1, n:n + 1].contiguous(), None, Tt[b:b + 1], True,
                                                      need_dT=False)
        same_bits(dx1[0, 0], dx[b, n], ("dx row", b, n))
    for b in range(B):
        _, dT1 = ops.transform_points_backward_direct(dyt[b:b + 1], xt[b:b + 1], None, True, need_dx=False)
        same_bits(dT1[0], dT[b], ("cloud", b))


@pytest.mark.parametrize("k,N,B", [(3, 65, 2), (64, 129, 2), (5, 1, 1)])
def test_outputs_prefilled_with_nan(k, N, B):
    """Every element of y, dx, dT (and G, norm, loss, the regulariser's dT) is written: the
    entries are called on NaN-filled buffers, straight through the C ABI."""
    from pn2 import _lib
    L = _lib.load()
    x, T, dy = data(B, N, k, 5 + k)
    xt, Tt, dyt = (torch.from_numpy(a).to(DEV) for a in (x, T, dy))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    y, dx, dT = nan(B, N, k), nan(B, N, k), nan(B, k, k)
    ws = torch.full((L.pn2_transform_workspace_bytes(B, N, k) // 8,), float("nan"), device=DEV, dtype=torch.float64)
    st = _lib.stream_ptr(xt.device)
    s = (N * k, k, 1)
    assert L.pn2_transform_points_f32(xt.data_ptr(), *s, Tt.data_ptr(), k, y.data_ptr(), *s, B, N, k, st) == 0
    assert L.pn2_transform_points_backward_f32(dyt.data_ptr(), *s, xt.data_ptr(), *s, Tt.data_ptr(), k, dx.data_ptr(),
                                               *s, dT.data_ptr(), B, N, k, ws.data_ptr(), ws.numel() * 8, st) == 0
    same_bits(y, R.transform_points(x, T))
    same_bits(dx, R.transform_points_dx(dy, T))
    same_bits(dT, R.transform_points_dT(dy, x, slab_rows()))
    G, norm, loss, gT = nan(B, k, k), nan(B), nan(1), nan(B, k, k)
    one = torch.ones(1, device=DEV)
    assert L.pn2_orthogonality_forward_f32(Tt.data_ptr(), k, B, k, G.data_ptr(), norm.data_ptr(), loss.data_ptr(),
                                           st) == 0
    assert L.pn2_orthogonality_backward_f32(Tt.data_ptr(), k, norm.data_ptr(), one.data_ptr(), B, k, gT.data_ptr(),
                                            st) == 0
    wl, wn, wG = R.orthogonality_forward(T)
    same_bits(G, wG), same_bits(norm, wn), same_bits(loss, np.array([wl]))
    same_bits(gT, R.orthogonality_backward(T, wn, 1.0))


def reg_input(B, k, seed, identity_at=None):
    rng = np.random.default_rng(seed)
    T = (np.eye(k) + 0.3 * rng.standard_normal((B, k, k)) / np.sqrt(k)).astype(np.float32)
    if identity_at is not None:
        T[identity_at] = np.eye(k, dtype=np.float32)
    return T


@pytest.mark.parametrize("B,k,identity_at", [(1, 3, None), (1, 3, 0), (3, 64, None), (3, 64, 1), (2, 5, None),
                                             (2, 5, 0)])
def test_regulariser_bits(B, k, identity_at):
    from pn2 import ops
    T = reg_input(B, k, 40 + k, identity_at)
    want_loss, want_norm, want_G = R.orthogonality_forward(T)
    Tn = torch.from_numpy(T).to(DEV)
    Tw = torch.full((B, k, k + 3), float("nan"), device=DEV)
    Tw[..., :k] = Tn
    for Tt in (Tn, Tw[..., :k]):
        loss, norm, G = ops.orthogonality_forward_direct(Tt, want_G=True)
        same_bits(G, want_G, "G")
        same_bits(G, G.transpose(1, 2), "G is bitwise symmetric")
        same_bits(norm, want_norm, "norm")
        same_bits(loss.reshape(1), np.array([want_loss]), "loss")
        for dl in (1.0, -0.37):
            dT = ops.orthogonality_backward_direct(Tt, norm, torch.tensor(dl, device=DEV))
            same_bits(dT, R.orthogonality_backward(T, want_norm, dl), ("dT", dl))
    if identity_at is not None:
        assert want_norm[identity_at] == 0 and (dT[identity_at] == 0).all() and torch.isfinite(dT).all()


def feat_close(got, ref, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = 1e-5 * ref.abs() + 1e-5 * ref.abs().max()
    assert ((got - ref).abs() <= bound).all(), (what, ((got - ref).abs() - bound).max().item())


@pytest.mark.parametrize("k,N,rows", [(3, 130, False), (64, 130, True), (64, 65, False), (5, 33, True)])
def test_autograd_against_torch_bmm(k, N, rows):
    from pn2 import train
    B = 3
    x, T, dy = data(B, N, k, 300 + k + N)
    xt, _ = layout(x, "rows" if rows else "cf")
    dyt, _ = layout(dy, "rows" if rows else "cf")
    Tt = torch.from_numpy(T).to(DEV)
    xa, Ta = xt.clone().requires_grad_(), Tt.clone().requires_grad_()
    xb, Tb = xt.clone().requires_grad_(), Tt.clone().requires_grad_()
    ya = train.transform_points(xa, Ta, rows)
    yb = torch.bmm(xb, Tb.transpose(1, 2)) if rows else torch.bmm(Tb, xb)
    feat_close(ya, yb, "y")
    ya.backward(dyt)
    yb.backward(dyt)
    feat_close(xa.grad, xb.grad, "dx")
    feat_close(Ta.grad, Tb.grad, "dT")
    # T alone needing a gradient: dx is skipped
    Tc = Tt.clone().requires_grad_()
    train.transform_points(xt, Tc, rows).backward(dyt)
    same_bits(Tc.grad, Ta.grad)


@pytest.mark.parametrize("B,k", [(1, 3), (3, 64), (2, 5)])
def test_autograd_against_torch_regulariser(B, k):
    from pn2 import ops, pointnet_utils as PU, train, tuning
    T = torch.from_numpy(reg_input(B, k, 90 + k)).to(DEV)
    Ta, Tb, Tc = (T.clone().requires_grad_() for _ in range(3))
    la = train.orthogonality_loss(Ta)
    lb = PU.feature_transform_reguliarzer(Tb)  # key 0: torch
    feat_close(la, lb, "loss")
    (la * 0.5).backward()
    (lb * 0.5).backward()
    feat_close(Ta.grad, Tb.grad, "dT")
    with tuning.override(v1_transform=1), ops.kernel_timer() as t:
        lc = PU.feature_transform_reguliarzer(Tc)
        (lc * 0.5).backward()
    assert set(t.summary()) == {"pn2_orthogonality_forward_f32", "pn2_orthogonality_backward_f32"}
    same_bits(lc.reshape(1), la.reshape(1)), same_bits(Tc.grad, Ta.grad)
    with tuning.override(v1_transform=1), ops.kernel_timer() as t, torch.no_grad():
        PU.feature_transform_reguliarzer(Tc)  # nothing to differentiate: torch
    assert not t.summary()

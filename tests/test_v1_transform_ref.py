"""tests/v1_transform_ref.py (the numpy restatement of csrc/v1_transform.hip's order rules)
pinned against CPU torch in float64: bmm forward, dx and dT by autograd,
feature_transform_reguliarzer and its gradient, the zero-norm case, G's bitwise symmetry, and
the vectorised fmaf against libm's.

Tolerances are float32 rounding bounds, evaluated in float64 from the inputs (u = 2^-24):
  a k-term float32 fma chain      |err| <= k u sum|terms|
  dT (float64 sums, one rounding) |err| <= u |ref| + N 2^-53 sum|terms|
  the regulariser                 the chain bound carried through the norm, the mean and c_b."""
import numpy as np
import pytest
import torch

import v1_transform_ref as R

U = 2.0 ** -24
SHAPES = [(1, 1, 1), (2, 7, 3), (3, 65, 5), (2, 130, 64)]  # (B, N, k)


def _data(B, N, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, N, k)).astype(np.float32)
    T = (rng.standard_normal((B, k, k)) / np.sqrt(k)).astype(np.float32)
    dy = rng.standard_normal((B, N, k)).astype(np.float32)
    return x, T, dy


def test_fmaf_is_libm_fmaf():
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(4000).astype(np.float32) for _ in range(3))
    # ties of the float64 sum: a*b needs 48 bits, c sits far above or just at the rounding point
    a2 = (1 + rng.integers(0, 2 ** 23, 2000) * 2.0 ** -23).astype(np.float32)
    b2 = (1 + rng.integers(0, 2 ** 23, 2000) * 2.0 ** -23).astype(np.float32)
    c2 = (rng.choice([2.0 ** 24, 2.0 ** 25, -2.0 ** 24, 2.0 ** 30, 0.5, -1.0], 2000) *
          (1 + rng.integers(0, 4, 2000) * 2.0 ** -23)).astype(np.float32)
    # a running chain: the accumulators the restatement actually feeds back
    x, T, _ = _data(1, 40, 64, 9)
    acc = np.zeros(40, dtype=np.float32)
    # (1 + 2^-23)(1 - 2^-23) + (2^24 + 2) = 2^24 + 3 - 2^-46: float64 rounds it onto the float32
    # tie 2^24 + 3, which then goes to even, 2^24 + 4; the fma gives 2^24 + 2
    a3, b3, c3 = (np.array([v], dtype=np.float32) for v in (1 + 2.0 ** -23, 1 - 2.0 ** -23, 2.0 ** 24 + 2))
    assert R.fmaf(a3, b3, c3)[0] == np.float32(2.0 ** 24 + 2)
    aa, bb, cc = [a, a2, a3], [b, b2, b3], [c, c2, c3]
    for j in range(64):
        aa.append(np.full(40, T[0, 3, j])), bb.append(x[0, :, j]), cc.append(acc)
        acc = R.fmaf(T[0, 3, j], x[0, :, j], acc)
    a, b, c = (np.concatenate(v) for v in (aa, bb, cc))
    got = R.fmaf(a, b, c)
    want = np.array([R.libm_fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], dtype=np.float32)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    # and it is not the twice-rounded float32(float64(a*b + c)) everywhere
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (twice.view(np.int32) != want.view(np.int32)).any()


@pytest.mark.parametrize("B,N,k", SHAPES)
def test_transform_against_torch_float64(B, N, k):
    x, T, dy = _data(B, N, k, 11 + k)
    xt = torch.from_numpy(x).double().requires_grad_()
    Tt = torch.from_numpy(T).double().requires_grad_()
    y = torch.bmm(xt, Tt.transpose(1, 2))  # rows: y[b,n,:] = T[b] x[b,n,:]
    y.backward(torch.from_numpy(dy).double())
    ax, aT, ad = np.abs(x).astype(np.float64), np.abs(T).astype(np.float64), np.abs(dy).astype(np.float64)
    got = R.transform_points(x, T)
    assert got.dtype == np.float32
    assert (np.abs(got - y.detach().numpy()) <= k * U * np.einsum("bij,bnj->bni", aT, ax) + 1e-300).all()
    # the channel-first form is the same function
    y_cf = torch.bmm(Tt, xt.transpose(1, 2)).transpose(1, 2)
    assert torch.equal(y_cf, y) or torch.allclose(y_cf, y, rtol=1e-14, atol=1e-14)
    dx = R.transform_points_dx(dy, T)
    assert (np.abs(dx - xt.grad.numpy()) <= k * U * np.einsum("bni,bij->bnj", ad, aT) + 1e-300).all()
    for slab in (1, 4, 128):
        dT = R.transform_points_dT(dy, x, slab)
        ref = Tt.grad.numpy()
        bound = U * np.abs(ref) + N * 2.0 ** -53 * np.einsum("bni,bnj->bij", ad, ax) + 1e-300
        assert dT.dtype == np.float32 and (np.abs(dT - ref) <= bound).all()


def _torch_reg(T64):
    from pn2.pointnet_utils import feature_transform_reguliarzer
    return feature_transform_reguliarzer(T64)


@pytest.mark.parametrize("B,k", [(1, 3), (2, 5), (3, 64)])
def test_regulariser_against_torch_float64(B, k):
    rng = np.random.default_rng(3 + k)
    T = (np.eye(k) + 0.3 * rng.standard_normal((B, k, k)) / np.sqrt(k)).astype(np.float32)
    Tt = torch.from_numpy(T).double().requires_grad_()
    loss = _torch_reg(Tt)
    loss.backward(torch.tensor(0.75, dtype=torch.float64))
    got_loss, norm, G = R.orthogonality_forward(T)
    np.testing.assert_array_equal(G.view(np.int32), G.transpose(0, 2, 1).view(np.int32))  # bitwise symmetric
    a = np.abs(T).astype(np.float64)
    T64 = T.astype(np.float64)
    G64 = T64 @ T64.transpose(0, 2, 1) - np.eye(k)
    E = (k + 1) * U * (a @ a.transpose(0, 2, 1) + np.eye(k))  # the chain and the subtraction
    assert (np.abs(G - G64) <= E).all()
    n64 = np.sqrt((G64 ** 2).sum((1, 2)))
    En = np.sqrt((E ** 2).sum((1, 2))) + 2 * U * n64  # |norm(G) - norm(G64)| <= ||G - G64||_F
    assert (np.abs(norm - n64) <= En).all()
    assert abs(float(got_loss) - loss.item()) <= En.mean() + U * loss.item()
    dT = R.orthogonality_backward(T, norm, np.float32(0.75))
    c64 = 2 * 0.75 / (B * n64)
    ref = Tt.grad.numpy()
    np.testing.assert_allclose(ref, c64[:, None, None] * (G64 @ T64), rtol=1e-9, atol=1e-12)  # the formula
    absGT = np.abs(G64) @ a
    bound = c64[:, None, None] * (E @ a + (k + 3) * U * absGT) + (En / n64 + 2 * U)[:, None, None] * np.abs(ref)
    assert (np.abs(dT - ref) <= bound + 1e-300).all()


def test_zero_norm_is_torchs_zero_gradient():
    """T = I: G is the zero matrix and the norm 0.  torch's CPU backward of
    torch.norm(..., dim=(1, 2)) fills the gradient with zeros there (no 0/0): so does the rule."""
    for k in (3, 64):
        T = np.stack([np.eye(k, dtype=np.float32), np.eye(k, dtype=np.float32) * np.float32(0.5)])
        for dtype in (torch.float32, torch.float64):
            Tt = torch.from_numpy(T).to(dtype).requires_grad_()
            _torch_reg(Tt).backward()
            assert torch.isfinite(Tt.grad).all() and (Tt.grad[0] == 0).all() and (Tt.grad[1] != 0).any()
        loss, norm, G = R.orthogonality_forward(T)
        assert norm[0] == 0 and (G[0] == 0).all() and norm[1] > 0
        dT = R.orthogonality_backward(T, norm, np.float32(1.0))
        assert (dT[0] == 0).all() and not np.signbit(dT[0]).any() and np.isfinite(dT).all()
        Tt = torch.from_numpy(T).double().requires_grad_()
        _torch_reg(Tt).backward()
        np.testing.assert_allclose(dT[1], Tt.grad[1].numpy(), rtol=1e-5, atol=1e-6)

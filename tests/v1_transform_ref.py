"""numpy restatement of the four order rules of csrc/v1_transform.hip (include/pn2.h): the
per-cloud transform, its backward (dx, dT) and the orthogonality regulariser, forward and
backward.  The GPU tests compare the kernels with it bit for bit; test_v1_transform_ref.py pins
it against CPU torch in float64.

The float64 chains (dT's slabs, the norm, the mean, c_b) are numpy float64 operations taken one
at a time in the stated order: exact restatements.  The float32 fma chains need a correctly
rounded fmaf.  This Python has no math.fma, and calling libm's fmaf through ctypes once per
element costs seconds at the test shapes, so ``fmaf`` below is vectorised: the product of two
float32 is exact in float64, the float64 sum with the addend is rounded TO ODD (round to nearest,
then repaired with the exact error of the addition), and rounding that to float32 is then the
correctly rounded fma (53 >= 2*24 + 2 bits).  test_v1_transform_ref.py checks it element by
element against libm's fmaf, ties and chain values included.  Finite, normal-range values only
(what the tests use)."""
import ctypes
import ctypes.util

import numpy as np

MAX_K = 64


def fmaf(a, b, c):
    """float32(a * b + c) with one rounding, elementwise over float32 arrays."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    p = a * b                      # exact: 24 + 24 bits
    t = p + c                      # round to nearest ...
    bb = t - p
    err = (p - (t - bb)) + (c - bb)  # ... and its exact error (TwoSum)
    bits = np.atleast_1d(t).view(np.int64)
    even = (bits & 1) == 0
    fix = even & (np.atleast_1d(err) != 0)
    up = np.nextafter(np.atleast_1d(t), np.where(np.atleast_1d(err) > 0, np.inf, -np.inf))
    odd = np.where(fix, up, np.atleast_1d(t)).reshape(np.shape(t))
    return odd.astype(np.float32)


_libm = None


def libm_fmaf(a, b, c):
    """libm's fmaf on three Python floats holding float32 values (the pin of ``fmaf``)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fmaf.restype = ctypes.c_float
        _libm.fmaf.argtypes = [ctypes.c_float] * 3
    return _libm.fmaf(a, b, c)


def _chain(terms_a, terms_b):
    """acc = fmaf(a_r, b_r, acc) over r = 0 .. from +0.0f; terms_*: sequences of broadcastable
    float32 arrays, one per step."""
    acc = None
    for a, b in zip(terms_a, terms_b):
        if acc is None:
            acc = np.zeros(np.broadcast(a, b).shape, dtype=np.float32)
        acc = fmaf(a, b, acc)
    return acc


def transform_points(x, T):
    """x [B,N,k], T [B,k,k] float32 -> y[b,n,i] = sum_j T[b,i,j] x[b,n,j], one fma chain over
    ascending j from +0.0f."""
    x = np.asarray(x, dtype=np.float32)
    T = np.asarray(T, dtype=np.float32)
    k = T.shape[1]
    return _chain([T[:, None, :, j] for j in range(k)], [x[:, :, j, None] for j in range(k)])


def transform_points_dx(dy, T):
    """dx[b,n,j] = sum_i dy[b,n,i] T[b,i,j], one fma chain over ascending i from +0.0f."""
    dy = np.asarray(dy, dtype=np.float32)
    T = np.asarray(T, dtype=np.float32)
    k = T.shape[1]
    return _chain([dy[:, :, i, None] for i in range(k)], [T[:, None, i, :] for i in range(k)])


def transform_points_dT(dy, x, slab_rows):
    """dT[b,i,j]: float64 slab partials over ascending n from +0.0 (exact products), added in
    ascending slab order from +0.0, rounded to float32 once."""
    dy = np.asarray(dy, dtype=np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    B, N, k = x.shape
    total = np.zeros((B, k, k), dtype=np.float64)
    for lo in range(0, N, slab_rows):
        part = np.zeros((B, k, k), dtype=np.float64)
        for n in range(lo, min(lo + slab_rows, N)):
            part = part + dy[:, n, :, None] * x[:, n, None, :]
        total = total + part
    return total.astype(np.float32)


def gram_minus_identity(T):
    """G[b] = T[b] T[b]^T - I: an fma chain over ascending l per element, then one float32
    subtraction of 1 on the diagonal."""
    T = np.asarray(T, dtype=np.float32)
    k = T.shape[1]
    G = _chain([T[:, :, None, l] for l in range(k)], [T[:, None, :, l] for l in range(k)])
    d = np.arange(k)
    G[:, d, d] = G[:, d, d] - np.float32(1.0)
    return G


def orthogonality_forward(T):
    """-> (loss float32, norm [B] float32, G [B,k,k] float32)."""
    G = gram_minus_identity(T)
    B, k, _ = G.shape
    sq = G.astype(np.float64).reshape(B, k * k) ** 2
    acc = np.zeros(B, dtype=np.float64)
    for e in range(k * k):  # row-major (i, j)
        acc = acc + sq[:, e]
    norm = np.sqrt(acc).astype(np.float32)
    s = np.float64(0.0)
    for b in range(B):
        s = s + np.float64(norm[b])
    return np.float32(s / np.float64(B)), norm, G


def orthogonality_backward(T, norm, dloss):
    """dT[b] = c_b * (G[b] T[b]); c_b = float32(2 dloss / (B norm[b])) in float64, +0 where
    norm[b] == 0."""
    T = np.asarray(T, dtype=np.float32)
    G = gram_minus_identity(T)
    B, k, _ = T.shape
    GT = _chain([G[:, :, l, None] for l in range(k)], [T[:, l, None, :] for l in range(k)])
    norm = np.asarray(norm, dtype=np.float32)
    c = np.zeros(B, dtype=np.float32)
    nz = norm != 0
    c[nz] = ((2.0 * np.float64(np.float32(dloss))) / (np.float64(B) * norm[nz].astype(np.float64))).astype(np.float32)
    return GT * c[:, None, None]

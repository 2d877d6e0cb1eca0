"""The training kernels of csrc/train.hip restated in numpy float64, operation by operation as
include/pn2.h documents them (batch-statistics BatchNorm, ReLU, max over K rows, and their
backward).  Every input is the float32 array the kernel receives, widened to float64; nothing
here rounds to float32, so a result is the exact-arithmetic value up to float64 noise.

  stats       column mean, biased variance, invstd; torch's running-stat update
  sxhat       sum over rows of xhat with float32 statistics
  apply       A = relu((Y - mean) * invstd * gamma + beta)
  group_max   max over each K rows and its first argmax, NaN above every number
  backward    dXn, dbeta, dgamma, dY, dbias and the magnitudes the error bounds are made of

tests/test_train_ref.py pins these to torch's float64 autograd; tests/test_gpu_train_kernels.py
compares the kernels with them.  The second half of the file makes that test's inputs, so that
the CPU test can check them (ReLU-mask ambiguity) without a device."""
import collections

import numpy as np

U = 2.0 ** -24       # float32 unit roundoff
TINY = 2.0 ** -40    # floor of the float64-accumulated quantities, relative to their scale


def f64(a):
    return np.asarray(a, dtype=np.float64)


def colsum(a):
    """Column sums of [M, C] by numpy's pairwise summation (along a contiguous axis; a sum over
    axis 0 of row-major rows adds them one after the other, M roundings deep)."""
    return np.ascontiguousarray(f64(a).T).sum(axis=1)


# ------------------------------------------------------------------ the four operations
Stats = collections.namedtuple("Stats", ["mean", "var", "invstd", "running_mean", "running_var"])


def stats(Y, eps, momentum=0.0, rm=None, rv=None):
    """Y [M, C].  Two-pass mean and biased variance, invstd = 1/sqrt(var + eps); with
    momentum > 0 the running statistics after the step (the unbiased variance enters
    running_var when M > 1), else rm / rv as given."""
    Y = f64(Y)
    M = Y.shape[0]
    mean = colsum(Y) / M
    var = colsum((Y - mean) ** 2) / M
    invstd = 1.0 / np.sqrt(var + eps)
    if momentum > 0.0 and rm is not None:
        unb = var * M / (M - 1) if M > 1 else var
        rm = (1.0 - momentum) * f64(rm) + momentum * mean
        rv = (1.0 - momentum) * f64(rv) + momentum * unb
    return Stats(mean, var, invstd, rm, rv)


def sxhat(Y, mean32, invstd32):
    """sum_r (Y[r] - mean32) * invstd32 as the header defines it: (sum y - M*mean32)*invstd32."""
    Y = f64(Y)
    return (colsum(Y) - Y.shape[0] * f64(mean32)) * f64(invstd32)


Apply = collections.namedtuple("Apply", ["A", "pre", "xhat", "mag"])


def apply(Y, mean32, invstd32, gamma, beta, relu=True):
    """-> A, the value before the ReLU, xhat, and mag = |xhat*gamma| + |beta| per element."""
    xhat = (f64(Y) - f64(mean32)) * f64(invstd32)
    xg = xhat * f64(gamma)
    pre = xg + f64(beta)
    A = np.where(pre > 0.0, pre, 0.0) if relu else pre
    return Apply(A, pre, xhat, np.abs(xg) + np.abs(f64(beta)))


def group_max(A, K):
    """A [G*K, C] -> (out [G, C] in A's dtype, arg [G, C] int32): the max over each K rows and
    its first index; a NaN is the maximum (the first NaN's index), as torch.max."""
    A = np.asarray(A)
    G, C = A.shape[0] // K, A.shape[1]
    a = A.reshape(G, K, C)
    nan = np.isnan(a)
    key = np.where(nan, np.inf, a)
    arg = np.where(nan.any(1), np.argmax(nan, axis=1), np.argmax(key, axis=1))
    out = np.take_along_axis(a, arg[:, None, :], 1)[:, 0]
    return out, arg.astype(np.int32)


def scatter(dOut, arg, K):
    """dA [G*K, C] of the max: dOut[g][c] on row g*K + arg[g][c], 0 elsewhere."""
    dOut = f64(dOut)
    G, C = dOut.shape
    dA = np.zeros((G, K, C))
    np.put_along_axis(dA, np.asarray(arg, np.int64)[:, None, :], dOut[:, None, :], 1)
    return dA.reshape(G * K, C)


Backward = collections.namedtuple("Backward", ["dXn", "dbeta", "dgamma", "dY", "dbias",
                                               "sum_abs_dXn", "sum_abs_dXn_xhat", "dY_mag"])


def backward(Y, mean32, invstd32, gamma, beta, dA=None, dOut=None, arg=None, K=0, sxhat=None,
             relu=True):
    """dA dense [M, C], or None: scattered from (dOut, arg, K).  dXn = dA * [pre > 0] (dA without
    the ReLU), dbeta = S1 = sum dXn, dgamma = S2 = sum dXn*xhat,
    dY = gamma*invstd*(dXn - S1/M - xhat*S2/M), dbias = -gamma*invstd*(S2/M)*sxhat (the header's
    closed form of sum_r dY; None without sxhat).  The magnitudes: sum |dXn|, sum |dXn*xhat| per
    column and |dXn| + |S1/M| + |xhat*S2/M| per element."""
    fw = apply(Y, mean32, invstd32, gamma, beta, relu)
    M = fw.xhat.shape[0]
    d = f64(dA) if dA is not None else scatter(dOut, arg, K)
    dXn = np.where(fw.pre > 0.0, d, 0.0) if relu else d
    S1 = colsum(dXn)
    S2 = colsum(dXn * fw.xhat)
    gi = f64(gamma) * f64(invstd32)
    dY = gi * (dXn - S1 / M - fw.xhat * (S2 / M))
    dbias = None if sxhat is None else -gi * (S2 / M) * f64(sxhat)
    mag = np.abs(dXn) + np.abs(S1 / M) + np.abs(fw.xhat * (S2 / M))
    return Backward(dXn, S1, S2, dY, dbias, colsum(np.abs(dXn)), colsum(np.abs(dXn * fw.xhat)), mag)


def ambiguous(fw):
    """Elements whose ReLU mask float32 may legitimately decide the other way: the value before
    the ReLU is within the forward's float32 error bound of zero."""
    return np.abs(fw.pre) <= 8.0 * U * fw.mag


# ------------------------------------------------------------------ the host's chunking
def chunk_rows(M, C):
    """csrc/train.hip chunk_rows: 1024 rows, halved down to 64 while column tiles x chunks
    would be fewer than 2048 blocks."""
    tiles = (C + 63) // 64
    ch = 1024
    while ch > 64 and tiles * ((M + ch - 1) // ch) < 2048:
        ch >>= 1
    return ch


def chunks(M, C):
    return (M + chunk_rows(M, C) - 1) // chunk_rows(M, C)


# ------------------------------------------------------------------ inputs of the GPU tests
EPS = 1e-5

# (M, C, pad of ld, pad of the second stride (lda / ldd / ldo), pad of ldy): a pad of 3 breaks
# the 16-byte alignment of the rows (scalar kernels), 4 keeps it (vector kernels with padding).
# C: scalar only (1, 3, 5, 63, 65), vector (64, 68), two column tiles (65, 68, 130) with a
# partial one; M: below / at / above the 64-row chunk and the 4 / 16 row lanes, 4097 and 8327
# rows = 65 and 131 chunk partials (wave_col_sum's second and third round).
DENSE_CASES = [
    (2, 1, 0, 0, 0), (3, 3, 3, 0, 4), (63, 5, 4, 3, 0), (64, 63, 0, 4, 3), (65, 64, 0, 0, 0),
    (65, 64, 4, 4, 4), (97, 64, 3, 0, 0), (97, 64, 0, 3, 0), (97, 64, 0, 0, 3), (97, 64, 4, 0, 0),
    (97, 64, 0, 4, 0), (97, 64, 0, 0, 4), (97, 65, 3, 4, 3), (64, 68, 4, 4, 4), (4097, 68, 0, 0, 0),
    (4097, 5, 3, 3, 3), (8327, 130, 3, 4, 0), (8327, 64, 4, 0, 4), (3, 130, 0, 0, 0),
]
BIG_CASE = (8197, 2048, 0, 0, 0)  # 128-row chunks, 65 of them, the last of 5 rows
# (G, K, C, pads): dA scattered from the max, M = G*K
SCATTER_CASES = [
    (97, 1, 5, 0, 0, 0), (33, 3, 64, 0, 0, 0), (33, 3, 64, 4, 4, 4), (33, 3, 64, 0, 3, 0),
    (131, 32, 65, 3, 4, 3), (84, 100, 68, 0, 0, 0), (84, 100, 68, 4, 0, 3), (5, 100, 3, 4, 3, 0),
    (2, 32, 1, 0, 0, 0), (4200, 3, 130, 0, 4, 4),
]
# the documented workspace against the gather pass's partials: K = 3 asked for 2730 partials
# of the 2048 the workspace holds; K = 4 is the power-of-two control
WORKSPACE_CASES = [(174678, 3, 4, 0, 0, 0), (174678, 4, 4, 0, 0, 0)]

Inputs = collections.namedtuple("Inputs", ["Y", "gamma", "beta", "rm", "rv", "d", "arg", "special"])


def special_columns(C):
    """-> dict kind -> column.  From 5 columns on each kind has its own (the last four); below,
    the two data kinds sit on the first columns and the two gamma kinds on the last ones."""
    if C >= 5:
        return {"mean30": C - 1, "const": C - 2, "gamma_neg": C - 3, "gamma_zero": C - 4}
    sp = {"mean30": 0, "gamma_neg": C - 1}
    if C >= 2:
        sp["const"] = 1
    if C >= 3:
        sp["gamma_zero"] = C - 2
    return sp


def case_seed(M, C, K=0):
    return 131 * M + 7 * C + K


def make_inputs(M, C, seed, G=0, K=0):
    """float32 inputs of one case: N(0,1) columns, one column N(30, 0.5) (a float32 sum of
    squares is visibly wrong there), one constant column (var = 0), one gamma < 0, one gamma = 0;
    running statistics; the incoming gradient d ([M, C], or [G, C] with a random arg when K)."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((M, C)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.uniform(-0.3, 0.3, C).astype(np.float32)
    sp = special_columns(C)
    Y[:, sp["mean30"]] = (30.0 + 0.5 * rng.standard_normal(M)).astype(np.float32)
    if "const" in sp:
        Y[:, sp["const"]] = np.float32(1.7)
    gamma[sp["gamma_neg"]] = np.float32(-0.8)
    if "gamma_zero" in sp:
        gamma[sp["gamma_zero"]] = 0.0
    rm = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    rv = rng.uniform(0.5, 1.5, C).astype(np.float32)
    arg = None
    if K:
        d = rng.standard_normal((G, C)).astype(np.float32)
        arg = rng.integers(0, K, (G, C)).astype(np.int32)
    else:
        d = rng.standard_normal((M, C)).astype(np.float32)
    return Inputs(Y, gamma, beta, rm, rv, d, arg, sp)


def rounded_stats(inp):
    """The statistics the apply / backward tests hand to the kernel: the reference's, rounded
    to float32 (not the stats kernel's output: each entry point is judged on its own)."""
    s = stats(inp.Y, EPS)
    return s.mean.astype(np.float32), s.invstd.astype(np.float32)


def zero_ambiguous(inp, mean32, invstd32, relu):
    """The incoming gradient with the ReLU-ambiguous elements zeroed (d[r][c], or dOut[g][c] when
    the ambiguous element is the group's argmax row), and the share of ambiguous elements among
    all elements of the columns that are not ambiguous by construction (gamma = 0 and the
    constant column: xhat*gamma is 0 or noise there)."""
    d = inp.d.copy()
    if not relu:
        return d, 0.0
    amb = ambiguous(apply(inp.Y, mean32, invstd32, inp.gamma, inp.beta, True))
    count = np.ones(inp.Y.shape[1], bool)
    for kind in ("const", "gamma_zero"):
        if kind in inp.special:
            count[inp.special[kind]] = False
    share = float(amb[:, count].sum()) / max(1, amb[:, count].size)
    if inp.arg is None:
        d[amb] = 0.0
    else:
        G, C = inp.arg.shape
        K = inp.Y.shape[0] // G
        at = np.take_along_axis(amb.reshape(G, K, C), inp.arg.astype(np.int64)[:, None, :], 1)[:, 0]
        d[at] = 0.0
    return d, share

"""The kernels behind the SA layers' differentiable eval forward (csrc/train.hip, ABI 19), called
through the C ABI:

  pn2_bn_relu_group_max_f32   against pn2_bn_relu_apply_f32 followed by pn2_group_max_f32, bit
                              for bit in `out` and `arg` (the header's contract)
  pn2_bn_relu_backward_f32    with PN2_LAYER_FROZEN_STATS against a float64 restatement:
                              tests/train_ref.py's backward with the batch-statistics correction
                              terms dropped (mean / invstd are constants of the backward)

Inputs, special columns and the float64 arithmetic come from tests/train_ref.py; runners, bounds
and the ReLU-ambiguity masking are those of tests/test_gpu_train_kernels.py for the same
quantities (u = 2^-24):
  dbeta   2u|ref| + 2^-40 sum|dXn|        dgamma  4u sum|dXn xhat|
  dY      8u |gamma invstd| |dXn|         (that file's bound with its two correction terms at 0)
  dbias   2u|ref| + |gamma invstd| * 2^-40 sum|dXn|   (gamma*invstd*dbeta from the float64 sum:
          one rounding to float32 plus the sum's own floor)
The statistics handed to the kernel are running statistics: mean = rm, invstd = 1/sqrt(rv + eps)
rounded to float32."""
import numpy as np
import pytest
import torch

import train_ref as tr
import test_gpu_train_kernels as tk
from test_gpu_train_kernels import rows_in, rows_out, take_rows, vec, within, workspace

pytestmark = pytest.mark.gpu

U, TINY, EPS = tr.U, tr.TINY, tr.EPS
NO_RELU, FROZEN = 1, 2
SENTINEL = tk.SENTINEL


# ------------------------------------------------------------------ fused apply + max
def _max_case(G, K, C, seed):
    """Y of small integers (exact ties survive the affine map: equal inputs, equal roundings),
    zeros of both signs, a -inf column in group 0, NaNs in the last group's last column, and a
    column whose values all map below zero (ReLU: max 0 at index 0)."""
    rng = np.random.default_rng(seed)
    y = rng.integers(-3, 4, (G, K, C)).astype(np.float32)
    y = np.where((y == 0) & (rng.random((G, K, C)) < 0.5), np.float32(-0.0), y)
    mean = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    invstd = (1.0 / np.sqrt(rng.uniform(0.5, 1.5, C) + EPS)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.uniform(-0.3, 0.3, C).astype(np.float32)
    if C > 2:
        gamma[C // 2] = np.float32(-0.8)  # a decreasing map: the max sits on the smallest input
    neg = 1 if C > 1 else 0
    y[:, :, neg] = -5.0 - np.abs(y[:, :, neg])
    gamma[neg] = abs(gamma[neg])
    y[0, :, 0] = -np.inf
    gamma[0] = abs(gamma[0])
    y[G - 1, rng.integers(0, K, 3), C - 1] = np.nan
    return y.reshape(G * K, C), mean, invstd, gamma, beta, neg


def _two_calls(L, lib, Yp, G, K, C, ld, dev, flags, st):
    """The reference: apply into a dense A, then the max."""
    A = torch.empty(G * K, C, device="cuda")
    lib.check(L.pn2_bn_relu_apply_f32(Yp, G * K, C, ld, *dev, A.data_ptr(), C, flags, st), "pn2_bn_relu_apply_f32")
    out = torch.empty(G, C, device="cuda")
    arg = torch.empty(G, C, dtype=torch.int32, device="cuda")
    lib.check(L.pn2_group_max_f32(A.data_ptr(), G, K, C, C, out.data_ptr(), C, arg.data_ptr(), st), "pn2_group_max_f32")
    return out.cpu().numpy(), arg.cpu().numpy()


# (pad of ld, pad of ldo, floats Y starts past a 16-byte boundary)
LAYOUTS = [(0, 0, 0), (3, 1, 0), (4, 4, 0), (0, 0, 1), (4, 0, 1)]


@pytest.mark.parametrize("C", [1, 5, 64, 65])
@pytest.mark.parametrize("K", [1, 2, 8, 9, 17, 255, 256, 257, 384, 385])
def test_fused_max_equals_apply_then_max(K, C):
    """Around the narrow kernels' 8- and 4-row rounds, the switch to the wide kernels at K = 256
    and their 128- / 64-row rounds; one and two column tiles; vector (C = 64, aligned, strides
    multiples of 4) and scalar paths; G = 1 and 3."""
    lib, L = tk._lib()
    for G in (1, 3):
        y, mean, invstd, gamma, beta, neg = _max_case(G, K, C, 1000 * G + 10 * K + C)
        params = [vec(a) for a in (mean, invstd, gamma, beta)]
        dev = [t.data_ptr() for t in params]
        for relu in (True, False):
            flags = 0 if relu else NO_RELU
            for pad, pad_o, offset in LAYOUTS:
                keep, Yp, ld = rows_in(y, pad, offset)
                st = tk._st(keep)
                want, want_arg = _two_calls(L, lib, Yp, G, K, C, ld, dev, flags, st)
                out, op, ldo = rows_out(G, C, pad_o)
                arg = torch.full((G, C), -1, dtype=torch.int32, device="cuda")
                lib.check(L.pn2_bn_relu_group_max_f32(Yp, G, K, C, ld, *dev, op, ldo, arg.data_ptr(), flags, st),
                          "pn2_bn_relu_group_max_f32")
                torch.cuda.synchronize()
                what = "G=%d relu=%s layout=%s" % (G, relu, (pad, pad_o, offset))
                np.testing.assert_array_equal(arg.cpu().numpy(), want_arg, err_msg=what)
                np.testing.assert_array_equal(take_rows(out, C, "max").view(np.int32), want.view(np.int32),
                                              err_msg=what)
                # the constructed columns did what they were made for
                if C < 5:  # the kinds share columns
                    continue
                if relu:
                    assert (want[:, neg] == 0).all() and (want_arg[:, neg] == 0).all()
                    assert want[0, 0] == 0 and want_arg[0, 0] == 0  # relu(-inf) = 0 on every row
                else:
                    assert np.isneginf(want[0, 0]) and want_arg[0, 0] == 0
                    assert np.isnan(want[G - 1, C - 1])
        # and the values are the float64 restatement's (the reference chain is not vacuous)
        ref = tr.apply(y, mean, invstd, gamma, beta, True)
        finite = np.isfinite(ref.A).all(0)
        ref_max = np.nanmax(np.where(np.isfinite(ref.A), ref.A, -np.inf).reshape(G, K, C), axis=1)
        keep, Yp, ld = rows_in(y, 0)
        got, _ = _two_calls(L, lib, Yp, G, K, C, ld, dev, 0, tk._st(keep))
        torch.cuda.synchronize()
        np.testing.assert_allclose(got[:, finite], ref_max[:, finite], rtol=1e-5, atol=1e-6)


def test_fused_max_many_groups():
    """More groups than one block row of either narrow kernel, K below the wide switch, and
    G = 65536 groups of K = 256 (past the wide kernels' range: the narrow kernel again)."""
    lib, L = tk._lib()
    for G, K, C in ((70, 32, 68), (65536, 256, 4)):
        rng = np.random.default_rng(G + K)
        y = rng.standard_normal((G * K, C)).astype(np.float32)
        params = [vec(rng.uniform(0.5, 1.5, C).astype(np.float32)) for _ in range(4)]
        dev = [t.data_ptr() for t in params]
        keep, Yp, ld = rows_in(y, 0)
        st = tk._st(keep)
        want, want_arg = _two_calls(L, lib, Yp, G, K, C, ld, dev, 0, st)
        out, op, ldo = rows_out(G, C, 0)
        arg = torch.full((G, C), -1, dtype=torch.int32, device="cuda")
        lib.check(L.pn2_bn_relu_group_max_f32(Yp, G, K, C, ld, *dev, op, ldo, arg.data_ptr(), 0, st),
                  "pn2_bn_relu_group_max_f32")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(arg.cpu().numpy(), want_arg)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


def test_custom_op_equals_the_c_entry():
    """torch.ops.pn2.bn_relu_group_max (pn2/ops.py, what pn2.train's frozen mode calls) against
    apply then max through the C ABI: shapes, dtypes and bits, with and without the ReLU; and
    the shape errors of its Python wrapper."""
    from pn2 import ops
    lib, L = tk._lib()
    G, K, C = 5, 12, 68
    y, mean, invstd, gamma, beta, _ = _max_case(G, K, C, 77)
    Y = vec(y)
    params = [vec(a) for a in (mean, invstd, gamma, beta)]
    for relu in (True, False):
        want, want_arg = _two_calls(L, lib, Y.data_ptr(), G, K, C, C, [t.data_ptr() for t in params],
                                    0 if relu else NO_RELU, tk._st(Y))
        for fn in (torch.ops.pn2.bn_relu_group_max, ops.bn_relu_group_max_direct):
            out, arg = fn(Y, K, *params, relu)
            assert out.shape == (G, C) and out.dtype == torch.float32
            assert arg.shape == (G, C) and arg.dtype == torch.int32
            np.testing.assert_array_equal(arg.cpu().numpy(), want_arg)
            np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    with pytest.raises(ValueError):
        ops.bn_relu_group_max_direct(Y, 7, *params, True)  # G*K rows
    with pytest.raises(ValueError):
        ops.bn_relu_group_max_direct(Y, K, params[0][:4], *params[1:], True)


# ------------------------------------------------------------------ frozen backward
def frozen_backward(Y, mean32, invstd32, gamma, beta, dA=None, dOut=None, arg=None, K=0, relu=True):
    """train_ref.backward with mean / invstd constant: dXn = dA*[pre > 0] (dA without the ReLU),
    dbeta = sum dXn, dgamma = sum dXn*xhat, dY = gamma*invstd*dXn, dbias = gamma*invstd*dbeta."""
    fw = tr.apply(Y, mean32, invstd32, gamma, beta, relu)
    d = tr.f64(dA) if dA is not None else tr.scatter(dOut, arg, K)
    dXn = np.where(fw.pre > 0.0, d, 0.0) if relu else d
    S1, S2 = tr.colsum(dXn), tr.colsum(dXn * fw.xhat)
    gi = tr.f64(gamma) * tr.f64(invstd32)
    return dict(dbeta=S1, dgamma=S2, dY=gi * dXn, dbias=gi * S1, sum_abs_dXn=tr.colsum(np.abs(dXn)),
                sum_abs_dXn_xhat=tr.colsum(np.abs(dXn * fw.xhat)), abs_dXn=np.abs(dXn))


def running_stats32(inp):
    return inp.rm, (1.0 / np.sqrt(tr.f64(inp.rv) + EPS)).astype(np.float32)


def run_frozen(inp, mean32, invstd32, d, pads, relu, K, dbias, offset):
    lib, L = tk._lib()
    M, C = inp.Y.shape
    pad, pad_d, pad_y = pads
    keep, Yp, ld = rows_in(inp.Y, pad, offset)
    keep_d, dp, ldd = rows_in(d, pad_d)
    dY, dYp, ldy = rows_out(M, C, pad_y)
    dev = [vec(a) for a in (mean32, invstd32, inp.gamma, inp.beta)]
    arg = vec(inp.arg, np.int32) if K else None
    outs = [torch.full((C,), float(SENTINEL), device="cuda") for _ in range(3)]  # dgamma, dbeta, dbias
    ws, n = workspace(L, M, C)
    flags = FROZEN | (0 if relu else NO_RELU)
    lib.check(L.pn2_bn_relu_backward_f32(Yp, M, C, ld, *[t.data_ptr() for t in dev], 0 if K else dp, ldd,
                                         dp if K else 0, ldd, arg.data_ptr() if K else 0, K, 0, dYp, ldy,
                                         outs[0].data_ptr(), outs[1].data_ptr(),
                                         outs[2].data_ptr() if dbias else 0, ws.data_ptr(), n, flags,
                                         tk._st(keep)), "pn2_bn_relu_backward_f32")
    torch.cuda.synchronize()
    dgamma, dbeta, db = [t.cpu().numpy() for t in outs]
    if not dbias:
        assert (db.view(np.int32) == SENTINEL.view(np.int32)).all()
    return take_rows(dY, C, "dY"), dgamma, dbeta, db if dbias else None


def check_frozen(inp, pads, relu, K=0, dbias=True, offset=0):
    M, C = inp.Y.shape
    mean32, invstd32 = running_stats32(inp)
    d, share = tr.zero_ambiguous(inp, mean32, invstd32, relu)
    assert share <= 1e-4, "ReLU-ambiguous share %g" % share
    dY, dgamma, dbeta, db = run_frozen(inp, mean32, invstd32, d, pads, relu, K, dbias, offset)
    kw = dict(dOut=d, arg=inp.arg, K=K) if K else dict(dA=d)
    ref = frozen_backward(inp.Y, mean32, invstd32, inp.gamma, inp.beta, relu=relu, **kw)
    gi = np.abs(tr.f64(inp.gamma) * tr.f64(invstd32))
    within("frozen dbeta", dbeta, ref["dbeta"], 2 * U * np.abs(ref["dbeta"]) + TINY * ref["sum_abs_dXn"])
    within("frozen dgamma", dgamma, ref["dgamma"], 4 * U * ref["sum_abs_dXn_xhat"])
    within("frozen dY", dY, ref["dY"], 8 * U * gi[None, :] * ref["abs_dXn"])
    if dbias:
        tol = 2 * U * np.abs(ref["dbias"]) + gi * TINY * ref["sum_abs_dXn"]
        within("frozen dbias", db, ref["dbias"], tol)
        if M >= 64 and C >= 5:  # definite values: the batch-statistics form (about 0) is far outside
            assert (np.abs(ref["dbias"]) > 10 * tol).any()
    # the correction terms are really gone: dY is zero wherever dXn is
    assert (dY[ref["abs_dXn"] == 0.0] == 0.0).all()


DENSE = tr.DENSE_CASES + [(2, 1, 3, 3, 3), (97, 65, 0, 0, 0), (4097, 68, 4, 4, 4)]


@pytest.mark.parametrize("dbias", [True, False], ids=["dbias", "nodbias"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("M,C,pad,pad_d,pad_y", DENSE)
def test_frozen_backward_dense(M, C, pad, pad_d, pad_y, relu, dbias):
    check_frozen(tk._inputs(M, C), (pad, pad_d, pad_y), relu, dbias=dbias)


@pytest.mark.parametrize("dbias", [True, False], ids=["dbias", "nodbias"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("G,K,C,pad,pad_o,pad_y", tr.SCATTER_CASES)
def test_frozen_backward_scatter(G, K, C, pad, pad_o, pad_y, relu, dbias):
    check_frozen(tk._inputs(G * K, C, G, K), (pad, pad_o, pad_y), relu, K=K, dbias=dbias)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_frozen_backward_unaligned_base(relu):
    """C = 64 with Y one float past a 16-byte boundary: the scalar kernels, dense and scattered."""
    check_frozen(tk._inputs(65, 64), (0, 0, 0), relu, offset=1)
    check_frozen(tk._inputs(33 * 3, 64, 33, 3), (0, 0, 0), relu, K=3, offset=1)


def test_unflagged_backward_is_the_batch_statistics_one():
    """Without the flag the entry is the train-mode backward, judged by that file's own check
    (one dense, one scattered case); tests/test_gpu_train_kernels.py pins the rest."""
    tk.check_backward(tk._inputs(97, 64), (0, 0, 0), True)
    tk.check_backward(tk._inputs(131 * 32, 65, 131, 32), (3, 4, 3), True, K=32)

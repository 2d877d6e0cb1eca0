"""The five training entry points of csrc/train.hip (pn2_bn_train_stats_f32, pn2_bn_relu_apply_f32,
pn2_bn_train_forward_f32, pn2_group_max_f32, pn2_bn_relu_backward_f32) called directly through
the C ABI and compared with tests/train_ref.py, the numpy float64 restatement of include/pn2.h.

Shapes (train_ref.DENSE_CASES / SCATTER_CASES) reach the scalar and the 16-byte kernels, one and
two column tiles with a partial one, the 4 / 16 row lanes and the 64-row chunk from both sides,
65 and 131 chunk partials, a 128-row chunk with a ragged last one, and every row stride at C,
C + 3 and C + 4.  Input padding is NaN; output padding holds a sentinel that must survive.
For apply and backward the statistics are the reference's rounded to float32, not the stats
kernel's output, so each entry point is judged on its own.

Bounds, from the arithmetic the header documents (u = 2^-24, ref = the restatement; float64
accumulations get a 2^-40 floor relative to what they sum):
  mean, running_mean   2u|ref| + 2^-40 max|Y|        invstd, running_var   relative 2u + 2^-40 E[y^2]/(var+eps)
  sxhat   relative 1e-6 + 2^-40 M max|Y| invstd, against (sum y - M mean)*invstd of the returned statistics
  A       8u (|xhat gamma| + |beta|)                   dbeta   2u|ref| + 2^-40 sum|dXn|
  dgamma  4u sum|dXn xhat|                             dY      8u |gamma invstd| (|dXn| + |S1/M| + |xhat S2/M|)
  dbias   2u|ref| + |gamma invstd sxhat / M| * (dgamma bound)
Where the value before the ReLU is within the forward bound of zero float32 may mask the other
way; the incoming gradient is zeroed there (at most 1e-4 of a case's elements, asserted).

With PN2_TRAIN_ERROR_RATIOS=<file> the worst error/bound ratio of each quantity is written there
when the module finishes (profiles/train_kernels/error_ratios.json is such a record)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import train_ref as tr

pytestmark = pytest.mark.gpu

U, TINY, EPS = tr.U, tr.TINY, tr.EPS
NO_RELU = 1  # PN2_LAYER_NO_RELU
SENTINEL = np.float32(-777.25)
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_ratios():
    yield
    path = os.environ.get("PN2_TRAIN_ERROR_RATIOS")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"error_over_bound_max": {k: float("%.4g" % v) for k, v in sorted(RATIOS.items())}},
                      f, indent=1)
            f.write("\n")


def within(name, got, ref, tol):
    """Every |got - ref| <= tol; the worst error/bound ratio is printed and recorded first."""
    got, ref, tol = tr.f64(got), tr.f64(ref), tr.f64(tol)
    assert got.shape == ref.shape, name
    assert np.isfinite(got).all(), name + ": not finite"
    err = np.abs(got - ref)
    ratio = np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    print("%s: worst error/bound %.3g" % (name, worst))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    assert worst <= 1.0, "%s: error/bound %.3g at %s (got %r, ref %r)" % (
        name, worst, at, got[at], ref[at])


@functools.lru_cache(maxsize=2)
def _inputs(M, C, G=0, K=0):
    return tr.make_inputs(M, C, tr.case_seed(M, C, K), G, K)


def _lib():
    from pn2 import _lib as lib
    return lib, lib.load()


def _st(t):
    from pn2.ops import _stream
    return _stream(t)


def rows_in(a, pad, offset=0):
    """a [M, C] -> device rows of stride C + pad, padding NaN, starting `offset` floats past an
    allocation's (16-byte aligned) base.  -> (keep-alive tensor, data pointer, stride)."""
    M, C = a.shape
    host = np.full((M, C + pad), np.nan, np.float32)
    host[:, :C] = a
    flat = torch.empty(M * (C + pad) + 4, device="cuda")
    flat[offset:offset + host.size] = torch.from_numpy(host.reshape(-1)).cuda()
    return flat, flat.data_ptr() + 4 * offset, C + pad


def rows_out(M, C, pad):
    t = torch.full((M, C + pad), float(SENTINEL), device="cuda")
    return t, t.data_ptr(), C + pad


def take_rows(t, C, what):
    """The [M, C] result of an output buffer, whose padding must still hold the sentinel."""
    host = t.cpu().numpy()
    assert (host[:, C:].view(np.int32) == SENTINEL.view(np.int32)).all(), what + ": padding written"
    return host[:, :C]


def vec(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def workspace(L, M, C):
    """Exactly the documented size."""
    n = int(L.pn2_bn_train_workspace_bytes(M, C))
    assert n == (tr.chunks(M, C) * 2 * C + 3 * C) * 8
    return torch.empty(n, dtype=torch.uint8, device="cuda"), n


# ------------------------------------------------------------------ statistics
def run_stats(inp, pad, momentum, running=True, offset=0):
    lib, L = _lib()
    M, C = inp.Y.shape
    keep, Yp, ld = rows_in(inp.Y, pad, offset)
    rm, rv = vec(inp.rm), vec(inp.rv)
    mean, invstd = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    sx = torch.empty(C, dtype=torch.float64, device="cuda")
    ws, n = workspace(L, M, C)
    lib.check(L.pn2_bn_train_stats_f32(Yp, M, C, ld, EPS, momentum, rm.data_ptr() if running else 0,
                                       rv.data_ptr() if running else 0, mean.data_ptr(), invstd.data_ptr(),
                                       sx.data_ptr(), ws.data_ptr(), n, _st(keep)), "pn2_bn_train_stats_f32")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (mean, invstd, sx, rm, rv)]


def check_stats(inp, got, momentum, running=True):
    mean, invstd, sx, rm, rv = got
    Y = tr.f64(inp.Y)
    M = Y.shape[0]
    ref = tr.stats(Y, EPS, momentum if running else 0.0, inp.rm, inp.rv)
    ymax = np.abs(Y).max(0)
    var_rel = 2 * U + TINY * (Y * Y).mean(0) / (ref.var + EPS)
    within("mean", mean, ref.mean, 2 * U * np.abs(ref.mean) + TINY * ymax)
    within("invstd", invstd, ref.invstd, var_rel * ref.invstd)
    want_sx = tr.sxhat(Y, mean, invstd)
    within("sxhat", sx, want_sx, 1e-6 * np.abs(want_sx) + TINY * M * ymax * tr.f64(invstd))
    if momentum > 0.0 and running:
        within("running_mean", rm, ref.running_mean, 2 * U * np.abs(ref.running_mean) + TINY * ymax)
        within("running_var", rv, ref.running_var, var_rel * np.abs(ref.running_var))
    else:  # momentum 0 (or no pointers): not a bit of the running statistics moves
        np.testing.assert_array_equal(rm.view(np.int32), inp.rm.view(np.int32))
        np.testing.assert_array_equal(rv.view(np.int32), inp.rv.view(np.int32))


STATS_CASES = sorted({(M, C, pad) for M, C, pad, _, _ in tr.DENSE_CASES}) + [(524034, 4, 0)]  # 2048 partials


@pytest.mark.parametrize("M,C,pad", STATS_CASES)
def test_stats(M, C, pad):
    inp = _inputs(M, C)
    check_stats(inp, run_stats(inp, pad, 0.1), 0.1)


@pytest.mark.parametrize("momentum,running", [(1.0, True), (0.0, True), (0.0, False)])
@pytest.mark.parametrize("M,C,pad", [(97, 65, 3), (4097, 68, 0)])
def test_stats_momentum_variants(M, C, pad, momentum, running):
    """momentum 1 (the first step of a cumulative average), and momentum 0 with and without
    running pointers: the running arrays stay as they were."""
    inp = _inputs(M, C)
    check_stats(inp, run_stats(inp, pad, momentum, running), momentum, running)


def test_stats_big_chunk():
    """C = 2048, M = 8197: 128-row chunks, the 65th of 5 rows."""
    M, C = tr.BIG_CASE[:2]
    inp = _inputs(M, C)
    check_stats(inp, run_stats(inp, 0, 0.1), 0.1)


def test_stats_unaligned_base():
    inp = _inputs(65, 64)
    check_stats(inp, run_stats(inp, 0, 0.1, offset=1), 0.1)


# ------------------------------------------------------------------ apply
def run_apply(inp, mean32, invstd32, pad, pad_a, relu, offset=0):
    lib, L = _lib()
    M, C = inp.Y.shape
    keep, Yp, ld = rows_in(inp.Y, pad, offset)
    A, Ap, lda = rows_out(M, C, pad_a)
    dev = [vec(a) for a in (mean32, invstd32, inp.gamma, inp.beta)]
    lib.check(L.pn2_bn_relu_apply_f32(Yp, M, C, ld, *[t.data_ptr() for t in dev], Ap, lda,
                                      0 if relu else NO_RELU, _st(keep)), "pn2_bn_relu_apply_f32")
    torch.cuda.synchronize()
    return take_rows(A, C, "A")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("M,C,pad,pad_a", sorted({c[:4] for c in tr.DENSE_CASES}))
def test_apply(M, C, pad, pad_a, relu):
    inp = _inputs(M, C)
    mean32, invstd32 = tr.rounded_stats(inp)
    got = run_apply(inp, mean32, invstd32, pad, pad_a, relu)
    ref = tr.apply(inp.Y, mean32, invstd32, inp.gamma, inp.beta, relu)
    within("A", got, ref.A, 8 * U * ref.mag)
    if relu:
        assert (got >= 0.0).all() and not np.signbit(got).any()
    sp = inp.special
    if "gamma_zero" in sp:  # gamma = 0: exactly (relu of) beta
        b = inp.beta[sp["gamma_zero"]]
        assert (got[:, sp["gamma_zero"]] == (max(b, np.float32(0)) if relu else b)).all()


def test_apply_unaligned_base():
    inp = _inputs(65, 64)
    mean32, invstd32 = tr.rounded_stats(inp)
    got = run_apply(inp, mean32, invstd32, 0, 0, True, offset=1)
    ref = tr.apply(inp.Y, mean32, invstd32, inp.gamma, inp.beta, True)
    within("A", got, ref.A, 8 * U * ref.mag)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("M,C,pad,pad_a", [(97, 65, 3, 4), (4097, 68, 0, 0), (65, 64, 4, 4), (2, 1, 0, 0)])
def test_forward_is_stats_then_apply(M, C, pad, pad_a, relu):
    """pn2_bn_train_forward_f32 = pn2_bn_train_stats_f32 then pn2_bn_relu_apply_f32, bit for bit."""
    lib, L = _lib()
    inp = _inputs(M, C)
    mean, invstd, sx, rm, rv = run_stats(inp, pad, 0.1)
    want_A = run_apply(inp, mean, invstd, pad, pad_a, relu)
    keep, Yp, ld = rows_in(inp.Y, pad)
    A, Ap, lda = rows_out(M, C, pad_a)
    rm2, rv2, ga, be = vec(inp.rm), vec(inp.rv), vec(inp.gamma), vec(inp.beta)
    st_mi = torch.empty(2 * C, device="cuda")
    sx2 = torch.empty(C, dtype=torch.float64, device="cuda")
    ws, n = workspace(L, M, C)
    lib.check(L.pn2_bn_train_forward_f32(Yp, M, C, ld, EPS, 0.1, rm2.data_ptr(), rv2.data_ptr(), ga.data_ptr(),
                                         be.data_ptr(), Ap, lda, 0 if relu else NO_RELU, st_mi.data_ptr(),
                                         sx2.data_ptr(), ws.data_ptr(), n, _st(keep)), "pn2_bn_train_forward_f32")
    torch.cuda.synchronize()
    for got, want, what in ((st_mi[:C], mean, "mean"), (st_mi[C:], invstd, "invstd"), (rm2, rm, "running_mean"),
                            (rv2, rv, "running_var")):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32), err_msg=what)
    np.testing.assert_array_equal(sx2.cpu().numpy().view(np.int64), sx.view(np.int64), err_msg="sxhat")
    np.testing.assert_array_equal(take_rows(A, C, "A").view(np.int32), want_A.view(np.int32), err_msg="A")


# ------------------------------------------------------------------ backward
def run_backward(inp, mean32, invstd32, d, sx, pads, relu, K=0, dbias=True, offset=0):
    """d: dA [M, C] (K == 0) or dOut [G, C] with inp.arg.  -> dY, dgamma, dbeta, dbias | None"""
    lib, L = _lib()
    M, C = inp.Y.shape
    pad, pad_d, pad_y = pads
    keep, Yp, ld = rows_in(inp.Y, pad, offset)
    keep_d, dp, ldd = rows_in(d, pad_d)
    dY, dYp, ldy = rows_out(M, C, pad_y)
    dev = [vec(a) for a in (mean32, invstd32, inp.gamma, inp.beta)]
    arg = vec(inp.arg, np.int32) if K else None
    sxd = vec(sx, np.float64) if dbias else None
    outs = [torch.full((C,), float(SENTINEL), device="cuda") for _ in range(3)]  # dgamma, dbeta, dbias
    ws, n = workspace(L, M, C)
    rc = L.pn2_bn_relu_backward_f32(Yp, M, C, ld, *[t.data_ptr() for t in dev],
                                    0 if K else dp, ldd, dp if K else 0, ldd, arg.data_ptr() if K else 0, K,
                                    sxd.data_ptr() if dbias else 0, dYp, ldy, outs[0].data_ptr(),
                                    outs[1].data_ptr(), outs[2].data_ptr() if dbias else 0, ws.data_ptr(), n,
                                    0 if relu else NO_RELU, _st(keep))
    lib.check(rc, "pn2_bn_relu_backward_f32")
    torch.cuda.synchronize()
    dgamma, dbeta, db = [t.cpu().numpy() for t in outs]
    if not dbias:  # a NULL dbias: nothing of ours written instead
        assert (db.view(np.int32) == SENTINEL.view(np.int32)).all()
    return take_rows(dY, C, "dY"), dgamma, dbeta, db if dbias else None


def check_backward(inp, pads, relu, K=0, dbias=True, offset=0):
    M, C = inp.Y.shape
    mean32, invstd32 = tr.rounded_stats(inp)
    sx = tr.sxhat(inp.Y, mean32, invstd32)
    d, share = tr.zero_ambiguous(inp, mean32, invstd32, relu)
    assert share <= 1e-4, "ReLU-ambiguous share %g" % share
    dY, dgamma, dbeta, db = run_backward(inp, mean32, invstd32, d, sx, pads, relu, K, dbias, offset)
    kw = dict(dOut=d, arg=inp.arg, K=K) if K else dict(dA=d)
    ref = tr.backward(inp.Y, mean32, invstd32, inp.gamma, inp.beta, sxhat=sx, relu=relu, **kw)
    gi = np.abs(tr.f64(inp.gamma) * tr.f64(invstd32))
    tol_dgamma = 4 * U * ref.sum_abs_dXn_xhat
    within("dbeta", dbeta, ref.dbeta, 2 * U * np.abs(ref.dbeta) + TINY * ref.sum_abs_dXn)
    within("dgamma", dgamma, ref.dgamma, tol_dgamma)
    within("dY", dY, ref.dY, 8 * U * gi * ref.dY_mag)
    if dbias:
        tol_dbias = 2 * U * np.abs(ref.dbias) + gi * np.abs(sx) / M * tol_dgamma
        within("dbias", db, ref.dbias, tol_dbias)
        if M >= 64:  # the value is definite: a zero or a flipped sign is far outside the bound
            assert (np.abs(ref.dbias) > 10 * tol_dbias).any()


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("M,C,pad,pad_d,pad_y", tr.DENSE_CASES)
def test_backward_dense(M, C, pad, pad_d, pad_y, relu):
    check_backward(_inputs(M, C), (pad, pad_d, pad_y), relu)


@pytest.mark.parametrize("M,C,pads", [(97, 64, (0, 0, 0)), (97, 65, (3, 4, 3))])
def test_backward_without_dbias(M, C, pads):
    check_backward(_inputs(M, C), pads, True, dbias=False)


def test_backward_unaligned_base():
    """C = 64 with Y one float past a 16-byte boundary: the scalar kernels, the same numbers."""
    check_backward(_inputs(65, 64), (0, 0, 0), True, offset=1)


def test_backward_big_chunk():
    M, C = tr.BIG_CASE[:2]
    check_backward(_inputs(M, C), (0, 0, 0), True)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("G,K,C,pad,pad_o,pad_y", tr.SCATTER_CASES)
def test_backward_scatter(G, K, C, pad, pad_o, pad_y, relu):
    check_backward(_inputs(G * K, C, G, K), (pad, pad_o, pad_y), relu, K=K)


@pytest.mark.parametrize("G,K,C,pad,pad_o,pad_y", tr.WORKSPACE_CASES)
def test_backward_scatter_fits_documented_workspace(G, K, C, pad, pad_o, pad_y):
    """A workspace of exactly pn2_bn_train_workspace_bytes(M, C) serves any K: with K = 3 the
    gather pass used to ask for 2730 partials of the 2048 and the entry refused the call."""
    check_backward(_inputs(G * K, C, G, K), (pad, pad_o, pad_y), True, K=K)


# ------------------------------------------------------------------ group max
def _max_input(G, K, C, seed):
    """Small integers (many exact ties), zeros of both signs, a -inf group, NaNs."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, (G, K, C)).astype(np.float32)
    a = np.where((a == 0) & (rng.random((G, K, C)) < 0.5), np.float32(-0.0), a)
    a[0, :, 0] = -np.inf
    a[G - 1, rng.integers(0, K, 3), C - 1] = np.nan
    if K > 1 and C > 1:
        a[0, :, 1] = np.where(rng.random(K) < 0.5, np.float32(-0.0), np.float32(0.0))  # only +-0
    return a.reshape(G * K, C)


def check_group_max(G, K, C, pad_a, pad_o):
    lib, L = _lib()
    a = _max_input(G, K, C, 1000 * G + 10 * K + C)
    keep, Ap, lda = rows_in(a, pad_a)
    out, op, ldo = rows_out(G, C, pad_o)
    arg = torch.full((G, C), -1, dtype=torch.int32, device="cuda")
    lib.check(L.pn2_group_max_f32(Ap, G, K, C, lda, op, ldo, arg.data_ptr(), _st(keep)), "pn2_group_max_f32")
    torch.cuda.synchronize()
    want, want_arg = tr.group_max(a, K)
    np.testing.assert_array_equal(arg.cpu().numpy(), want_arg)
    # bit for bit: the sign of a zero and a NaN are those of the first maximal row
    np.testing.assert_array_equal(take_rows(out, C, "max").view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("C", [1, 5, 64, 65])
@pytest.mark.parametrize("K", [1, 2, 8, 9, 10, 17, 255, 256, 257, 383, 384, 385])
def test_group_max(K, C):
    """Around the narrow kernel's 8-row unroll (which starts at row 1), the switch to the wide
    kernel at 256 and its 128-row rounds; G below, at and above the narrow kernel's 4 groups
    per block; strides above C."""
    for G in (1, 4, 5):
        pad_a, pad_o = [(0, 0), (3, 1), (4, 4)][(G + K + C) % 3]
        check_group_max(G, K, C, pad_a, pad_o)


def test_group_max_many_wide_groups():
    """G = 65536 groups of K = 256: past the wide kernel's grid, back on the narrow kernel."""
    check_group_max(65536, 256, 2, 0, 0)


@pytest.mark.parametrize("K,C", [(2, 1), (1, 5)])
def test_group_max_many_groups(K, C):
    """G = 262145 groups of a small K: one more block of groups than a grid's second dimension
    holds (4 groups per block x 65535), where the launch used to be refused.  Small integers
    (ties) throughout; group 0 and the last group hold a NaN, and where K allows it a tie:
    K = 2 gives them two NaNs (the first wins), and their neighbours a NaN after a number and
    two equal numbers."""
    lib, L = _lib()
    G = 262145
    rng = np.random.default_rng(7 * K + C)
    a = rng.integers(-3, 4, (G, K, C)).astype(np.float32)
    a[0, :, 0] = np.nan
    a[G - 1, :, C - 1] = np.nan
    if K > 1:
        a[1, :, 0] = [1.0, np.nan]
        a[G - 2, :, C - 1] = [3.0, 3.0]
    a = a.reshape(G * K, C)
    keep, Ap, lda = rows_in(a, 0)
    out, op, ldo = rows_out(G, C, 0)
    arg = torch.full((G, C), -1, dtype=torch.int32, device="cuda")
    lib.check(L.pn2_group_max_f32(Ap, G, K, C, lda, op, ldo, arg.data_ptr(), _st(keep)), "pn2_group_max_f32")
    torch.cuda.synchronize()
    want, want_arg = tr.group_max(a, K)
    assert want_arg[0, 0] == 0 and want_arg[G - 1, C - 1] == 0 and np.isnan(want[0, 0])
    np.testing.assert_array_equal(arg.cpu().numpy(), want_arg)
    np.testing.assert_array_equal(take_rows(out, C, "max").view(np.int32), want.view(np.int32))

"""tests/train_ref.py (the float64 restatement the GPU kernel tests compare with) against torch's
own float64 CPU autograd of BatchNorm1d(train) -> ReLU -> max over K, and the no-ReLU and no-max
variants; its dbias closed form against the direct sum of its dY; its transcription of the
host's chunking against the library's workspace size; and the ReLU-ambiguity cap of the inputs
tests/test_gpu_train_kernels.py uses, which needs the reference alone.  No device."""
import numpy as np
import pytest
import torch

import train_ref as tr


def close12(got, want, what):
    """1e-12 relative with a max-scaled floor: float64 sums in another order."""
    got, want = tr.f64(got), tr.f64(want)
    tol = 1e-12 * np.abs(want) + 1e-12 * max(float(np.abs(want).max()), 1e-300)
    err = np.abs(got - want)
    assert (err <= tol).all(), "%s: worst error/bound %.3g" % (what, float((err / tol).max()))


def _torch_step(inp, G, K, relu, momentum):
    """torch float64: -> out, arg (None without the max), dY, dgamma, dbeta, running stats."""
    C = inp.Y.shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=tr.EPS, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(inp.gamma).double())
        bn.bias.copy_(torch.from_numpy(inp.beta).double())
        bn.running_mean.copy_(torch.from_numpy(inp.rm).double())
        bn.running_var.copy_(torch.from_numpy(inp.rv).double())
    Y = torch.from_numpy(inp.Y).double().requires_grad_(True)
    A = bn(Y)
    if relu:
        A = torch.relu(A)
    arg = None
    if K:
        out, arg = torch.max(A.view(G, K, C), 1)
    else:
        out = A
    (out * torch.from_numpy(inp.d).double()).sum().backward()
    return (out.detach().numpy(), None if arg is None else arg.numpy(), Y.grad.numpy(),
            bn.weight.grad.numpy(), bn.bias.grad.numpy(), bn.running_mean.numpy(), bn.running_var.numpy())


@pytest.mark.parametrize("G,K,C,relu", [(13, 7, 9, True), (13, 7, 9, False), (1, 50, 6, True),
                                        (40, 0, 5, True), (40, 0, 5, False), (2, 1, 3, True),
                                        (300, 3, 1, True)])
def test_restatement_matches_torch_float64(G, K, C, relu):
    M = G * max(K, 1)
    inp = tr.make_inputs(M, C, 17 * M + C, G if K else 0, K)
    want_out, want_arg, want_dY, want_dg, want_db, want_rm, want_rv = _torch_step(inp, G, K, relu, 0.1)
    s = tr.stats(inp.Y, tr.EPS, 0.1, inp.rm, inp.rv)
    close12(s.running_mean, want_rm, "running_mean")
    close12(s.running_var, want_rv, "running_var")
    fw = tr.apply(inp.Y, s.mean, s.invstd, inp.gamma, inp.beta, relu)
    if K:
        out, arg = tr.group_max(fw.A, K)
        np.testing.assert_array_equal(arg, want_arg)
        close12(out, want_out, "max")
        bw = tr.backward(inp.Y, s.mean, s.invstd, inp.gamma, inp.beta, dOut=inp.d, arg=arg, K=K, relu=relu)
    else:
        close12(fw.A, want_out, "A")
        bw = tr.backward(inp.Y, s.mean, s.invstd, inp.gamma, inp.beta, dA=inp.d, relu=relu)
    close12(bw.dbeta, want_db, "dbeta")
    close12(bw.dgamma, want_dg, "dgamma")
    close12(bw.dY, want_dY, "dY")


def test_unbiased_variance_needs_two_rows():
    """M == 1: the biased variance (0) enters running_var, as the kernel documents."""
    inp = tr.make_inputs(1, 3, 5)
    s = tr.stats(inp.Y, tr.EPS, 0.25, inp.rm, inp.rv)
    np.testing.assert_array_equal(s.var, 0.0)
    close12(s.running_var, 0.75 * tr.f64(inp.rv), "running_var")
    close12(s.running_mean, 0.75 * tr.f64(inp.rm) + 0.25 * tr.f64(inp.Y[0]), "running_mean")
    s0 = tr.stats(inp.Y, tr.EPS, 0.0, inp.rm, inp.rv)
    assert s0.running_mean is inp.rm and s0.running_var is inp.rv  # momentum 0: untouched


def test_group_max_first_index_nan_and_signed_zero():
    a = np.array([[1, -0.0, np.nan, -np.inf], [3, 0.0, 1, -np.inf], [3, -0.0, np.nan, -np.inf]], np.float32)
    out, arg = tr.group_max(a, 3)
    np.testing.assert_array_equal(arg, [[1, 0, 0, 0]])
    np.testing.assert_array_equal(out.view(np.int32), a[[1, 0, 0, 0], [0, 1, 2, 3]][None].view(np.int32))
    t_out, t_arg = torch.max(torch.from_numpy(a).view(1, 3, 4), 1)
    np.testing.assert_array_equal(arg, t_arg.numpy())
    np.testing.assert_array_equal(out, t_out.numpy())


@pytest.mark.parametrize("G,K,C,relu", [(13, 7, 9, True), (500, 0, 6, True), (500, 0, 6, False),
                                        (64, 3, 5, True)])
def test_dbias_closed_form_is_the_sum_of_dY(G, K, C, relu):
    """With the float32-rounded statistics the kernels use, sum_r xhat is not 0 and the conv bias
    gradient is a definite number: -gamma*invstd*(S2/M)*sxhat must be the direct sum over rows of
    the reference's dY, to that sum's cancellation noise (float64 pairwise sums: a few 2^-53 of
    the summed magnitudes, here 1e-13 of them, for dY and for the two terms of sxhat)."""
    M = G * max(K, 1)
    inp = tr.make_inputs(M, C, 3 * M + C, G if K else 0, K)
    mean32, invstd32 = tr.rounded_stats(inp)
    sx = tr.sxhat(inp.Y, mean32, invstd32)
    kw = dict(dOut=inp.d, arg=inp.arg, K=K) if K else dict(dA=inp.d)
    bw = tr.backward(inp.Y, mean32, invstd32, inp.gamma, inp.beta, sxhat=sx, relu=relu, **kw)
    direct = bw.dY.sum(0)
    fac = np.abs(tr.f64(inp.gamma) * tr.f64(invstd32) * bw.dgamma / M)
    sx_noise = (np.abs(tr.f64(inp.Y)).sum(0) + M * np.abs(tr.f64(mean32))) * tr.f64(invstd32)
    tol = 1e-13 * (np.abs(bw.dY).sum(0) + fac * sx_noise)
    assert (np.abs(bw.dbias - direct) <= tol).all(), (bw.dbias, direct, tol)
    live = [c for k, c in inp.special.items() if k == "mean30"]
    assert np.abs(bw.dbias[live]).min() > 0.0  # a definite value, not an analytic zero


def test_chunking_transcription_matches_the_library():
    """train_ref.chunks is the host's chunks(M, C): the library's workspace size is
    chunks*2*C + 3*C doubles.  (The library loads without a device.)"""
    from pn2 import _lib
    L = _lib.load()
    shapes = [(M, C) for M in (1, 2, 64, 65, 4097, 8197, 8327, 131072, 524034, 524035, 698712, 4000000)
              for C in (1, 4, 64, 65, 130, 2048)]
    for M, C in shapes:
        assert L.pn2_bn_train_workspace_bytes(M, C) == (tr.chunks(M, C) * 2 * C + 3 * C) * 8, (M, C)
    # the shapes the GPU tests rely on
    assert (tr.chunks(4097, 64), tr.chunks(4097, 68), tr.chunks(8327, 130)) == (65, 65, 131)
    assert (tr.chunk_rows(8197, 2048), tr.chunks(8197, 2048)) == (128, 65)
    # what the gather pass of the backward asked for before it was fitted to the workspace
    G, K, C = tr.WORKSPACE_CASES[0][:3]
    assert (G + tr.chunk_rows(G, C) - 1) // tr.chunk_rows(G, C) == 2730 and tr.chunks(G * K, C) == 2048


def _backward_cases():
    for M, C, *_ in tr.DENSE_CASES + [tr.BIG_CASE]:
        yield M, C, 0, 0
    for G, K, C, *_ in tr.SCATTER_CASES + tr.WORKSPACE_CASES:
        yield G * K, C, G, K


@pytest.mark.parametrize("M,C,G,K", sorted(set(_backward_cases())))
def test_gpu_inputs_meet_the_ambiguity_cap(M, C, G, K):
    """At most 1e-4 of a case's elements may have their gradient zeroed for a ReLU mask that
    float32 could decide either way (the constant and gamma = 0 columns aside)."""
    inp = tr.make_inputs(M, C, tr.case_seed(M, C, K), G, K)
    mean32, invstd32 = tr.rounded_stats(inp)
    d, share = tr.zero_ambiguous(inp, mean32, invstd32, True)
    assert share <= 1e-4, share
    assert d.shape == inp.d.shape

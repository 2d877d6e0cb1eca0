"""tests/optim_ref.py -- the numpy float32 restatement of the optimizer kernels' rule -- against
a float64 Adam and SGD written here, with torch's own CPU single-tensor float32 optimizers as the
yardstick: over 5 steps the restatement's largest error against float64 is at most twice torch's
largest error against float64 on the same inputs, per state tensor.  (Bit equality with torch is
not asked: ATen's vectorised lerp and addcmul contract differently on CPU and GPU.)"""
import numpy as np
import pytest
import torch

import optim_ref

STEPS = 5
WD = 1e-4
SIZES = (7, 1000, 4099)
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    # gradient magnitudes log-uniform over [1e-4, 10], random signs, new ones every step
    gs = [(np.exp(rng.uniform(np.log(1e-4), np.log(10.0), n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
          for _ in range(STEPS)]
    return p, gs


def adam64(p, gs, lr, betas, eps, wd):
    p = p.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    b1, b2 = betas
    for t, g in enumerate(gs, 1):
        g = g.astype(np.float64)
        if wd != 0:
            g = g + wd * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        mhat = m / (1 - b1 ** t)
        vhat = v / (1 - b2 ** t)
        p = p - lr * mhat / (np.sqrt(vhat) + eps)
    return p, m, v


def sgd64(p, gs, lr, mu, damp, wd):
    p = p.astype(np.float64)
    buf = None
    for g in gs:
        g = g.astype(np.float64)
        if wd != 0:
            g = g + wd * p
        if mu != 0:
            buf = g.copy() if buf is None else mu * buf + (1 - damp) * g
            g = buf
        p = p - lr * g
    return p, buf


def _err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


def _check(name, ours, theirs, want):
    eo, et = _err(ours, want), _err(theirs, want)
    print("%s: restatement %.3e torch %.3e (max |x| %.3e)" % (name, eo, et, float(np.abs(want).max())))
    assert eo <= 2 * et, (name, eo, et)


@pytest.mark.parametrize("n", SIZES)
def test_adam_restatement_error_within_twice_torchs(n):
    p0, gs = _inputs(n, 100 + n)
    want = adam64(p0, gs, LR, BETAS, EPS, WD)

    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, g in enumerate(gs, 1):
        optim_ref.adam_step(p, g, m, v, optim_ref.adam_scalars(LR, BETAS, EPS, WD, t))

    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    for g in gs:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    st = opt.state[tp]
    _check("p", p, tp.detach().numpy(), want[0])
    _check("exp_avg", m, st["exp_avg"].numpy(), want[1])
    _check("exp_avg_sq", v, st["exp_avg_sq"].numpy(), want[2])
    # the stated rule and ATen's kernels agree in all but a small share of the elements
    for name, a, b in (("p", p, tp.detach().numpy()), ("exp_avg", m, st["exp_avg"].numpy()),
                       ("exp_avg_sq", v, st["exp_avg_sq"].numpy())):
        print("%s: %d of %d values differ from torch" % (name, int((a != b).sum()), n))


@pytest.mark.parametrize("mu", (0.0, 0.9))
@pytest.mark.parametrize("n", SIZES)
def test_sgd_restatement_error_within_twice_torchs(n, mu):
    lr = 0.01
    p0, gs = _inputs(n, 200 + n)
    want = sgd64(p0, gs, lr, mu, 0.0, WD)

    p = p0.copy()
    buf = np.zeros(n, np.float32) if mu != 0 else None
    for t, g in enumerate(gs):
        optim_ref.sgd_step(p, g, buf, optim_ref.sgd_scalars(lr, mu, 0.0, WD, first=(t == 0)))

    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, weight_decay=WD, foreach=False)
    for g in gs:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    _check("p", p, tp.detach().numpy(), want[0])
    if mu != 0:
        _check("momentum_buffer", buf, opt.state[tp]["momentum_buffer"].numpy(), want[1])


def test_scalars_are_torchs_expressions_rounded_once():
    s = optim_ref.adam_scalars(1e-3, (0.9, 0.999), 1e-8, 1e-4, 3)
    assert s["ss"] == np.float32(-(1e-3 / (1 - 0.9 ** 3.0)))
    assert s["bc2_sqrt"] == np.float32((1 - 0.999 ** 3.0) ** 0.5)
    assert s["omb1"] == np.float32(1 - 0.9) and s["omb2"] == np.float32(1 - 0.999)
    assert all(v.dtype == np.float32 for v in s.values())

"""numpy float32 restatement of the optimizer kernels' arithmetic rule (include/pn2.h, the
optimizer block): every line is one numpy float32 operation, so each rounds once, in the rule's
order.  The host's scalar expressions (pn2/optim.py) are restated too.  Arrays are updated in
place; they must be float32."""
import numpy as np

F = np.float32


def adam_scalars(lr, betas, eps, weight_decay, step):
    """The Adam scalar block for the step-th update (step counts from 1): Python floats, rounded
    to float32 once."""
    beta1, beta2 = betas
    bias_correction1 = 1 - beta1 ** float(step)
    bias_correction2 = 1 - beta2 ** float(step)
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return dict(ss=F(-step_size), bc2_sqrt=F(bias_correction2_sqrt), omb1=F(1 - beta1), beta2=F(beta2),
                omb2=F(1 - beta2), eps=F(eps), wd=F(weight_decay))


def adam_step(p, g, m, v, s):
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    if s["wd"] != 0:
        t = s["wd"] * p
        g = g + t
    d = g - m
    d = s["omb1"] * d
    m[...] = m + d
    v[...] = v * s["beta2"]
    t = s["omb2"] * g
    t = t * g
    v[...] = v + t
    den = np.sqrt(v)
    den = den / s["bc2_sqrt"]
    den = den + s["eps"]
    q = m / den
    q = s["ss"] * q
    p[...] = p + q
    assert all(a.dtype == np.float32 for a in (p, m, v, den, q))


def sgd_scalars(lr, momentum, dampening, weight_decay, first):
    return dict(lr=F(lr), mu=F(momentum), omd=F(1 - dampening), wd=F(weight_decay), first=bool(first))


def sgd_step(p, g, buf, s):
    """buf: the momentum buffer, or None for a tensor without one (momentum == 0)."""
    assert p.dtype == np.float32 and g.dtype == np.float32
    if s["wd"] != 0:
        t = s["wd"] * p
        g = g + t
    if buf is not None:
        if s["first"]:
            buf[...] = g
        else:
            a = buf * s["mu"]
            b = s["omd"] * g
            buf[...] = a + b
        g = buf
    t = s["lr"] * g
    p[...] = p - t
    assert p.dtype == np.float32 and t.dtype == np.float32

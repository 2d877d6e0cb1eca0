"""pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32 (csrc/fc_train.hip; contracts and order rules
in include/pn2.h), their ops, train.linear_bn_train and the train_head route of the heads.

The kernels are checked against a float64 numpy formulation on host copies.  Y takes
test_gpu_train_gemm's float32-sum bound 2 (n+3) 2^-24 sum|a||b| (derived there); A, stats and
the running statistics take close(..., 1e-4), the gradients close(..., 1e-3): the project's two
training tolerances.  Where the float64 pre-activation is within 1e-4 of the ReLU's kink the
upstream gradient is zeroed (a float32 forward may land on the other side; the rule of
test_gpu_train_gemm._clear_pairs): no tolerance is loosened.  B = 2 takes eps = 0.25: with two
rows and eps -> 0 the batch-statistics dY is analytically zero and there is nothing to compare."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from test_gpu_train_gemm import Mat, bits, want_and_bound
from test_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_RELU, FROZEN = 1, 2
MOM = 0.1


def _lib():
    from pn2 import _lib as lib
    return lib, lib.load()


def max_rows():
    return int(_lib()[1].pn2_fc_train_max_rows())


SHAPES = [(2, 1, 1), (3, 6, 3), (24, 13, 131), (33, 70, 64), (64, 70, 259), ("max", 17, 40)]
MODES = ["contig", "ld", "offset"]
BNS = ["batch", "frozen", "none"]


def make_inputs(B, N, K, seed, ties=False):
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s, dtype=np.float32)
    d = dict(X=f(B, K), W=f(N, K) / np.float32(np.sqrt(K)), bias=f(N) * np.float32(0.3),
             gamma=(g.random(N, dtype=np.float32) + np.float32(0.5)), beta=f(N) * np.float32(0.3),
             rm=f(N) * np.float32(0.1), rv=g.random(N, dtype=np.float32) + np.float32(0.5), dA=f(B, N),
             eps=0.25 if B == 2 else 1e-5)
    if ties:
        # column 0: every pre-activation negative in every variant (Y = -3 in all rows)
        d["W"][0] = 0
        d["bias"][0], d["beta"][0], d["gamma"][0], d["rm"][0], d["rv"][0] = -3, -1, 1, 0, 1
        d["X"][1] = d["X"][0]  # a row that repeats another
    return d


def reference(d, bn, relu):
    """The float64 formulation -> dict of everything the two entries write."""
    X, W = d["X"].astype(np.float64), d["W"].astype(np.float64)
    B = X.shape[0]
    Y = X @ W.T + d["bias"].astype(np.float64)
    out = {"Y": Y}
    ga, be = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    if bn == "batch":
        mean, var = Y.mean(0), Y.var(0)
        out["rm"] = (1 - MOM) * d["rm"] + MOM * mean
        out["rv"] = (1 - MOM) * d["rv"] + MOM * var * B / (B - 1)
    elif bn == "frozen":
        mean, var = d["rm"].astype(np.float64), d["rv"].astype(np.float64)
    if bn == "none":
        pre = Y
    else:
        invstd = 1.0 / np.sqrt(var + d["eps"])
        xhat = (Y - mean) * invstd
        pre = xhat * ga + be
        out["mean"], out["invstd"] = mean, invstd
    out["A"] = np.maximum(pre, 0) if relu else pre
    dA = d["dA"].astype(np.float64)
    if relu:
        dA = dA * (np.abs(pre) > 1e-4)  # nothing rides on the side of the kink
    out["dA"] = dA.astype(np.float32)
    dXn = dA * (pre > 0) if relu else dA
    if bn == "none":
        dY = dXn
    else:
        out["dbeta"], out["dgamma"] = dXn.sum(0), (dXn * xhat).sum(0)
        dY = ga * invstd * dXn
        if bn == "batch":
            dY = ga * invstd * (dXn - out["dbeta"] / B - xhat * out["dgamma"] / B)
    out["dY"], out["dbias"], out["dW"] = dY, dY.sum(0), dY.T @ X
    return out


def dvec(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


OUT = ("Y", "A", "stats", "rm", "rv", "dY", "dW", "dbias", "dgamma", "dbeta")


def run_entries(d, bn, relu, mode, momentum=MOM, rows=False):
    """The forward and the backward C entry (rows: the any-B pair) on Mat operands, the upstream
    gradient d["dA"] -> dict of host results.  Mat.result() checks the guard bands around every
    matrix, the vectors carry a guard element behind their edge, the inputs must keep their bits
    and every output element must have been written."""
    lib, L = _lib()
    fwd = L.pn2_fc_bn_forward_rows_f32 if rows else L.pn2_fc_bn_forward_f32
    bwd = L.pn2_fc_bn_backward_rows_f32 if rows else L.pn2_fc_bn_backward_f32
    B, K = d["X"].shape
    N = d["W"].shape[0]
    flags = (0 if relu else NO_RELU) | (FROZEN if bn == "frozen" else 0)
    x, w, dA = Mat(B, K, mode, d["X"]), Mat(N, K, mode, d["W"]), Mat(B, N, mode, d["dA"])
    y, a, dy, dw = Mat(B, N, mode), Mat(B, N, mode), Mat(B, N, mode), Mat(N, K, mode)
    bias, gamma, beta, rm, rv = (dvec(d[k]) for k in ("bias", "gamma", "beta", "rm", "rv"))
    stats, dbias, dgamma, dbeta = (torch.full((n + 1,), float("nan"), device=DEV) for n in (2 * N, N, N, N))
    has = bn != "none"
    p = lambda t: t.data_ptr() if has else 0
    st = lib.stream_ptr(x.buf.device)
    lib.check(fwd(x.ptr, x.ld, w.ptr, w.ld, bias.data_ptr(), B, N, K, d["eps"], momentum, p(rm), p(rv), p(gamma),
                  p(beta), y.ptr, y.ld, a.ptr, a.ld, p(stats), flags, st), "forward")
    out = {"Y": y.result(), "A": a.result(), "rm": rm.cpu().numpy(), "rv": rv.cpu().numpy()}
    lib.check(bwd(dA.ptr, dA.ld, y.ptr, y.ld, x.ptr, x.ld, p(stats), p(gamma), p(beta), B, N, K, dy.ptr, dy.ld,
                  dw.ptr, dw.ld, dbias.data_ptr(), p(dgamma), p(dbeta), flags, st), "backward")
    out.update(dY=dy.result(), dW=dw.result())
    for k, t in (("stats", stats), ("dbias", dbias), ("dgamma", dgamma), ("dbeta", dbeta)):
        h = t.cpu().numpy()
        assert np.isnan(h[-1]), "%s: a write behind its edge" % k
        out[k] = h[:-1]
    # the inputs keep their bits (Y is the backward's input)
    for m, k in ((x, "X"), (w, "W"), (dA, "dA")):
        assert np.array_equal(bits(m.result()), bits(d[k])), k
    assert np.array_equal(bits(y.result()), bits(out["Y"])), "Y"
    for t, k in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        assert np.array_equal(bits(t.cpu().numpy()), bits(d[k])), k
    for k in ("Y", "A", "dY", "dW", "dbias"):
        assert not np.isnan(out[k]).any(), "%s: an element was not written" % k
    if has:
        for k in ("stats", "dgamma", "dbeta"):
            assert not np.isnan(out[k]).any(), "%s: an element was not written" % k
    else:
        assert all(np.isnan(out[k]).all() for k in ("stats", "dgamma", "dbeta")), "touched without BN"
    return out


def check_case(B, N, K, bn, relu, mode, seed, ties=False, momentum=MOM):
    d = make_inputs(B, N, K, seed, ties)
    want = reference(d, bn, relu)
    d["dA"] = want["dA"]
    got = run_entries(d, bn, relu, mode, momentum)
    _, bound = want_and_bound("nt", d["X"], d["W"], d["bias"])
    err = np.abs(got["Y"].astype(np.float64) - want["Y"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("B=%d N=%d K=%d %s relu=%d %s: Y worst error / bound = %.3f" % (B, N, K, bn, relu, mode, worst))
    assert (err <= bound).all(), "Y worst error / bound = %.3f" % worst
    close(got["A"], want["A"], 1e-4, "A")
    if bn != "none":
        close(got["stats"][:N], want["mean"], 1e-4, "mean")
        close(got["stats"][N:], want["invstd"], 1e-4, "invstd")
        close(got["dgamma"], want["dgamma"], 1e-3, "dgamma")
        close(got["dbeta"], want["dbeta"], 1e-3, "dbeta")
    if bn == "batch" and momentum > 0:
        close(got["rm"], want["rm"], 1e-4, "running_mean")
        close(got["rv"], want["rv"], 1e-4, "running_var")
    else:  # frozen, no BN, momentum 0: the running statistics keep their bits
        assert np.array_equal(bits(got["rm"]), bits(d["rm"])) and np.array_equal(bits(got["rv"]), bits(d["rv"]))
    close(got["dY"], want["dY"], 1e-3, "dY")
    close(got["dW"], want["dW"], 1e-3, "dW")
    if bn == "batch":  # analytically zero: float noise on both sides
        assert float(np.abs(got["dbias"]).max()) <= 1e-4 * float(np.abs(got["dW"]).max()), "dbias"
    else:
        close(got["dbias"], want["dbias"], 1e-3, "dbias")
    return d, got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("bn", BNS)
@pytest.mark.parametrize("B,N,K", SHAPES)
def test_kernels_against_float64(B, N, K, bn, relu, mode):
    B = max_rows() if B == "max" else B
    check_case(B, N, K, bn, relu, mode, seed=B * 7 + N * 3 + K)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("bn", BNS)
def test_real_shape(bn, relu):
    check_case(24, 512, 1024, bn, relu, "contig", seed=9)


@pytest.mark.parametrize("bn", BNS)
def test_momentum_zero_keeps_running_statistics(bn):
    check_case(24, 13, 131, bn, 1, "ld", seed=12, momentum=0.0)


@pytest.mark.parametrize("bn", BNS)
@pytest.mark.parametrize("B,N,K", [(24, 13, 131), (33, 70, 64)])
def test_relu_ties(B, N, K, bn):
    """A column whose pre-activations are all negative (a zero column of A, of dY and a zero row
    of dW), and a row that repeats another."""
    d, got = check_case(B, N, K, bn, 1, "offset", seed=31, ties=True)
    assert not got["A"][:, 0].any() and not got["dY"][:, 0].any() and not got["dW"][0].any()
    assert np.array_equal(bits(got["Y"][0]), bits(got["Y"][1]))
    assert np.array_equal(bits(got["A"][0]), bits(got["A"][1]))


# ------------------------------------------------------------------------------ row independence
def test_row_independence_of_y():
    from pn2 import ops
    d = make_inputs(37, 70, 131, seed=21)
    X, W, b = dvec(d["X"]), dvec(d["W"]), dvec(d["bias"])
    fwd = lambda x: ops.fc_bn_forward_direct(x, W, b, None, None, None, None, 0.0, 0.0, False, False)[0]
    full = fwd(X).cpu().numpy()
    sel = np.random.default_rng(3).permutation(37)[:11]
    part = fwd(X[torch.from_numpy(sel).to(DEV)].contiguous()).cpu().numpy()
    assert np.array_equal(bits(part), bits(full[sel]))
    one = fwd(X[29:30]).cpu().numpy()
    assert one.shape == (1, 70) and np.array_equal(bits(one), bits(full[29:30]))
    # batch statistics change A, never Y
    g, be, rm, rv = (dvec(d[k]) for k in ("gamma", "beta", "rm", "rv"))
    Yb = ops.fc_bn_forward_direct(X, W, b, g, be, rm, rv, 1e-5, 0.1, True, False)[0].cpu().numpy()
    assert np.array_equal(bits(Yb), bits(full))


# ------------------------------------------------------------------------------ order observable
def test_dbeta_is_the_ascending_float64_sum():
    d = make_inputs(37, 70, 131, seed=5)
    d["dA"] = reference(d, "batch", 1)["dA"]
    got = run_entries(d, "batch", 1, "contig")
    N = 70
    mu, is_ = got["stats"][:N], got["stats"][N:]
    pre = ((got["Y"] - mu) * is_) * d["gamma"] + d["beta"]  # float32, each operation rounded
    assert pre.dtype == np.float32
    dXn = np.where(pre > 0, d["dA"], np.float32(0))
    s64 = np.zeros(N, np.float64)
    s32 = np.zeros(N, np.float32)
    for r in range(37):
        s64 += dXn[r].astype(np.float64)
        s32 = (s32 + dXn[r]).astype(np.float32)
    assert np.array_equal(bits(got["dbeta"]), bits(s64.astype(np.float32)))
    assert not np.array_equal(bits(s32), bits(s64.astype(np.float32))), "the order is not observable"


@pytest.mark.parametrize("bn", BNS)
def test_same_bits_twice(bn):
    d = make_inputs(33, 70, 259, seed=41)
    d["dA"] = reference(d, bn, 1)["dA"]
    a = run_entries(d, bn, 1, "ld")
    b = run_entries(d, bn, 1, "ld")
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


# ------------------------------------------------------------------------------ routes
class _Tail(torch.nn.Module):
    """Runs a module's FC tail and records the gradient of the first hidden activation (the
    input of the first dropout call)."""

    def __init__(self, mod, run):
        super().__init__()
        self.mod, self.run, self.hidden_grad = mod, run, None

    def forward(self, x):
        seen = []

        def hook(_, inp):
            if not seen and inp[0].requires_grad:
                seen.append(1)
                inp[0].register_hook(lambda g: setattr(self, "hidden_grad", g.detach().clone()))
        drops = [m for m in self.mod.modules() if isinstance(m, torch.nn.Dropout)]
        hs = [m.register_forward_pre_hook(hook) for m in drops]
        try:
            return self.run(self.mod, x)
        finally:
            for h in hs:
                h.remove()


def _route(mod0, run, x0, R, key, train):
    from pn2 import tuning
    mod = copy.deepcopy(mod0).train(train)
    tail = _Tail(mod, run)
    x = x0.clone().requires_grad_(True)
    with tuning.override(train_head=key):
        torch.manual_seed(77)  # the dropout masks
        out = tail(x)
        (out * R).sum().backward()
    return out.detach(), x.grad, mod, tail.hidden_grad


def _routes_agree(mod0, run, x0, R, train, fc_bias_names):
    o0, g0, m0, h0 = _route(mod0, run, x0, R, 0, train)
    o1, g1, m1, h1 = _route(mod0, run, x0, R, 1, train)
    close(o1.cpu(), o0.cpu(), 1e-4, "out")
    close(g1.cpu(), g0.cpu(), 1e-3, "input grad")
    p0 = dict(m0.named_parameters())
    for k, p in m1.named_parameters():
        if p0[k].grad is None:
            assert p.grad is None, k
            continue
        if train and k in fc_bias_names:  # analytically zero (a bias before a batch-statistics BN)
            wmax = float(dict(m1.named_parameters())[k[:-4] + "weight"].grad.abs().max())
            assert float(p.grad.abs().max()) <= 1e-4 * wmax, k
            continue
        close(p.grad.cpu(), p0[k].grad.cpu(), 1e-3, "grad " + k)
    b0 = dict(m0.named_buffers())
    for k, b in m1.named_buffers():
        close(b.float().cpu(), b0[k].float().cpu(), 1e-4, k)
    if h0 is not None or h1 is not None:  # the masks were equal
        assert torch.equal(h0 == 0, h1 == 0)
        if train:
            assert (h0 == 0).any() and (h0 != 0).any()


@pytest.mark.parametrize("train", [True, False])
def test_fc_head_routes_agree(train):
    from pn2 import heads
    mod = cases.build_head(heads.RotationSSG, 90).to(DEV)
    g = torch.Generator().manual_seed(91)
    x0 = torch.randn(5, 1024, generator=g).to(DEV)
    R = torch.randn(5, 3, generator=g).to(DEV)
    _routes_agree(mod, lambda m, x: m._fc(x), x0, R, train, ("fc1.bias", "fc2.bias"))


@pytest.mark.parametrize("train", [True, False])
def test_mean_mlp_routes_agree(train):
    from pn2 import heads
    mod = cases.build_head(heads.TranslationSSG, 92).to(DEV)
    g = torch.Generator().manual_seed(93)
    x0 = torch.randn(5, 3, generator=g).to(DEV)
    R = torch.randn(5, 3, generator=g).to(DEV)
    _routes_agree(mod, lambda m, x: m._mean_mlp(x), x0, R, train, ("mean_fc1.bias",))


@pytest.mark.parametrize("train", [True, False])
def test_tnet_routes_agree(train):
    from pn2 import pointnet_utils as PU
    torch.manual_seed(94)
    mod = PU.TNet3d(channel=3)
    cases.randomize_bn(mod, 95)
    mod = mod.to(DEV)
    g = torch.Generator().manual_seed(96)
    x0 = torch.randn(4, 3, 50, generator=g).to(DEV)
    R = torch.randn(4, 3, 3, generator=g).to(DEV)
    # bn3.bias: the rows of fc1's input gradient sum to zero (bn4's batch statistics), and every
    # pooled relu(bn3) channel is active, so its gradient is analytically zero as well
    _routes_agree(mod, lambda m, x: m(x), x0, R, train,
                  ("fc1.bias", "fc2.bias", "conv1.bias", "conv2.bias", "conv3.bias", "bn3.bias"))


@pytest.mark.parametrize("train", [True, False])
def test_v1_tail_routes_agree(train):
    from pn2 import heads_v1
    mod = cases.build_head(heads_v1.SignV1, 97).to(DEV)
    g = torch.Generator().manual_seed(98)
    x0 = torch.randn(5, 1024, generator=g).to(DEV)
    R = torch.randn(5, 1, generator=g).to(DEV)
    _routes_agree(mod, lambda m, x: m._tail(x), x0, R, train, ("fc.0.bias", "fc.1.bias"))


# ------------------------------------------------------------------------------ route taken
def _cls_tail(B, train=True):
    from pn2 import heads
    mod = cases.build_head(heads.ClsSSG, 60).to(DEV).train(train)
    x = torch.randn(B, 1024, generator=torch.Generator().manual_seed(61)).to(DEV).requires_grad_(True)
    return mod, x


def test_route_records_the_kernels():
    from pn2 import ops, tuning
    mod, x = _cls_tail(6)
    assert tuning.get("train_head") == 0
    with ops.kernel_timer() as t:
        mod._fc(x).sum().backward()
    assert not [r[0] for r in t.records if r[0].startswith("pn2_fc_bn")]
    with tuning.override(train_head=1), ops.kernel_timer() as t:
        mod._fc(x).sum().backward()
    names = [r[0] for r in t.records]
    assert names.count("pn2_fc_bn_forward_f32") == 3 and names.count("pn2_fc_bn_backward_f32") == 3
    assert names.count("pn2_gemm_nn_f32") == 3  # x needs a gradient
    with tuning.override(train_head=1), ops.kernel_timer() as t:
        mod._fc(x.detach()).sum().backward()
    assert [r[0] for r in t.records].count("pn2_gemm_nn_f32") == 2


def test_above_max_rows_falls_back():
    from pn2 import ops, tuning
    B = max_rows() + 1
    res = []
    for key in (0, 1):
        mod, x = _cls_tail(B)
        with tuning.override(train_head=key), ops.kernel_timer() as t:
            torch.manual_seed(3)
            out = mod._fc(x)
            out.sum().backward()
        assert not [r[0] for r in t.records if r[0].startswith("pn2_fc_bn")]
        res.append((out.detach(), x.grad, mod))
    (o0, g0, m0), (o1, g1, m1) = res
    close(o1.cpu(), o0.cpu(), 1e-4, "out")
    close(g1.cpu(), g0.cpu(), 1e-3, "input grad")
    for (k, p), (_, q) in zip(m1.named_buffers(), m0.named_buffers()):
        close(p.float().cpu(), q.float().cpu(), 1e-4, k)


def test_single_row_in_train_mode_raises_as_the_modules():
    from pn2 import tuning
    for key in (0, 1):
        mod, x = _cls_tail(1)
        with tuning.override(train_head=key), pytest.raises(ValueError, match="more than 1 value per channel"):
            mod._fc(x)
    # a single row with frozen statistics is served by the kernels
    mod, x = _cls_tail(1, train=False)
    ref = mod._fc(x).detach()
    with tuning.override(train_head=1):
        close(mod._fc(x).detach().cpu(), ref.cpu(), 1e-4, "eval row")


# ------------------------------------------------------------------------------ reproducible step
def _two_model_steps(mod, forward_loss):
    """Two train steps (forward, loss, backward, Adam.step) from one saved state under the three
    reproducibility keys -> two dicts of host arrays."""
    from pn2 import tuning
    state = copy.deepcopy(mod.state_dict())
    out = []
    for _ in range(2):
        mod.load_state_dict(state)
        mod.zero_grad(set_to_none=True)
        opt = torch.optim.Adam(mod.parameters(), lr=1e-3)
        with tuning.override(train_gemm=1, group_backward=1, train_head=1):
            torch.manual_seed(5)  # the FPS start draws and the dropout masks
            loss = forward_loss(mod)
            loss.backward()
        step = {"loss": loss.detach().clone()}
        step.update({"grad " + k: p.grad.clone() for k, p in mod.named_parameters()})
        opt.step()
        step.update({"param " + k: p.detach().clone() for k, p in mod.named_parameters()})
        step.update({"buf " + k: b.detach().clone() for k, b in mod.named_buffers()})
        out.append({k: v.cpu().numpy() for k, v in step.items()})
    return out


@pytest.mark.parametrize("which", ["cls_ssg", "translation_ssg"])
def test_reproducible_whole_model_step(which):
    """Every gradient, buffer and parameter after the optimizer step bit-identical between two
    runs of the same step: the SA layers, the FC tail (and the mean MLP) on this project's
    kernels; dropout, the loss and Adam are torch (elementwise, or one reduction per tensor)."""
    from pn2 import heads, ops
    B, N = 3, 512
    g = torch.Generator().manual_seed(80)
    if which == "cls_ssg":
        mod = cases.build_head(heads.ClsSSG, 81).to(DEV).train()
        pts = cases.cloud("uniform3", B, N, 82).permute(0, 2, 1).contiguous().to(DEV)
        target = torch.tensor([1, 4, 6], device=DEV)
        fl = lambda m: F.nll_loss(m(pts)[0], target)
    else:
        mod = cases.build_head(heads.TranslationSSG, 83).to(DEV).train()
        pts = cases.cloud("onehot10", B, N, 84).permute(0, 2, 1).contiguous().to(DEV)
        mean = torch.randn(B, 3, generator=g).to(DEV)
        target = torch.randn(B, 3, generator=g).to(DEV)
        fl = lambda m: F.mse_loss(m(pts, mean), target)
    with ops.kernel_timer() as t:
        a, b = _two_model_steps(mod, fl)
    names = [r[0] for r in t.records]
    per_step = 5 if which == "translation_ssg" else 3
    assert names.count("pn2_fc_bn_forward_f32") == 2 * per_step == names.count("pn2_fc_bn_backward_f32")
    assert a.keys() == b.keys() and len(a) > 20
    for k in a:
        if a[k].dtype == np.float32:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k
    for layer in ("fc1.weight", "fc3.weight", "sa1.mlp_convs.0.weight"):
        assert float(np.abs(a["grad " + layer]).max()) > 0, layer

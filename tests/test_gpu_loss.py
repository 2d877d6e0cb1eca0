"""csrc/loss.hip on the device: pn2_log_softmax_rows_f32 / _backward_f32, pn2_criterion_forward_f32
/ _backward_f32, pn2_meter_update, their ops, pn2.losses, pn2.metrics and the train_loss route of
the heads (contracts and order rules: include/pn2.h).

Tolerances.  exp and log are the only operations of these kernels that are not correctly
rounded; a float64 value within an ulp of the exact one moves the float32 rounding by at most
one step, so everything that goes through them is held to 1 float32 ulp of the float64 host
evaluation (ulps(): the distance in representable float32 values).  Everything else is IEEE
arithmetic in a stated order and is held bit for bit to the same expression in numpy float64.
Every output matrix lies in a sentinel guard band (Mat3: contiguous, or leading dimension K + 3)
that result() checks.

The order of the loss chain.  At the input the order test is given -- one difference of 2^27,
the others near 1 -- the ascending and the reversed float64 chains differ (asserted on the
host), but both round to the same float32, so that input alone cannot tell a device's order
from the float32 result.  test_loss_order_shows_in_float32 adds inputs built so that the two
orders round to different float32 values (a chain that sits on a float32 tie unless four terms
of 2^-30 are added before the large ones)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
import metrics_ref as mr
from test_gpu_fc_train import _two_model_steps
from test_gpu_train_gemm import G, SENT, Mat, bits
from test_losses_host import bits64, run_meter
from test_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
NLL, MSE, L1, BCE = 0, 1, 2, 3
KINDS = {"nll": NLL, "mse": MSE, "l1": L1, "bce": BCE}
MEAN, SUM = 0, 1
LAYOUTS = ["contig", "ld"]


def _lib():
    from pn2 import _lib as lib
    return lib, lib.load()


class Mat3(Mat):
    """Mat with the leading dimension c + 3 in mode 'ld' (16-byte aligned base in both modes)."""

    def __init__(self, r, c, mode, host=None):
        self.r, self.c = r, c
        self.ld = c + 3 if mode == "ld" else c
        self.off = G
        self.buf = torch.full((self.off + r * self.ld + G,), SENT, device=DEV)
        if host is None:
            self.view().fill_(float("nan"))
        else:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(host, np.float32)))
        self.ptr = self.buf.data_ptr() + 4 * self.off


def ulps(a, b):
    """The distance between float32 arrays in representable values (NaN against NaN: 0)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(ordered(a) - ordered(b))
    both_nan = np.isnan(a) & np.isnan(b)
    assert not (np.isnan(a) ^ np.isnan(b)).any(), "NaN on one side only"
    return np.where(both_nan, 0, d)


# ------------------------------------------------------------------------------ log_softmax
@functools.lru_cache(maxsize=None)
def ls_inputs(B, K):
    g = np.random.default_rng(1000 * B + K)
    x = g.uniform(-30, 30, (B, K)).astype(np.float32)
    if B > 1:
        x[B // 2] = np.float32(1.25)  # a row of equal values
    dy = g.standard_normal((B, K), dtype=np.float32)
    x.setflags(write=False)
    dy.setflags(write=False)
    return x, dy


def ls_run(x, dy, mode):
    lib, L = _lib()
    B, K = x.shape
    X, Y, DY, DX = Mat3(B, K, mode, x), Mat3(B, K, mode), Mat3(B, K, mode, dy), Mat3(B, K, mode)
    st = lib.stream_ptr(X.buf.device)
    lib.check(L.pn2_log_softmax_rows_f32(X.ptr, X.ld, Y.ptr, Y.ld, B, K, st), "pn2_log_softmax_rows_f32")
    lib.check(L.pn2_log_softmax_rows_backward_f32(DY.ptr, DY.ld, Y.ptr, Y.ld, DX.ptr, DX.ld, B, K, st),
              "pn2_log_softmax_rows_backward_f32")
    y, dx = Y.result(), DX.result()
    assert np.array_equal(bits(X.result()), bits(x)) and np.array_equal(bits(DY.result()), bits(dy))
    return y, dx


@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("K", [1, 3, 7, 40])
@pytest.mark.parametrize("B", [1, 2, 65])
def test_log_softmax_values(B, K, mode):
    x, dy = ls_inputs(B, K)
    y, dx = ls_run(x, dy, mode)
    x64 = x.astype(np.float64)
    m = x64.max(1, keepdims=True)
    want = (x64 - m) - np.log(np.exp(x64 - m).sum(1, keepdims=True))
    worst = int(ulps(y, want.astype(np.float32)).max())
    print("log_softmax B=%d K=%d %s: forward worst %d ulp" % (B, K, mode, worst))
    assert worst <= 1
    if B > 1:
        # (x - m) - log(s) with x == m and s == K exactly
        assert np.array_equal(bits(y[B // 2]), bits(np.full(K, 0.0 - np.log(np.float64(K)), np.float32)))
    y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
    want_dx = dy64 - np.exp(y64) * dy64.sum(1, keepdims=True)
    worst = int(ulps(dx, want_dx.astype(np.float32)).max())
    print("log_softmax B=%d K=%d %s: backward worst %d ulp" % (B, K, mode, worst))
    assert worst <= 1


def test_log_softmax_rows_are_independent_and_repeat():
    from pn2 import ops
    x, dy = ls_inputs(65, 7)
    X, DY = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    Y = ops.log_softmax_rows_direct(X)
    DX = ops.log_softmax_rows_backward_direct(DY, Y)
    rows_y = torch.cat([ops.log_softmax_rows_direct(X[r:r + 1]) for r in range(65)])
    rows_dx = torch.cat([ops.log_softmax_rows_backward_direct(DY[r:r + 1], Y[r:r + 1]) for r in range(65)])
    assert np.array_equal(bits(rows_y.cpu().numpy()), bits(Y.cpu().numpy()))
    assert np.array_equal(bits(rows_dx.cpu().numpy()), bits(DX.cpu().numpy()))
    a, b = ls_run(x, dy, "ld"), ls_run(x, dy, "ld")
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(bits(a[0]), bits(Y.cpu().numpy())) and np.array_equal(bits(a[1]), bits(DX.cpu().numpy()))


def test_log_softmax_function_and_autograd():
    from pn2 import losses
    x, dy = ls_inputs(65, 7)
    X = torch.from_numpy(x).to(DEV).requires_grad_(True)
    Y = losses.log_softmax(X)
    (Y * torch.from_numpy(dy).to(DEV)).sum().backward()
    y, dx = ls_run(x, dy, "contig")
    assert np.array_equal(bits(Y.detach().cpu().numpy()), bits(y))
    assert np.array_equal(bits(X.grad.cpu().numpy()), bits(dx))


# ------------------------------------------------------------------------------ criteria
def crit_run(kind, reduction, p, t, mode, g=None):
    """Both C entries on Mat3 operands -> (loss float32 0-d, dP or None without g)."""
    lib, L = _lib()
    B, K = p.shape
    Pm = Mat3(B, K, mode, p)
    if kind == NLL:
        T = torch.from_numpy(np.ascontiguousarray(t, np.int64)).to(DEV)
        tp, ldt = T.data_ptr(), 0
    else:
        Tm = Mat3(B, K, mode, t)
        tp, ldt = Tm.ptr, Tm.ld
    loss = Mat3(1, 1, "contig")
    st = lib.stream_ptr(Pm.buf.device)
    rc = L.pn2_criterion_forward_f32(kind, reduction, Pm.ptr, Pm.ld, tp, ldt, B, K, loss.ptr, st)
    assert rc == 0
    dP = None
    if g is not None:
        gd = Mat3(1, 1, "contig", np.float32([[g]]))
        D = Mat3(B, K, mode)
        rc = L.pn2_criterion_backward_f32(kind, reduction, Pm.ptr, Pm.ld, tp, ldt, gd.ptr, B, K, D.ptr, D.ld, st)
        assert rc == 0
        dP = D.result()
    assert np.array_equal(bits(Pm.result()), bits(p))
    return loss.result()[0, 0], dP


@functools.lru_cache(maxsize=None)
def crit_inputs(kind, B):
    """(p, t) host arrays: K = 7 for nll (log-probabilities), 3 for mse / l1, 1 for bce (p with
    exactly 0, 1 and 0.5 in its first rows)."""
    g = np.random.default_rng(B * 10 + KINDS[kind])
    if kind == "nll":
        x = g.uniform(-5, 5, (B, 7))
        p = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
        t = g.integers(0, 7, size=B).astype(np.int64)
    elif kind == "bce":
        p = g.random((B, 1)).astype(np.float32)
        p[:3, 0] = np.float32([0.0, 1.0, 0.5])[:B]
        t = (g.random((B, 1)) < 0.5).astype(np.float32)
        if B >= 2:
            t[0, 0], t[1, 0] = 1.0, 0.0  # the clamped logarithms carry weight
    else:
        p = g.standard_normal((B, 3)).astype(np.float32)
        t = g.standard_normal((B, 3)).astype(np.float32)
        p[B // 2, 1] = t[B // 2, 1]  # p == t
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


def terms64(kind, p, t):
    """The float64 element terms, row-major, as include/pn2.h states them."""
    p64 = p.astype(np.float64)
    if kind == "nll":
        return -p64[np.arange(p.shape[0]), t]
    t64 = t.astype(np.float64)
    if kind == "bce":
        with np.errstate(divide="ignore"):
            lp, lq = np.maximum(np.log(p64), -100.0), np.maximum(np.log(1.0 - p64), -100.0)
        return (-(t64 * lp + (1.0 - t64) * lq)).reshape(-1)
    d = (p64 - t64).reshape(-1)
    return d * d if kind == "mse" else np.abs(d)


def chain(terms, reduction):
    """The ascending float64 chain from +0.0 (before the one rounding to float32)."""
    acc = np.float64(0.0)
    for v in terms:
        acc = acc + v
    return acc / np.float64(len(terms)) if reduction == MEAN else acc


@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("reduction", [MEAN, SUM])
@pytest.mark.parametrize("B", [1, 2, 65, 257])
@pytest.mark.parametrize("kind", ["nll", "bce"])
def test_nll_and_bce_forward(kind, B, reduction, mode):
    p, t = crit_inputs(kind, B)
    got, _ = crit_run(KINDS[kind], reduction, p, t, mode)
    terms = terms64(kind, p, t)
    assert np.isfinite(terms).all()
    want = terms.sum() / len(terms) if reduction == MEAN else terms.sum()
    d = int(np.max(ulps(got, np.float32(want))))
    print("%s B=%d reduction=%d %s: %d ulp" % (kind, B, reduction, mode, d))
    assert d <= 1
    if kind == "nll":  # no transcendental: the chain itself
        assert np.array_equal(bits(got), bits(np.float32(chain(terms, reduction))))


@functools.lru_cache(maxsize=None)
def order_inputs(B):
    """mse / l1 inputs whose sum depends on the order in float64: row 0 has a difference of 2^27,
    the rest random differences near 1."""
    g = np.random.default_rng(700 + B)
    t = g.standard_normal((B, 3)).astype(np.float32)
    p = (t + g.uniform(0.5, 1.4, (B, 3)).astype(np.float32) * g.choice(np.float32([-1, 1]), (B, 3))).astype(
        np.float32)
    p[0, 0] = np.float32(2.0 ** 27)
    t[0, 0] = np.float32(0.0)
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("reduction", [MEAN, SUM])
@pytest.mark.parametrize("B", [1, 2, 65, 257])
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_mse_and_l1_forward_is_the_ascending_chain(kind, B, reduction, mode):
    p, t = order_inputs(B)
    terms = terms64(kind, p, t)
    assert terms[0] == (2.0 ** 54 if kind == "mse" else 2.0 ** 27)
    up, down = chain(terms, reduction), chain(terms[::-1], reduction)
    if B >= 65:  # the two orders are different float64 numbers for this input
        assert not np.array_equal(bits64(up), bits64(down)), "the order is not observable"
    got, _ = crit_run(KINDS[kind], reduction, p, t, mode)
    assert np.array_equal(bits(got), bits(np.float32(up)))
    # and on everyday values
    p, t = crit_inputs(kind, B)
    got, _ = crit_run(KINDS[kind], reduction, p, t, mode)
    assert np.array_equal(bits(got), bits(np.float32(chain(terms64(kind, p, t), reduction))))


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_loss_order_shows_in_float32(kind):
    """Terms [2^24, 1, 2^-30 x 4] in some row-major arrangement: ascending, each 2^-30 is below
    half a float64 ulp of 2^24 + 1 and is lost, the chain is 2^24 + 1, a float32 tie that rounds
    to 2^24; with the small terms first they add up to 2^-28 and survive, and the chain rounds
    to 2^24 + 2.  The device must give the first for [large, small] and the second for
    [small, large]."""
    root = (lambda v: np.sqrt(v)) if kind == "mse" else (lambda v: v)
    large = [root(2.0 ** 24), 1.0]
    small = [root(2.0 ** -30)] * 4
    for seq, want in ((large + small, 2.0 ** 24), (small + large, 2.0 ** 24 + 2)):
        p = np.float32(seq).reshape(2, 3)
        t = np.zeros((2, 3), np.float32)
        terms = terms64(kind, p, t)
        assert sorted(terms.tolist()) == sorted([2.0 ** 24, 1.0] + [2.0 ** -30] * 4)
        assert np.float32(chain(terms, SUM)) == np.float32(want)
        assert np.float32(chain(terms[::-1], SUM)) != np.float32(want)
        for mode in LAYOUTS:
            got, _ = crit_run(KINDS[kind], SUM, p, t, mode)
            assert np.array_equal(bits(got), bits(np.float32(want))), (seq, mode)


def dterm64(kind, p, t):
    """term' [B, K] in float64 (include/pn2.h)."""
    p64 = p.astype(np.float64)
    if kind == "nll":
        out = np.zeros(p.shape)
        out[np.arange(p.shape[0]), t] = -1.0
        return out
    d = p64 - t.astype(np.float64)
    if kind == "mse":
        return 2.0 * d
    if kind == "l1":
        return np.sign(d)
    return d / np.maximum((1.0 - p64) * p64, 1e-12)


@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("reduction", [MEAN, SUM])
@pytest.mark.parametrize("B", [1, 2, 65, 257])
@pytest.mark.parametrize("kind", ["nll", "mse", "l1", "bce"])
def test_criterion_backward(kind, B, reduction, mode):
    p, t = crit_inputs(kind, B)
    g = np.float32(-1.7) if B == 2 else np.float32(0.37)
    _, dP = crit_run(KINDS[kind], reduction, p, t, mode, g=g)
    count = B if kind == "nll" else p.size
    c = np.float64(1.0) / np.float64(count) if reduction == MEAN else np.float64(1.0)
    want = ((np.float64(g) * c) * dterm64(kind, p, t)).astype(np.float32)
    assert np.array_equal(bits(dP), bits(want))
    assert np.isfinite(dP).all()
    if kind == "l1":
        assert dP[B // 2, 1] == 0  # p == t
    # torch's float64 autograd of the matching loss
    red = "mean" if reduction == MEAN else "sum"
    P64 = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    T = torch.from_numpy(t if kind == "nll" else t.astype(np.float64))
    fn = {"nll": lambda a, b: F.nll_loss(a, b, reduction=red), "mse": nn.MSELoss(reduction=red),
          "l1": nn.L1Loss(reduction=red), "bce": nn.BCELoss(reduction=red)}[kind]
    (fn(P64, T) * float(g)).backward()
    ref = P64.grad.numpy()
    assert (np.abs(dP.astype(np.float64) - ref) <= 1e-6 * np.abs(ref)).all()


@pytest.mark.parametrize("mode", LAYOUTS)
@pytest.mark.parametrize("reduction", [MEAN, SUM])
def test_bad_nll_target(reduction, mode):
    p, t = crit_inputs("nll", 65)
    t = t.copy()
    t[3], t[40] = -1, 7
    loss, dP = crit_run(NLL, reduction, p, t, mode, g=np.float32(1.0))  # both launches return 0
    assert np.isnan(loss)
    assert not bits(dP[3]).any() and not bits(dP[40]).any()
    good = np.ones(65, bool)
    good[[3, 40]] = False
    c = 1.0 / 65 if reduction == MEAN else 1.0
    assert np.array_equal(bits(dP[good]), bits((c * dterm64("nll", p[good], t[good])).astype(np.float32)))


@pytest.mark.parametrize("kind", ["nll", "mse", "l1", "bce"])
def test_loss_modules_run_the_kernels(kind):
    from pn2 import losses, ops
    p, t = crit_inputs(kind, 65)
    module, red = {"nll": (losses.ClsLoss(), MEAN), "mse": (losses.PoseLoss("L2_loss", "sum"), SUM),
                   "l1": (losses.PoseLoss("L1_loss", "mean"), MEAN), "bce": (losses.SignLoss(), MEAN)}[kind]
    P = torch.from_numpy(p).to(DEV).requires_grad_(True)
    with ops.kernel_timer() as timer:
        loss = module(P, torch.from_numpy(t).to(DEV))
        (loss * 0.37).backward()
    assert [r[0] for r in timer.records] == ["pn2_criterion_forward_f32", "pn2_criterion_backward_f32"]
    want, dP = crit_run(KINDS[kind], red, p, t, "contig", g=np.float32(0.37))
    assert loss.shape == () and np.array_equal(bits(loss.item()), bits(want))
    assert np.array_equal(bits(P.grad.cpu().numpy()), bits(dP))


# ------------------------------------------------------------------------------ meters
METERS = {"cls": "ClassificationMeter", "sign": "SignMeter", "pose": "PoseMeter"}


def same_result(a, b):
    assert type(a) is type(b)
    for name, x, y in zip(a._fields, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, name
        view = np.uint32 if x.dtype == np.float32 else np.uint64 if x.dtype == np.float64 else x.dtype
        assert np.array_equal(np.ascontiguousarray(x).view(view), np.ascontiguousarray(y).view(view)), name


@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("kind", sorted(METERS))
def test_device_meters_equal_the_numpy_path(kind, B):
    from pn2 import metrics
    data = mr.batches(B, 100 + B)
    cls = getattr(metrics, METERS[kind])
    dev_meter, host_meter = cls(mr.NUM_CATEGORY), cls(mr.NUM_CATEGORY)
    got = run_meter(dev_meter, data, kind, DEV)
    want = run_meter(host_meter, data, kind)
    same_result(got, want)
    acc, invalid, records = dev_meter._snapshot()
    acc_h, invalid_h, records_h = host_meter._snapshot()
    assert np.array_equal(bits64(acc), bits64(acc_h)) and invalid == invalid_h == 0
    assert np.array_equal(bits64(records), bits64(records_h))


@pytest.mark.parametrize("kind", sorted(METERS))
def test_device_meter_invalid_labels(kind):
    from pn2 import metrics
    data = mr.batches(5, 105)
    for d in data:
        d["label"][1], d["label"][3] = -1, mr.NUM_CATEGORY
    cls = getattr(metrics, METERS[kind])
    got = run_meter(cls(mr.NUM_CATEGORY), data, kind, DEV)
    want = run_meter(cls(mr.NUM_CATEGORY), data, kind)
    same_result(got, want)
    assert got.invalid == 6
    clean = [{k: v[[0, 2, 4]] for k, v in d.items()} for d in data]
    rest = run_meter(cls(mr.NUM_CATEGORY), clean, kind)
    cols = slice(0, 4) if kind == "pose" else slice(0, 2)
    if kind == "cls":  # the category is the target: the skipped rows are wrong predictions or not rows at all
        assert np.array_equal(got.table[:, 1], rest.table[:, 1])
    else:
        assert np.array_equal(bits64(got.table[:, cols]), bits64(rest.table[:, cols]))


def test_device_meter_grows_its_records():
    from pn2 import metrics
    m, h = metrics.ClassificationMeter(3), metrics.ClassificationMeter(3)
    for i in range(150):
        pred, target = torch.tensor([i % 3, 1, 2]), torch.tensor([0, 1, (i // 2) % 3])
        m.update(pred.to(DEV), target.to(DEV))
        h.update(pred, target)
    same_result(m.result(), h.result())
    assert len(m.result().records) == 150


def test_no_host_sync():
    """update of each meter, and each criterion's forward and backward, under torch's sync
    debug mode 'error' (a first call outside it binds the thread's error slot)."""
    from pn2 import losses, metrics
    data = [{k: v.to(DEV) for k, v in d.items()} for d in mr.batches(5, 105)]
    meters = {"cls": metrics.ClassificationMeter(7), "sign": metrics.SignMeter(7), "pose": metrics.PoseMeter(7)}
    crits = []
    for kind, module in (("nll", losses.ClsLoss()), ("mse", losses.PoseLoss("L2_loss", "sum")),
                         ("l1", losses.PoseLoss("L1_loss", "mean")), ("bce", losses.SignLoss())):
        p, t = crit_inputs(kind, 65)
        crits.append((module, torch.from_numpy(p).to(DEV).requires_grad_(True), torch.from_numpy(t).to(DEV)))
    x = torch.from_numpy(ls_inputs(65, 7)[0]).to(DEV).requires_grad_(True)

    def work():
        for d in data:  # update only: result() is the one readback
            meters["cls"].update(d["pred_choice"], d["label"])
            meters["sign"].update(d["sign"], d["sign_target"], d["label"])
            meters["pose"].update(d["pred"], d["target"], d["label"])
        for module, P, T in crits:
            module(P, T).backward()
        losses.log_softmax(x).sum().backward()

    work()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(30):  # past the first record buffer: the growth does not wait either
            work()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for m in meters.values():
        assert len(m.result().records) == 3 * 31


# ------------------------------------------------------------------------------ heads
def _head_outputs(which, key):
    """Train-mode forward at B = 4 -> (the head's log-probabilities, the logits its log_softmax
    received, the names of the kernels that ran)."""
    from pn2 import heads, heads_v1, ops, tuning
    module, factory, seed = {"cls_ssg": (heads, heads.ClsSSG, 300), "v1": (heads_v1, heads_v1.PointNetCls, 301)}[which]
    mod = cases.build_head(factory, seed).to(DEV).train()
    pts = cases.cloud("uniform3", 4, 1024, seed + 1).permute(0, 2, 1).contiguous().to(DEV)
    seen = []
    orig = module.head_log_softmax
    module.head_log_softmax = lambda x: seen.append(x.detach().clone()) or orig(x)
    try:
        with tuning.override(train_loss=key), ops.kernel_timer() as timer:
            torch.manual_seed(7)
            out = mod(pts)[0]
    finally:
        module.head_log_softmax = orig
    assert len(seen) == 1 and out.requires_grad and tuple(out.shape) == (4, 7)
    return out.detach(), seen[0], [r[0] for r in timer.records]


@pytest.mark.parametrize("which", ["cls_ssg", "v1"])
def test_heads_train_loss_route(which):
    out, logits, names = _head_outputs(which, 1)
    assert names.count("pn2_log_softmax_rows_f32") == 1
    x64 = logits.cpu().numpy().astype(np.float64)
    m = x64.max(1, keepdims=True)
    want = (x64 - m) - np.log(np.exp(x64 - m).sum(1, keepdims=True))
    assert int(ulps(out.cpu().numpy(), want.astype(np.float32)).max()) <= 1
    out0, logits0, names0 = _head_outputs(which, 0)
    assert "pn2_log_softmax_rows_f32" not in names0
    assert np.array_equal(bits(out0.cpu().numpy()), bits(F.log_softmax(logits0, -1).cpu().numpy()))


# ------------------------------------------------------------------------------ whole-model step
@pytest.mark.parametrize("which", ["cls_ssg", "translation_ssg"])
def test_reproducible_whole_model_step_with_the_loss_kernels(which):
    """Two steps from one saved state under group_backward, train_gemm, train_head (set by
    _two_model_steps) and train_loss: the loss, every gradient, buffer and parameter after
    Adam.step() bit-identical; and against the same step with the torch criterion, the
    tolerances of test_gpu_fc_train.py (1e-4 for outputs and buffers, 1e-3 for what comes from
    gradients -- the parameters after the step)."""
    from pn2 import heads, losses, ops, tuning
    B, N = 4, 1024
    g = torch.Generator().manual_seed(180)
    if which == "cls_ssg":
        mod = cases.build_head(heads.ClsSSG, 181).to(DEV).train()
        pts = cases.cloud("uniform3", B, N, 182).permute(0, 2, 1).contiguous().to(DEV)
        target = torch.tensor([1, 4, 6, 0], device=DEV)
        crit = losses.ClsLoss()
        ours = lambda m: crit(m(pts)[0], target, None)
        theirs = lambda m: F.nll_loss(m(pts)[0], target)
    else:
        mod = cases.build_head(heads.TranslationSSG, 183).to(DEV).train()
        pts = cases.cloud("onehot10", B, N, 184).permute(0, 2, 1).contiguous().to(DEV)
        mean = torch.randn(B, 3, generator=g).to(DEV)
        target = torch.randn(B, 3, generator=g).to(DEV)
        crit = losses.PoseLoss("L2_loss", "sum")
        ours = lambda m: crit(m(pts, mean), target)
        theirs = lambda m: F.mse_loss(m(pts, mean), target, reduction="sum")

    def with_key(fn):
        def run(m):
            with tuning.override(train_loss=1):
                return fn(m)
        return run

    state = copy.deepcopy(mod.state_dict())  # _two_model_steps leaves the model one step on
    with ops.kernel_timer() as timer:
        a, b = _two_model_steps(mod, with_key(ours))
    names = [r[0] for r in timer.records]
    assert names.count("pn2_criterion_forward_f32") == 2 == names.count("pn2_criterion_backward_f32")
    assert names.count("pn2_log_softmax_rows_f32") == (2 if which == "cls_ssg" else 0)
    assert names.count("pn2_log_softmax_rows_backward_f32") == (2 if which == "cls_ssg" else 0)
    assert a.keys() == b.keys() and len(a) > 20
    for k in a:
        if a[k].dtype == np.float32:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["loss"]) and float(np.abs(a["grad fc3.weight"]).max()) > 0
    mod.load_state_dict(state)
    ref, _ = _two_model_steps(mod, with_key(theirs))
    close(a["loss"], ref["loss"], 1e-4, "loss")
    for k in a:
        if k.startswith("param "):
            close(a[k], ref[k], 1e-3, k)
        elif k.startswith("buf ") and a[k].dtype == np.float32:
            close(a[k], ref[k], 1e-4, k)

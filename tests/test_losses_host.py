"""pn2.losses and pn2.metrics on CPU tensors (no GPU): the modules call the torch functions the
reference's get_loss classes call -- the same bits, the same gradients -- and the meters' numpy
path is held against the reference test loops restated in tests/metrics_ref.py.

Bounds of the pose meter against the loops' torch float32 means, per averaged set of n rows:
    |got - torch| <= (n - 1) * 2^-24 * max|a|           (a float32 sum of n terms)
summed over the batches for an accumulated class sum; and each record within one float32 ulp of
float32(np.mean(a.astype(float64), 0))."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import metrics_ref as mr

U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pair(module, reference, pred0, *rest):
    out = []
    for fn in (module, reference):
        pred = pred0.clone().requires_grad_(True)
        loss = fn(pred, *rest)
        loss.backward()
        out.append((loss.detach().numpy(), pred.grad.numpy()))
    (l0, g0), (l1, g1) = out
    assert l0.dtype == np.float32 and l0.shape == l1.shape == ()
    assert np.array_equal(bits(l0), bits(l1))
    assert np.array_equal(bits(g0), bits(g1))


def test_cls_loss_is_nll_loss_on_cpu():
    from pn2 import losses
    g = torch.Generator().manual_seed(1)
    pred = F.log_softmax(torch.randn(24, 7, generator=g) * 3, -1)
    target = torch.randint(0, 7, (24,), generator=g)
    _pair(losses.ClsLoss(), lambda p, t: F.nll_loss(p, t), pred, target)
    _pair(lambda p, t: losses.ClsLoss()(p, t, torch.zeros(3)), lambda p, t: F.nll_loss(p, t), pred, target)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("kind", ["L2_loss", "L1_loss"])
def test_pose_loss_is_the_torch_module_on_cpu(kind, reduction):
    from pn2 import losses
    g = torch.Generator().manual_seed(2)
    pred, target = torch.randn(32, 3, generator=g), torch.randn(32, 3, generator=g)
    ref = nn.MSELoss(reduction=reduction) if kind == "L2_loss" else nn.L1Loss(reduction=reduction)
    _pair(losses.PoseLoss(kind, reduction), ref, pred, target)


def test_pose_loss_defaults_are_the_reference_s():
    from pn2 import losses
    m = losses.PoseLoss()
    assert (m.kind, m.reduction) == ("mse", "mean")
    assert losses.PoseLoss(type="anything else").kind == "l1"


def test_sign_loss_is_bce_loss_on_cpu():
    from pn2 import losses
    g = torch.Generator().manual_seed(3)
    pred = torch.sigmoid(torch.randn(24, 1, generator=g) * 4)
    target = (torch.rand(24, 1, generator=g) < 0.5).float()
    _pair(losses.SignLoss(), nn.BCELoss(), pred, target)


def test_log_softmax_on_cpu_is_torch_s():
    from pn2 import losses, tuning
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(4))
    assert torch.equal(losses.log_softmax(x), F.log_softmax(x, -1))
    with tuning.override(train_loss=1):
        assert torch.equal(losses.head_log_softmax(x.requires_grad_(True)), F.log_softmax(x, -1))


# ------------------------------------------------------------------------------ meters
def run_meter(meter, data, kind, device=None):
    """Feed the three batches to a fresh meter -> its result (device None: the numpy path)."""
    to = (lambda t: t) if device is None else (lambda t: t.to(device))
    for d in data:
        if kind == "cls":
            meter.update(to(d["pred_choice"]), to(d["label"]))
        elif kind == "sign":
            meter.update(to(d["sign"]), to(d["sign_target"]), to(d["label"]))
        else:
            meter.update(to(d["pred"]), to(d["target"]), to(d["label"]))
    return meter.result()


def same64(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(bits64(a), bits64(b)), what  # NaN included: numpy's quiet NaN on both sides


@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("kind", ["cls", "sign"])
def test_accuracy_meters_match_the_reference_loops(kind, B):
    from pn2 import metrics
    data = mr.batches(B, 100 + B)
    if kind == "cls":
        got = run_meter(metrics.ClassificationMeter(mr.NUM_CATEGORY), data, kind)
        inst, cls, table, per_batch = mr.classification_test(data)
    else:
        got = run_meter(metrics.SignMeter(mr.NUM_CATEGORY), data, kind)
        inst, cls, table, per_batch = mr.sign_test(data)
    same64(got.instance_accuracy, inst, "instance accuracy")
    same64(got.class_accuracy, cls, "class accuracy")
    same64(got.table, table, "table")
    same64(got.records, per_batch, "per-batch records")
    assert got.invalid == 0
    assert np.isnan(got.table[6, 2]) and np.isnan(got.class_accuracy)  # category 6 never appears
    if B == 65:
        present = [set(d["label"].tolist()) for d in data]
        assert 2 in present[0] and 2 not in present[1] and 2 in present[2]
        assert got.table[2, 1] == (2 if kind == "cls" else sum(int((d["label"] == 2).sum()) for d in data))


@pytest.mark.parametrize("B", [1, 5, 65])
def test_pose_meter_against_the_reference_loop(B):
    from pn2 import metrics
    data = mr.batches(B, 100 + B)
    got = run_meter(metrics.PoseMeter(mr.NUM_CATEGORY), data, "pose")
    mean_loss, table, per_batch = mr.pose_test(data)
    assert got.table.shape == table.shape == (7, 7) and got.records.shape == per_batch.shape == (3, 3)
    assert got.records.dtype == np.float32 and got.invalid == 0
    same64(got.table[:, 0], table[:, 0], "batches per class")
    sum_bound = np.zeros((7, 3))
    for i, d in enumerate(data):
        a = np.abs(d["pred"].numpy() - d["target"].numpy())
        assert a.dtype == np.float32
        # the records: the loop's float32 mean, and the float64 mean rounded once
        bound = (B - 1) * U * float(a.max())
        err = np.abs(got.records[i].astype(np.float64) - per_batch[i].astype(np.float64))
        print("B=%d batch %d: record error %.3g bound %.3g" % (B, i, err.max(), bound))
        assert (err <= bound).all(), "record %d" % i
        want = np.mean(a.astype(np.float64), 0).astype(np.float32)
        assert (np.abs(got.records[i].astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
        for c in range(7):
            rows = d["label"].numpy() == c
            if rows.any():
                sum_bound[c] += (int(rows.sum()) - 1) * U * a[rows].max(0).astype(np.float64)
    err = np.abs(got.table[:, 1:4] - table[:, 1:4])
    print("B=%d: class sum error %.3g, bound %.3g" % (B, err.max(), sum_bound.max()))
    assert (err <= sum_bound).all(), "class sums"
    # the quotients and the final mean are the reference's operations on the meter's own numbers
    with np.errstate(invalid="ignore", divide="ignore"):
        same64(got.table[:, 4:7], got.table[:, 1:4] / got.table[:, :1], "class means")
    assert np.isnan(got.table[6, 4:7]).all() and not got.table[6, :4].any()
    assert got.mean_loss.dtype == np.float32
    assert np.array_equal(bits(got.mean_loss), bits(np.mean(got.records)))
    # against the loop's: the records differ by at most the bound above, and each side's np.mean
    # is a float32 sum of 9 terms
    amax = max(float(np.abs(d["pred"].numpy() - d["target"].numpy()).max()) for d in data)
    assert abs(float(got.mean_loss) - float(mean_loss)) <= (B - 1) * U * amax + 2 * 8 * U * amax


def test_invalid_labels_are_counted_not_indexed():
    from pn2 import metrics
    label = torch.tensor([0, -1, 7, 3, 3])
    pred = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    target = torch.zeros(5, 3)
    m = metrics.PoseMeter(7)
    m.update(pred, target, label)
    r = m.result()
    assert r.invalid == 2 and r.table[:, 0].tolist() == [1, 0, 0, 1, 0, 0, 0]
    assert r.table[0, 1:4].tolist() == [0, 1, 2] and r.table[3, 1:4].tolist() == [10.5, 11.5, 12.5]
    assert r.records.tolist() == [[6, 7, 8]]  # the record averages every row
    c = metrics.ClassificationMeter(7)
    c.update(torch.tensor([0, 1, 2, 3, 3]), label)
    r = c.result()
    assert r.invalid == 2 and r.table[:, 1].tolist() == [1, 0, 0, 1, 0, 0, 0] and r.records.tolist() == [0.6]
    s = metrics.SignMeter(7)
    s.update(torch.ones(5, 1), torch.tensor([1., 1., -1., 1., -1.]), label)
    r = s.result()
    assert r.invalid == 2 and r.table[:, :2].tolist() == [[1, 1], [0, 0], [0, 0], [1, 2], [0, 0], [0, 0], [0, 0]]


def test_reset_and_many_batches():
    from pn2 import metrics
    m = metrics.ClassificationMeter(3)
    for i in range(70):
        m.update(torch.tensor([i % 3, 1]), torch.tensor([0, 1]))
    r = m.result()
    assert len(r.records) == 70 and r.table[0, 1] == 70
    m.reset()
    assert len(m.result().records) == 0 and not m.result().table[:, :2].any()

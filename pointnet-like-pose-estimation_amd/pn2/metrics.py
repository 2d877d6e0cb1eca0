"""The reference loops' per-batch and per-class metrics, accumulated where the predictions are.

The reference's test loops index with a boolean mask and read one number back per category and
batch, its train loops one per step:

  ClassificationMeter  train_classification.py:121-122 (train), 144-156 (test)
  SignMeter            train_sign.py:123-124, 148-159
  PoseMeter            train_rotation.py:126-127, 130-131 (train), 157-169 (test); the
                       translation loop likewise

``update(...)`` of a meter fed CUDA tensors issues ONE launch (pn2_meter_update, csrc/loss.hip)
into float64 state on that device and never waits for the device; ``result()`` does the one
readback and finishes as the reference does: ``np.mean`` of the per-batch records, the
per-class quotients, ``np.mean`` of those (a class that never appeared gives numpy's NaN, as
there).  CPU tensors or arrays take a numpy path with the same arithmetic, operation for
operation (include/pn2.h states it), so both give the same bits.  A label outside
[0, num_category) is skipped and counted in ``invalid`` (the reference would index out of
range, or wrap a negative one).  Not captured into graphs: the record slot is a launch
argument.
"""
import collections

import numpy as np
import torch

from . import ops

AccuracyResult = collections.namedtuple("AccuracyResult", ["instance_accuracy", "class_accuracy", "table",
                                                           "invalid", "records"])
PoseResult = collections.namedtuple("PoseResult", ["mean_loss", "table", "invalid", "records"])


def _host(t, dtype):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


def _chain(v):
    """The float64 sum of v in index order from +0.0 (np.add.accumulate is strictly serial)."""
    v = np.asarray(v, np.float64)
    return np.add.accumulate(np.concatenate((np.zeros(1), v)))[-1]


class _Meter:
    kind = None

    def __init__(self, num_category):
        self.num_category = int(num_category)
        if self.num_category < 1:
            raise ValueError("num_category must be positive")
        self.reset()

    def reset(self):
        """Forget every batch (the state is allocated again by the next update)."""
        self._device = None   # None: nothing yet; "numpy"; or a torch.device
        self._state = None    # device: one float64 tensor [acc | invalid | records]
        self._acc = self._invalid = self._records = None  # numpy path, or views of _state
        self._n = 0
        self._D = 1

    # ---- state
    def _widths(self):
        return (1 + self._D, self._D) if self.kind == "pose" else (2, 1)

    def _views(self, state, cap):
        W, RW = self._widths()
        a = self.num_category * W
        return state[:a].view(self.num_category, W), state[a:a + 1], state[a + 1:].view(cap, RW)

    def _begin(self, device, D):
        if self._device is None:
            self._device, self._D = device, D
            W, RW = self._widths()
            if device == "numpy":
                self._acc = np.zeros((self.num_category, W))
                self._invalid = np.zeros(1)
                self._records = []
            else:
                cap = 64
                self._state = torch.zeros(self.num_category * W + 1 + cap * RW, dtype=torch.float64, device=device)
                self._acc, self._invalid, self._records = self._views(self._state, cap)
        elif self._device != device or self._D != D:
            raise ValueError("a meter's batches come from one device and have one width (reset() between)")
        if device != "numpy" and self._n == self._records.shape[0]:
            # grow between launches: a device copy on the stream, no wait
            cap = 2 * self._n
            W, RW = self._widths()
            head = self.num_category * W + 1
            state = torch.zeros(head + cap * RW, dtype=torch.float64, device=device)
            state[:self._state.numel()].copy_(self._state)
            self._state = state
            self._acc, self._invalid, self._records = self._views(state, cap)

    def _launch(self, pred, target, label):
        ops.meter_update_direct(self.kind, pred, target, label, self.num_category, self._acc, self._invalid,
                                self._records, self._n)
        self._n += 1

    def _snapshot(self):
        """(acc, invalid, records [n, RW]) on the host: the one readback."""
        W, RW = self._widths()
        if self._device is None:
            return np.zeros((self.num_category, W)), 0, np.zeros((0, RW))
        if self._device == "numpy":
            return self._acc.copy(), int(self._invalid[0]), np.asarray(self._records, np.float64).reshape(-1, RW)
        host = self._state.cpu().numpy()
        a = self.num_category * W
        return (host[:a].reshape(self.num_category, W).copy(), int(host[a]),
                host[a + 1:a + 1 + self._n * RW].reshape(self._n, RW).copy())

    # ---- numpy path pieces
    def _count_invalid(self, label):
        self._invalid[0] += float(np.count_nonzero((label < 0) | (label >= self.num_category)))


class _AccuracyMeter(_Meter):
    def _update_host(self, hit, label):
        B = hit.shape[0]
        for c in range(self.num_category):
            rows = label == c
            count = int(np.count_nonzero(rows))
            if count == 0:
                continue
            correct = int(np.count_nonzero(hit[rows]))
            if self.kind == "cls":
                self._acc[c, 0] += float(correct) / float(count)
                self._acc[c, 1] += 1.0
            else:
                self._acc[c, 0] += float(correct)
                self._acc[c, 1] += float(count)
        self._records.append([float(np.count_nonzero(hit)) / float(B)])
        self._count_invalid(label)
        self._n += 1

    def result(self):
        """AccuracyResult(instance_accuracy, class_accuracy, table [num_category, 3] -- the
        reference's class_accuracy array --, invalid, records): train_classification.py:152-156."""
        acc, invalid, records = self._snapshot()
        table = np.zeros((self.num_category, 3))
        table[:, :2] = acc
        with np.errstate(invalid="ignore", divide="ignore"):
            table[:, 2] = table[:, 0] / table[:, 1]
            class_accuracy = np.mean(table[:, 2])
            instance_accuracy = np.mean(records[:, 0]) if len(records) else np.float64("nan")
        return AccuracyResult(instance_accuracy, class_accuracy, table, invalid, records[:, 0])


class ClassificationMeter(_AccuracyMeter):
    """update(pred_choice, target): the predicted and the true class of every cloud of a batch."""
    kind = "cls"

    def update(self, pred_choice, target):
        if torch.is_tensor(pred_choice) and pred_choice.is_cuda:
            self._begin(pred_choice.device, 1)
            self._launch(pred_choice.detach().reshape(-1).long(),
                         target.detach().to(pred_choice.device).reshape(-1).long(), None)
            return
        pred_choice, target = _host(pred_choice, np.int64).reshape(-1), _host(target, np.int64).reshape(-1)
        self._begin("numpy", 1)
        self._update_host(pred_choice == target, target)


class SignMeter(_AccuracyMeter):
    """update(sign, target, label): the sign head's output [B, 1] (or [B]), its target and the
    category of every cloud; a cloud is correct when sign == target as floats."""
    kind = "sign"

    def update(self, sign, target, label):
        if torch.is_tensor(sign) and sign.is_cuda:
            self._begin(sign.device, 1)
            self._launch(sign.detach().reshape(-1).float(), target.detach().to(sign.device).reshape(-1).float(),
                         label.detach().to(sign.device).reshape(-1).long())
            return
        sign, target = _host(sign, np.float32).reshape(-1), _host(target, np.float32).reshape(-1)
        self._begin("numpy", 1)
        self._update_host(sign == target, _host(label, np.int64).reshape(-1))


class PoseMeter(_Meter):
    """update(pred, target, label): the regressed and the true vector [B, D] (D = 3 in the
    reference) and the category of every cloud; the metric is the mean absolute error per axis."""
    kind = "pose"

    def update(self, pred, target, label):
        if torch.is_tensor(pred) and pred.is_cuda:
            if pred.dim() != 2:
                raise ValueError("PoseMeter: pred [B, D]")
            self._begin(pred.device, pred.shape[1])
            self._launch(pred.detach().float(), target.detach().to(pred.device).float(),
                         label.detach().to(pred.device).reshape(-1).long())
            return
        pred, target = _host(pred, np.float32), _host(target, np.float32)
        if pred.ndim != 2 or target.shape != pred.shape:
            raise ValueError("PoseMeter: pred [B, D] and a target of its shape")
        label = _host(label, np.int64).reshape(-1)
        B, D = pred.shape
        self._begin("numpy", D)
        a = np.abs(pred - target)  # float32: one subtraction
        for c in range(self.num_category):
            rows = label == c
            count = int(np.count_nonzero(rows))
            if count == 0:
                continue
            self._acc[c, 0] += 1.0
            for k in range(D):
                self._acc[c, 1 + k] += np.float64(np.float32(_chain(a[rows, k]) / np.float64(count)))
        self._records.append([np.float64(np.float32(_chain(a[:, k]) / np.float64(B))) for k in range(D)])
        self._count_invalid(label)
        self._n += 1

    def result(self):
        """PoseResult(mean_loss, table [num_category, 1 + 2 D] -- the reference's class_loss
        array: batches seen, the per-axis sums, the per-axis means --, invalid, records float32
        [batches, D]): train_rotation.py:165-169."""
        acc, invalid, records = self._snapshot()
        D = self._D
        table = np.zeros((self.num_category, 1 + 2 * D))
        table[:, :1 + D] = acc
        records = records.astype(np.float32)  # exact: every record is a float32 mean
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in range(D):
                table[:, 1 + D + k] = table[:, 1 + k] / table[:, 0]
            mean_loss = np.mean(records) if len(records) else np.float32("nan")
        return PoseResult(mean_loss, table, invalid, records)

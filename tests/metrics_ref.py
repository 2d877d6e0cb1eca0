"""The reference test loops' metric bookkeeping restated over lists of batches, with the torch
and numpy calls the loops make (CPU tensors), so that pn2.metrics can be held against them:

  classification_test  train_classification.py:128-156: per category of a batch (np.unique of the
                       targets, :144) the share of correct predictions among that category's
                       clouds is added to column 0 and 1 to column 1 (:145-147); per batch
                       correct / B is appended (:149-150); at the end column 2 = column 0 /
                       column 1, the class accuracy is its np.mean and the instance accuracy the
                       np.mean of the appended values (:152-154)
  sign_test            train_sign.py:130-159: per category of a batch (the labels, :148) the
                       number of clouds whose sign equals the target (cast to long, :149) goes to
                       column 0 and the category's cloud count to column 1 (:150); the batch
                       record compares with the float target (:152-153); the end as above
  pose_test            train_rotation.py:136-171: per category of a batch torch.mean over that
                       category's rows of |pred - target| (:158) is added, as a float32 numpy
                       array, to columns 1:4 of a float64 table and 1 to column 0 (:159-160);
                       the batch record is torch.mean(|pred - target|, dim=0) (:162-163); at the
                       end columns 4:7 = columns 1:4 / column 0 (:165-167) and the loss is the
                       np.mean of the stacked float32 records (:168-169)

``batches(B, seed)`` makes the three-batch inputs the tests share: 7 categories with unequal
shares, category 2 absent from the second batch, category 6 never present."""
import numpy as np
import torch

NUM_CATEGORY = 7


def batches(B, seed):
    """Three batches of B clouds -> list of dicts of CPU tensors: label int64 [B], pred_choice
    int64 [B] (about 60% right), sign / sign_target float32 [B,1] / [B] in {-1, 0, 1} / {-1, 1},
    pred / target float32 [B,3]."""
    g = np.random.default_rng(seed)
    shares = np.array([0.35, 0.05, 0.2, 0.1, 0.1, 0.2, 0.0])
    out = []
    for i in range(3):
        p = shares.copy()
        if i == 1:
            p[2] = 0.0
        label = g.choice(NUM_CATEGORY, size=B, p=p / p.sum())
        wrong = g.integers(0, NUM_CATEGORY, size=B)
        pred_choice = np.where(g.random(B) < 0.6, label, wrong)
        sign_target = g.choice(np.array([-1.0, 1.0], np.float32), size=B)
        sign = np.where(g.random(B) < 0.7, sign_target, g.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=B))
        pred = g.standard_normal((B, 3), dtype=np.float32)
        target = pred + g.standard_normal((B, 3), dtype=np.float32) * np.float32(0.1 * (i + 1))
        out.append(dict(label=torch.from_numpy(label.astype(np.int64)),
                        pred_choice=torch.from_numpy(pred_choice.astype(np.int64)),
                        sign=torch.from_numpy(sign.astype(np.float32).reshape(B, 1)),
                        sign_target=torch.from_numpy(sign_target.astype(np.float32)),
                        pred=torch.from_numpy(pred), target=torch.from_numpy(target)))
    return out


def _finish(table, per_batch):
    with np.errstate(invalid="ignore", divide="ignore"):
        table[:, 2] = table[:, 0] / table[:, 1]
        return np.mean(per_batch), np.mean(table[:, 2]), table, per_batch


def classification_test(data, num_category=NUM_CATEGORY):
    """-> (instance accuracy, class accuracy, the [num_category, 3] table, the per-batch list)."""
    per_batch = []
    table = np.zeros((num_category, 3))
    for d in data:
        chosen, target = d["pred_choice"], d["label"]
        for cat in np.unique(target.cpu()):
            rows = target == cat
            right = chosen[rows].eq(target[rows].long().data).cpu().sum()
            table[cat, 0] += right.item() / float(chosen[rows].size()[0])
            table[cat, 1] += 1
        right = chosen.eq(target.long().data).cpu().sum()
        per_batch.append(right.item() / float(chosen.size()[0]))
    return _finish(table, per_batch)


def sign_test(data, num_category=NUM_CATEGORY):
    per_batch = []
    table = np.zeros((num_category, 3))
    for d in data:
        sign, target, label = d["sign"], d["sign_target"], d["label"]
        for cat in np.unique(label.cpu()):
            rows = label == cat
            table[cat, 0] += sign[rows].reshape(1, -1).eq(target[rows].long().data).cpu().sum()
            table[cat, 1] += float(sign[rows].size()[0])
        right = sign.eq(target.float().reshape(-1, 1).data).cpu().sum()
        per_batch.append(right.item() / float(sign.size()[0]))
    return _finish(table, per_batch)


def pose_test(data, num_category=NUM_CATEGORY):
    """-> (mean loss, the [num_category, 7] table, the stacked float32 per-batch records)."""
    per_batch = []
    table = np.zeros((num_category, 7))
    for d in data:
        pred, target, label = d["pred"], d["target"], d["label"]
        for cat in np.unique(label.cpu()):
            rows = label == cat
            err = torch.abs(pred[rows] - target[rows])
            table[cat, 1:4] += torch.mean(err, dim=0).detach().cpu().numpy()
            table[cat, 0] += 1
        err = torch.abs(pred - target)
        per_batch.append(torch.mean(err, dim=0).detach().cpu().numpy())
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            table[:, 4 + k] = table[:, 1 + k] / table[:, 0]
    per_batch = np.asanyarray(per_batch)
    return np.mean(per_batch), table, per_batch

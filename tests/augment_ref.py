"""The training scripts' per-batch preparation restated in numpy (train_translation.py:109-119
with provider.py's random_point_dropout :157-164, random_scale_point_cloud :144-155 and
shift_point_cloud :131-142), split in two so that the draws can be handed over:

  literal_draws   the generator calls of the three functions, cloud by cloud, as they make them
  prepare_train   what they do to the batch with those draws, then the eval-side preparation
                  (oracle.prepare_points: mean of the first 3 points, normalization, float32,
                  one-hot)

tests/test_augment.py pins both to the reference through tests/golden/augment_*.npz, which
make_goldens_augment.py wrote by running the reference's own functions."""
import collections

import numpy as np

import oracle

Draws = collections.namedtuple("Draws", ["drop", "scale", "shift"])


def literal_draws(B, N, rs=None, dropout=True, scale=True, shift=True, max_dropout_ratio=0.875,
                  scale_low=0.8, scale_high=1.25, shift_range=0.1):
    """rs: np.random (None) or a RandomState.  One generator call per call of the reference."""
    rs = np.random if rs is None else rs
    drop = sc = sh = None
    if dropout:
        drop = np.zeros((B, N), dtype=bool)
        for b in range(B):
            dropout_ratio = rs.random_sample() * max_dropout_ratio
            drop[b] = rs.random_sample((N,)) <= dropout_ratio
    if scale:
        sc = rs.uniform(scale_low, scale_high, B)
    if shift:
        sh = rs.uniform(-shift_range, shift_range, (B, 3))
    return Draws(drop, sc, sh)


def augment(points, draws):
    """float64 [B,N,C] -> the augmented float64 copy (the reference works in place)."""
    points = np.array(points, dtype=np.float64, copy=True)
    B = points.shape[0]
    for b in range(B):
        if draws.drop is not None:
            drop_idx = np.where(draws.drop[b])[0]
            if len(drop_idx) > 0:
                points[b, drop_idx, :] = points[b, 0, :]
    for b in range(B):
        if draws.scale is not None:
            points[b, :, 0:3] *= draws.scale[b]
    for b in range(B):
        if draws.shift is not None:
            points[b, :, 0:3] += draws.shift[b, :]
    return points


def prepare_train(points, labels, draws, num_category=7, with_mean=True, normalize=True):
    """-> (float32 [B,N,C+K] storage of the model input, float32 mean [B,C] or None)."""
    with np.errstate(invalid="ignore", divide="ignore"):  # an all-dropped cloud: 0 / 0
        return oracle.prepare_points(augment(points, draws), labels, num_category,
                                     with_mean=with_mean, normalize=normalize)

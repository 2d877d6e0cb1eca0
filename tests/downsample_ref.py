"""The reference's numpy farthest-point downsampling restated (provider.py:183-204, and the
textually identical copies data_utils/ModelDataLoader.py:10-31, data_utils/ModelNetDataLoader.py:
25-46, point_collect/transformer.py:120-141, colledt_data_structure/transformer.py:120-141,
data_build/Cube.py:102-123), split in two so that the start can be handed over:

  sample_indices   the serial loop for a given start: which row each iteration picks
  farthest_point_sample / farthest_point_sample_loop
                   the draw (one np.random.randint(0, N) per cloud, from the global generator)
                   and the gather of all C columns

The rule, in the cloud's own dtype (float64 rows of np.loadtxt; float32 in the ModelNet loader):
only columns 0..2 are measured; the running distance starts at a finite 1e10 and is replaced
where the new distance is strictly smaller; the next centroid is the first index of the
maximum; `number` iterations run even past N (indices then repeat).

tests/test_downsample_ref.py pins this file to the reference through tests/golden/
downsample_*.npz, which make_goldens_downsample.py wrote by running the reference's own function.

The variants (arith=...) are what a kernel could get wrong, for the goldens whose purpose is to
tell them apart: "wide" measures a float32 cloud in float64, "fma" contracts the channel sum's
multiplies into its adds the way a compiler would: fma(d2, d2, fma(d1, d1, d0*d0)).

PROPERTIES names what each golden exists for; the generator searches its seeds until the
property holds and tests/test_downsample_ref.py checks it again."""
import fractions
import math

import numpy as np


def _dist_exact(xyz, centroid):
    return np.sum((xyz - centroid) ** 2, -1)


def _dist_wide(xyz, centroid):
    return np.sum((xyz.astype(np.float64) - centroid.astype(np.float64)) ** 2, -1)


def _fma32(a, b, c):
    """float32 fma through float64: the product is exact there (24 + 24 bits) and the sum is
    rounded to 53 bits before the rounding to 24.  That double rounding can differ from a true
    fma on a rare tie, which is harmless here: the goldens need a contracted sequence that
    differs from the exact one, not every contracted sequence."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _fma64(a, b, c):
    """float64 fma, exact: math.fma where the interpreter has it, else rational arithmetic
    (float() of a Fraction rounds once, to nearest even)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    F = fractions.Fraction
    return float(F(a) * F(b) + F(c))


def _dist_fma(xyz, centroid):
    d = xyz - centroid
    if xyz.dtype == np.float32:
        s = d[:, 0] * d[:, 0]
        s = _fma32(d[:, 1], d[:, 1], s)
        return _fma32(d[:, 2], d[:, 2], s)
    out = np.empty(len(d), dtype=np.float64)
    for n, (a, b, c) in enumerate(d.tolist()):
        out[n] = _fma64(c, c, _fma64(b, b, a * a))
    return out


_DIST = {"exact": _dist_exact, "wide": _dist_wide, "fma": _dist_fma}


def sample_indices(point_cloud, number, start, arith="exact", ties=None):
    """-> int64 [number]: the row picked by each iteration.  ties: a list that receives, per
    iteration, the (first, last) index holding the maximum."""
    N = point_cloud.shape[0]
    xyz = point_cloud[:, :3]
    dist_of = _DIST[arith]
    idx = np.zeros((number,), dtype=np.int64)
    distance = np.full((N,), 1e10, dtype=np.float64 if arith == "wide" else point_cloud.dtype)
    farthest = int(start)
    for i in range(number):
        idx[i] = farthest
        dist = dist_of(xyz, xyz[farthest, :])
        mask = dist < distance
        distance[mask] = dist[mask]
        farthest = int(np.argmax(distance, -1))
        if ties is not None:
            holders = np.flatnonzero(distance == distance[farthest])
            ties.append((int(holders[0]), int(holders[-1])))
    return idx


def farthest_point_sample(point_cloud, number):
    """The reference's function: one draw from the global generator, then the gathered rows."""
    N, C = point_cloud.shape
    start = np.random.randint(0, N)
    return point_cloud[sample_indices(point_cloud, number, start)]


def farthest_point_sample_loop(clouds, number):
    """The reference called once per cloud, in list order -> list of [number, C] arrays."""
    return [farthest_point_sample(pc, number) for pc in clouds]


# ------------------------------------------------------------------ what a golden exists for
def _has_tie(cloud, number, idx):
    ties = []
    sample_indices(cloud, number, idx[0], ties=ties)
    return any(a != b for a, b in ties[:-1])  # the last iteration's argmax is never used


def _differs(arith):
    def prop(cloud, number, idx):
        return not np.array_equal(sample_indices(cloud, number, idx[0], arith=arith), idx)
    return prop


def _all_far(cloud, number, idx):
    xyz = cloud[:, :3]
    d = np.sum((xyz[:, None, :] - xyz[None, :, :]) ** 2, -1)
    np.fill_diagonal(d, np.inf)
    return bool((d > 1e10).all())


PROPERTIES = {
    "plain": lambda cloud, number, idx: True,
    # more iterations than points: every point taken, then repeats
    "repeat": lambda cloud, number, idx: number > len(cloud) and len(set(idx.tolist())) == len(cloud),
    # some iteration's maximum is held by more than one point (first holder != last holder)
    "ties": _has_tie,
    # a float32 cloud whose sequence changes when measured in float64
    "wide": lambda cloud, number, idx: cloud.dtype == np.float32 and _differs("wide")(cloud, number, idx),
    # a cloud whose sequence changes when the channel sum is contracted into fmas
    "fma": _differs("fma"),
    # every pairwise distance above the initial 1e10: no running distance but a centroid's own
    # is ever replaced
    "far": _all_far,
    # columns past the third exist and vary: they are carried into the result, never measured
    "columns": lambda cloud, number, idx: cloud.shape[1] > 3 and bool(np.ptp(cloud[:, 3:], axis=0).all()),
}

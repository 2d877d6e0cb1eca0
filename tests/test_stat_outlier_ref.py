"""tests/stat_outlier_ref.py -- the numpy restatement the GPU is compared with -- against a plain
Python-loop formulation of include/pn2.h S1 to S5, and the edge rules of S1, S4 and S5."""
import math

import numpy as np
import pytest

import collect_ref
import stat_outlier_ref as ref


def loop_means(pc, k):
    """S1-S3 one float64 operation at a time (Python floats are IEEE doubles; math.sqrt is
    correctly rounded)."""
    rows = [[float(np.float64(v)) for v in r[:3]] for r in pc]
    fin = [all(math.isfinite(v) for v in r) for r in rows]
    F = sum(fin)
    out = []
    for i, p in enumerate(rows):
        if not fin[i]:
            out.append(-1.0)
            continue
        d2 = []
        for j, c in enumerate(rows):
            if fin[j]:
                dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
                d2.append(((dx * dx) + (dy * dy)) + (dz * dz))
        k_eff = min(k, F)
        s = 0.0
        for v in sorted(d2)[:k_eff]:
            s = s + math.sqrt(v)
        out.append(s / float(k_eff))
    return out, F


def loop_stats(mean, std_ratio, F):
    s = 0.0
    for m in mean:
        if m > 0:
            s = s + m
    cloud_mean = s / F if F else math.nan
    q = 0.0
    for m in mean:
        q = q + ((m - cloud_mean) * (m - cloud_mean) if m > 0 else 0.0)
    std = math.sqrt(q / (F - 1)) if F > 1 else math.nan  # 0/0
    return [cloud_mean, std, cloud_mean + std_ratio * std, float(F)]


def with_bad_rows(pc):
    pc = np.array(pc)
    pc[3, 0], pc[10, 2], pc[11, 1] = np.nan, np.inf, -np.inf
    return pc


CLOUDS = {
    "uniform200": lambda dt: collect_ref.uniform_cloud(200, seed=1, C=3, dtype=dt),
    "uniform97_c6": lambda dt: collect_ref.uniform_cloud(97, seed=2, C=6, dtype=dt),
    "lattice": lambda dt: collect_ref.lattice_cloud(side=5, dtype=dt),
    "copies": lambda dt: np.vstack([collect_ref.copies_cloud(30, dtype=dt), collect_ref.uniform_cloud(40, dtype=dt)]),
    "bad_rows": lambda dt: with_bad_rows(collect_ref.uniform_cloud(60, seed=3, dtype=dt)),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("k", [1, 7, 30, 500])
def test_restatement_against_the_loop(name, k, dtype):
    pc = CLOUDS[name](dtype)
    assert len(pc) <= 200
    want, F = loop_means(pc, k)
    got = ref.knn_mean_distance(pc, k)
    assert got.dtype == np.float64 and ref.same_bits(got, want)
    for ratio in (0.1, 2.0):
        stats = loop_stats(want, ratio, F)
        assert ref.same_bits(ref.statistics(got, ratio), stats)
        keep = np.array([m > 0 and m < stats[2] for m in want], dtype=bool)
        assert np.array_equal(ref.keep_mask(got, ratio), keep)
        assert np.array_equal(ref.delet_outlier_statistical(pc, k, ratio), pc[keep])
    if name == "uniform200" and k in (7, 30):
        assert 0 < ref.keep_mask(got, 0.1).sum() < len(pc)


def test_chain_sum_is_left_to_right():
    v = np.array([1.0] + [2.0 ** -53] * 1000)  # each small term alone is rounded away
    s = 0.0
    for x in v.tolist():
        s = s + x
    assert s == 1.0 and ref.chain_sum(v) == s and np.sum(v) > s  # the pairwise sum keeps them
    assert ref.chain_sum(np.zeros(0)) == 0.0


def test_k_above_n_takes_every_row():
    pc = collect_ref.uniform_cloud(50, seed=4)
    assert ref.same_bits(ref.knn_mean_distance(pc, 51), ref.knn_mean_distance(pc, 50))
    assert ref.same_bits(ref.knn_mean_distance(pc, 10 ** 6), ref.knn_mean_distance(pc, 50))
    assert not ref.same_bits(ref.knn_mean_distance(pc, 49), ref.knn_mean_distance(pc, 50))


def test_k_one_keeps_nothing():
    pc = collect_ref.uniform_cloud(50, seed=5)
    mean = ref.knn_mean_distance(pc, 1)
    assert (mean == 0).all()  # every row's nearest row is itself
    assert len(ref.delet_outlier_statistical(pc, 1, 5.0)) == 0


def test_one_valid_row_keeps_nothing():
    pc = np.full((6, 3), np.nan)
    pc[4] = [1.0, 2.0, 3.0]
    mean = ref.knn_mean_distance(pc, 3)
    assert mean.tolist() == [-1, -1, -1, -1, 0, -1]
    stats = ref.statistics(mean, 1.0)
    assert stats[0] == 0 and np.isnan(stats[1]) and np.isnan(stats[2]) and stats[3] == 1
    assert len(ref.delet_outlier_statistical(pc, 3, 1.0)) == 0
    # and two valid rows at the same place: mean 0 both, nothing kept either
    pc[1] = pc[4]
    assert len(ref.delet_outlier_statistical(pc, 3, 1.0)) == 0
    # no valid row, no row
    assert len(ref.delet_outlier_statistical(np.full((4, 3), np.inf), 3, 1.0)) == 0
    assert ref.delet_outlier_statistical(np.zeros((0, 6)), 3, 1.0).shape == (0, 6)


def test_nan_rows_are_dropped_and_never_counted():
    clean = collect_ref.uniform_cloud(80, seed=6, C=6)
    dirty = np.insert(clean, [0, 17, 17, 80], np.nan, axis=0)
    dirty[0, 3:] = 0.5  # non-finite in the coordinates only counts
    dirty[18, :2] = [np.inf, 0.0]
    bad = ~ref.finite_rows(dirty)
    assert bad.sum() == 4
    for k in (5, 200):
        mean = ref.knn_mean_distance(dirty, k)
        assert (mean[bad] == -1).all() and ref.same_bits(mean[~bad], ref.knn_mean_distance(clean, k))
        assert ref.same_bits(ref.statistics(mean, 1.5), ref.statistics(ref.knn_mean_distance(clean, k), 1.5))
        assert np.array_equal(ref.delet_outlier_statistical(dirty, k, 1.5), ref.delet_outlier_statistical(clean, k, 1.5))
    # a NaN in a colour column is not a coordinate: the row is kept or dropped like any other
    colour = np.array(clean)
    colour[5, 4] = np.nan
    assert np.array_equal(ref.keep_mask(ref.knn_mean_distance(colour, 5), 1.5),
                          ref.keep_mask(ref.knn_mean_distance(clean, 5), 1.5))


def test_a_blob_loses_exactly_its_far_points():
    rng = np.random.RandomState(7)
    blob = collect_ref.blob(rng, [0, 0, 1], 300, 0.05)
    far = rng.uniform(3, 9, (5, 3)) * rng.choice([-1, 1], (5, 3))
    pc = np.vstack([blob, far])
    order = rng.permutation(305)
    pc = pc[order]
    got = ref.delet_outlier_statistical(pc, 20, 2.0)
    want = pc[order < 300]
    assert len(got) == 300 and np.array_equal(got, want)


def test_arguments():
    pc = collect_ref.uniform_cloud(10)
    for k, r in ((0, 1.0), (-1, 1.0), (3, 0.0), (3, -2.0)):
        with pytest.raises(ValueError):
            ref.delet_outlier_statistical(pc, k, r)

"""pn2.collect.knn_mean_distance / delet_outlier_statistical (csrc/knn.hip) against the numpy
restatement tests/stat_outlier_ref.py: the mean distances (as int64), the four statistics and the
kept rows bit for bit.  (A NaN statistic equals a NaN: stat_outlier_ref.same_bits.)"""
import functools

import numpy as np
import pytest
import torch

import collect_ref
import stat_outlier_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def _collect():
    from pn2 import collect
    return collect


def _kmax():
    from pn2 import _lib
    return int(_lib.load().pn2_knn_max_k())


@functools.lru_cache(maxsize=None)
def _uniform(N, C, dtype):
    pc = collect_ref.uniform_cloud(N, seed=N % 97, C=C, dtype=dtype)
    pc.setflags(write=False)
    return pc


def check(pc, k, ratio=1.0):
    """-> (mean, kept) of the GPU after comparing mean, flags, stats and kept rows with the rule."""
    c = _collect()
    want = ref.knn_mean_distance(pc, k)
    mean = c.knn_mean_distance(pc, k)
    assert isinstance(mean, np.ndarray) and mean.dtype == np.float64 and mean.shape == (len(pc),)
    assert ref.same_bits(mean, want), np.flatnonzero(mean.view(np.int64) != want.view(np.int64))[:8]
    assert mean.tobytes() == c.knn_mean_distance(pc, k).tobytes()  # two runs, the same bits
    flags, stats = c._stat_flags(torch.from_numpy(mean).cuda(), ratio)
    assert ref.same_bits(stats.cpu().numpy(), ref.statistics(want, ratio)), (stats, ref.statistics(want, ratio))
    keep = ref.keep_mask(want, ratio)
    assert np.array_equal(flags.cpu().numpy(), keep.astype(np.int32))
    kept = c.delet_outlier_statistical(pc, k, ratio)
    assert isinstance(kept, np.ndarray) and kept.dtype == pc.dtype
    assert kept.shape == (int(keep.sum()), pc.shape[1]) and np.array_equal(kept, pc[keep])
    return mean, kept


# ------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,k", [(1, 4), (2, 4), (63, 4), (64, 4), (65, 4),  # smallest sizes, wave boundaries
                                 (119, 120), (120, 120), (121, 120),          # k_eff = N, the first full selection
                                 (1025, 120), (2500, 120),                    # candidate tiles, many refills
                                 (600, 1), (600, 2), (600, None)])            # smallest and largest k
def test_sizes(N, k, dtype):
    k = _kmax() if k is None else k
    pc = _uniform(N, 6 if N == 1025 else 3, dtype)
    mean, kept = check(pc, k)
    if k == 1:
        assert (mean == 0).all() and len(kept) == 0
    elif N >= 63:
        assert 0 < len(kept) < N


# ---------------------------------------------------------------------------- ties, duplicates
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [2, 4, 7, 20, 120])
def test_lattice_ties_at_the_kth_place(k, dtype):
    pc = collect_ref.lattice_cloud(dtype=dtype)  # 343 points, every d2 exact: 6, 12, 8 ... rows tie
    mean, _ = check(pc, k, 0.5)
    if k == 2:
        assert (mean == 0.0625).all()  # (0 + 0.125) / 2 at every point


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_copies_have_mean_zero_and_go(dtype):
    pc = np.vstack([collect_ref.copies_cloud(300, C=4, dtype=dtype), collect_ref.uniform_cloud(150, C=4, dtype=dtype)])
    pc = pc[np.random.RandomState(8).permutation(len(pc))]
    copy = (pc[:, :3] == pc[np.flatnonzero(pc[:, 1] < 0)[0], :3]).all(1)
    assert copy.sum() == 300
    for k in (120, 256):
        mean, kept = check(pc, k, 3.0)
        assert (mean[copy] == 0).all() and (mean[~copy] > 0).all()
        assert 0 < len(kept) <= 150 and (kept[:, 1] >= 0).all()  # no copy survives
    check(collect_ref.copies_cloud(130, dtype=dtype), 120)  # nothing but copies: every mean 0


# ------------------------------------------------------------------------ presentation order
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sorted_along_x_and_shuffled(dtype):
    """Sorted, every step brings nearer candidates than the bound for half the sweep; the
    selection must not depend on the order, so each point's own mean is the same."""
    pc = np.array(_uniform(1500, 3, dtype))
    pc = pc[np.argsort(pc[:, 0], kind="stable")]
    perm = np.random.RandomState(9).permutation(len(pc))
    for k in (16, 120):
        m_sorted, _ = check(pc, k)
        m_rev, _ = check(pc[::-1].copy(), k)
        m_shuffled, _ = check(pc[perm], k)
        assert m_shuffled.tobytes() == m_sorted[perm].tobytes() and m_rev.tobytes() == m_sorted[::-1].tobytes()


# ----------------------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_and_inf_rows(dtype):
    clean = _uniform(700, 6, dtype)
    pc = np.insert(clean, [0, 63, 64, 64, 300, 700], 0.5, axis=0)
    bad = np.flatnonzero(~(pc[:, :3] != 0.5).any(1))
    assert len(bad) == 6
    for n, (col, v) in zip(bad, [(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (2, np.nan), (1, np.nan)]):
        pc[n, col] = v
    pc[bad[3], :3] = np.nan
    pc[5, 4] = np.nan  # a colour, not a coordinate
    for k in (4, 120):
        mean, kept = check(pc[:, :3], k)
        assert (mean[bad] == -1).all() and (np.delete(mean, bad) > 0).all()
        assert np.delete(mean, bad).tobytes() == _collect().knn_mean_distance(clean, k).tobytes()
        assert np.isfinite(kept).all()
    c = _collect()
    got = c.delet_outlier_statistical(pc, 120, 1.0)  # array_equal is no use on a NaN colour
    want = ref.delet_outlier_statistical(pc, 120, 1.0)
    assert got.tobytes() == want.tobytes() and np.isnan(got[:, 4]).sum() == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exactly_one_finite_row(dtype):
    pc = np.full((130, 3), np.nan, dtype=dtype)
    pc[::2, 0], pc[1::2, 2] = 1.0, np.inf
    pc[77] = [1.0, 2.0, 3.0]
    mean, kept = check(pc, 4)  # valid == 1: cloud_mean 0, std and threshold NaN, nothing kept
    assert mean[77] == 0 and (np.delete(mean, 77) == -1).all() and len(kept) == 0
    mean, kept = check(np.full((70, 3), np.nan, dtype=dtype), 4)  # and none at all
    assert (mean == -1).all() and len(kept) == 0


def test_distances_that_overflow():
    """Finite rows whose d2 overflows to +inf are candidates like any other (S1 asks for finite
    coordinates, not finite distances)."""
    pc = np.array(_uniform(100, 3, np.float64))
    pc[:10] *= 1e200
    c = _collect()
    for k in (4, 120):
        want = ref.knn_mean_distance(pc, k)
        assert np.isinf(want).sum() == (10 if k == 4 else 100)  # 90 rows lie within a finite distance
        assert ref.same_bits(c.knn_mean_distance(pc, k), want)


@pytest.mark.parametrize("N", [1, 2047, 2048, 2049, 4097, 9000])
def test_statistics_on_given_means(N):
    """pn2_stat_outlier_flags alone, on means it is handed: whole staged chunks of 2048, one more,
    and both halves of the staging buffer used again; -1 and 0 entries never add."""
    rng = np.random.RandomState(N)
    mean = rng.uniform(0.01, 0.02, N) * rng.choice([1.0, 1.0, 1.0, 8.0], N)
    mean[rng.rand(N) < 0.05] = -1.0
    mean[rng.rand(N) < 0.05] = 0.0
    for ratio in (0.1, 1.0):
        flags, stats = _collect()._stat_flags(torch.from_numpy(mean).cuda(), ratio)
        assert ref.same_bits(stats.cpu().numpy(), ref.statistics(mean, ratio))
        assert np.array_equal(flags.cpu().numpy(), ref.keep_mask(mean, ratio).astype(np.int32))


# ------------------------------------------------------------------------ layouts, return types
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padded_rows_and_tensors(dtype):
    c = _collect()
    pc = _uniform(1000, 6, dtype)
    want_mean = ref.knn_mean_distance(pc, 30)
    want = ref.delet_outlier_statistical(pc, 30, 1.0)
    assert 0 < len(want) < len(pc)
    wide = torch.zeros(1000, 8, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    wide[:, :6] = torch.from_numpy(np.array(pc)).cuda()
    view = wide[:, :6]  # C = 6, ld = 8
    assert view.stride() == (8, 1)
    mean = c.knn_mean_distance(view, 30)
    assert isinstance(mean, torch.Tensor) and mean.is_cuda and mean.dtype == torch.float64
    assert ref.same_bits(mean.cpu().numpy(), want_mean)
    got = c.delet_outlier_statistical(view, 30, 1.0)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == view.dtype
    assert np.array_equal(got.cpu().numpy(), want)
    host = c.delet_outlier_statistical(torch.from_numpy(np.array(pc)), 30, 1.0)  # a host tensor: a tensor back
    assert isinstance(host, torch.Tensor) and np.array_equal(host.cpu().numpy(), want)
    assert np.array_equal(c.delet_outlier_statistical(pc, 30, 1.0), want)  # an array: an array back
    assert c.delet_outlier_statistical(np.zeros((0, 6), dtype=dtype)).shape == (0, 6)
    assert c.knn_mean_distance(np.zeros((0, 3), dtype=dtype), 5).shape == (0,)


# --------------------------------------------------------------------------------- end to end
def test_defaults_on_two_blobs_and_noise():
    import collect
    rng = np.random.RandomState(10)
    parts = [collect_ref.blob(rng, [0, 0, 1], 1700, 0.06), collect_ref.blob(rng, [0.5, 0, 1.2], 1200, 0.05)]
    noise = rng.uniform(-3, 3, (100, 3))
    noise = noise[np.abs(noise - [0.25, 0, 1.1]).max(1) > 1.0]
    xyz = np.vstack(parts + [noise[:100]])
    marked = np.hstack([xyz, np.zeros((len(xyz), 3))])
    marked[2900:, 3] = 1.0  # the noise rows carry a mark through the filter
    pc = marked[rng.permutation(len(marked))]
    assert len(pc) >= 2950
    got = collect.delet_outlier_statistical(pc)  # nb_neighbors = 120, std_ratio = 0.1
    want = ref.delet_outlier_statistical(pc)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert 0 < len(got) <= 2900 and (got[:, 3] == 0).all()  # the noise is among the rows removed
    check(pc, 120, 0.1)

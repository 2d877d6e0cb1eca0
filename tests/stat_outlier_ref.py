"""delet_outlier_statistical restated in numpy (include/pn2.h, "statistical outlier removal", S1 to
S5): Open3D's RemoveStatisticalOutliers with the kd-tree written out as exact arithmetic.

Every sum is np.cumsum(...)[-1], a left-to-right float64 chain; np.sum adds pairwise and must not
be used.  np.sqrt and the float64 division are correctly rounded, one operation each."""
import numpy as np

SLAB = 256  # query rows per [SLAB, F] block of d2: the arithmetic does not depend on it


def finite_rows(point_cloud):
    """S1: the rows whose three coordinates are finite."""
    return np.isfinite(point_cloud[:, :3].astype(np.float64)).all(1)


def d2_rows(xyz, rows):
    """S2, collect_ref.neighbour_matrix's arithmetic without the compare: d2 of the given query rows
    to every row, every operation a numpy ufunc of its own."""
    d = xyz[rows, None, :] - xyz[None, :, :]
    s = d * d
    return (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]


def chain_sum(values):
    """A left-to-right float64 chain from 0.0 (0.0 + v0 == v0 for every v0 >= 0)."""
    return np.cumsum(values, dtype=np.float64)[-1] if len(values) else np.float64(0.0)


def knn_mean_distance(point_cloud, nb_neighbors):
    """S3: float64 [N], -1.0 for a non-finite row."""
    k = int(nb_neighbors)
    assert k >= 1
    fin = finite_rows(point_cloud)
    xyz = point_cloud[fin, :3].astype(np.float64)
    F = len(xyz)
    k_eff = min(k, F)
    means = np.empty(F, dtype=np.float64)
    with np.errstate(over="ignore"):
        for r in range(0, F, SLAB):
            near = np.sort(d2_rows(xyz, slice(r, r + SLAB)), axis=1)[:, :k_eff]
            means[r:r + SLAB] = np.cumsum(np.sqrt(near), axis=1, dtype=np.float64)[:, -1] / np.float64(k_eff)
    out = np.full(len(point_cloud), -1.0, dtype=np.float64)
    out[fin] = means
    return out


def statistics(mean, std_ratio):
    """S4: float64 [4] = cloud_mean, std, threshold, valid."""
    mean = np.asarray(mean, dtype=np.float64)
    valid = np.float64(np.count_nonzero(mean >= 0))  # a non-finite row carries -1
    pos = mean > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cloud_mean = chain_sum(mean[pos]) / valid
        dev = mean - cloud_mean
        sq_sum = chain_sum(np.where(pos, dev * dev, 0.0))
        std = np.sqrt(sq_sum / (valid - np.float64(1.0)))
        threshold = cloud_mean + np.float64(std_ratio) * std
    return np.array([cloud_mean, std, threshold, valid], dtype=np.float64)


def keep_mask(mean, std_ratio):
    """S5."""
    mean = np.asarray(mean, dtype=np.float64)
    if len(mean) == 0:
        return np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore"):
        return (mean > 0) & (mean < statistics(mean, std_ratio)[2])


def delet_outlier_statistical(point_cloud, nb_neighbors=120, std_ratio=0.1):
    if nb_neighbors < 1 or not std_ratio > 0:
        raise ValueError("nb_neighbors must be >= 1 and std_ratio > 0")
    return point_cloud[keep_mask(knn_mean_distance(point_cloud, nb_neighbors), std_ratio)]


def same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN: 0/0 has no one sign or payload (x86 gives
    the negative quiet NaN, the GPU the positive)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))

"""delete_plane / segment_plane restated in numpy (include/pn2.h, "plane segmentation", P1 to P7):
Open3D's RANSAC segment_plane with the draws made an input and everything after them written out
as exact float64 arithmetic.

Every sum is a left-to-right float64 chain from 0.0, written np.cumsum(...)[-1] over the values
with 0.0 put in front (0.0 + -0.0 is +0.0: the start matters for the sign of a zero); np.sum adds
pairwise and must not be used.  Every product, sum, difference, division and square root is a
numpy ufunc of its own: rounded once, nothing contracted."""
import numpy as np

CHUNK = 1024  # PN2_PLANE_CHUNK: P4's and P7's sums are chains within a chunk, then over the chunks


def chain_rows(values):
    """[R, L] -> [R]: each row one chain from 0.0."""
    values = np.asarray(values, dtype=np.float64)
    return np.cumsum(np.concatenate([np.zeros((len(values), 1)), values], axis=1), axis=1, dtype=np.float64)[:, -1]


def chain_sum(values):
    return chain_rows(np.asarray(values, dtype=np.float64)[None, :])[0]


def xyz_of(point_cloud):
    return np.asarray(point_cloud)[:, :3].astype(np.float64)


def draw_samples(N, ransac_n, num_iterations):
    """P1: the one draw of the default path, from numpy's global generator."""
    return np.random.randint(0, N, size=(num_iterations, ransac_n))


# ------------------------------------------------------------------------------ P2 / P3
def _normalised(a, b, c, q):
    """The norm, the zero test and the normalisation; q [M, 3] the point d is taken at.
    -> (planes [M, 4], zero [M])"""
    norm = np.sqrt((a * a + b * b) + c * c)
    zero = norm == 0
    a, b, c = a / norm, b / norm, c / norm
    d = -((a * q[:, 0] + b * q[:, 1]) + c * q[:, 2])
    planes = np.stack([a, b, c, d], 1)
    planes[zero] = 0.0
    return planes, zero


def planes_of_moments(xx, xy, xz, yy, yz, zz, centroid):
    """P2 after the sums: arrays [M], centroid [M, 3] -> (planes [M, 4], zero [M])"""
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    first = (det_x > det_y) & (det_x > det_z)
    second = ~first & (det_y > det_z)
    a = np.where(first, det_x, np.where(second, xz * yz - xy * zz, xy * yz - xz * yy))
    b = np.where(first, xz * yz - xy * zz, np.where(second, det_y, xy * xz - yz * xx))
    c = np.where(first, xy * yz - xz * yy, np.where(second, xy * xz - yz * xx, det_z))
    return _normalised(a, b, c, centroid)


def hypotheses(xyz, samples):
    """P1-P3 -> (planes float64 [M, 4], skipped bool [M]); a skipped row (an index outside [0, N),
    or a zero plane) carries the zero plane."""
    samples = np.asarray(samples)
    M, n = samples.shape
    bad = ((samples < 0) | (samples >= len(xyz))).any(1)
    p = xyz[np.where(bad[:, None], 0, samples)]  # [M, n, 3]; what a bad row gathers is never used
    with np.errstate(all="ignore"):
        if n == 3:
            e0, e1 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
            planes, zero = _normalised(e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1],
                                       e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                                       e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0], p[:, 0])
        else:
            centroid = np.stack([chain_rows(p[:, :, k]) for k in range(3)], 1) / np.float64(n)
            r = p - centroid[:, None, :]
            moments = [chain_rows(r[:, :, i] * r[:, :, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
            planes, zero = planes_of_moments(*moments, centroid)
    planes[bad] = 0.0
    return planes, bad | zero


# ----------------------------------------------------------------------------------- P4
def distances(xyz, planes):
    """[M, L] for the L rows given."""
    a, b, c, d = (planes[:, k, None] for k in range(4))
    with np.errstate(all="ignore"):
        return np.abs(((a * xyz[None, :, 0] + b * xyz[None, :, 1]) + c * xyz[None, :, 2]) + d)


def score(xyz, planes, skipped, distance_threshold):
    """-> (count int32 [M], err float64 [M]).  A row that is no inlier adds +0.0 to its chunk's
    chain, which leaves it as it is: a chain of distances (>= 0) from +0.0 is never -0.0."""
    M = len(planes)
    count, err = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.float64)
    thr = np.float64(distance_threshold)
    for c0 in range(0, len(xyz), CHUNK):
        dist = distances(xyz[c0:c0 + CHUNK], planes)
        with np.errstate(invalid="ignore"):
            inlier = (dist < thr) & ~skipped[:, None]  # a NaN fails; a skipped plane is not scored
        count += inlier.sum(1)
        err = err + chain_rows(np.where(inlier, dist, 0.0))  # the chunk sums, one chain over the chunks
    return count.astype(np.int32), err


# ----------------------------------------------------------------------------------- P5
def best(planes, count, err):
    """-> float64 [8] = a, b, c, d, index, count, err, 0"""
    bc, be, bi = 0, np.float64(0.0), -1
    for m in range(len(count)):
        if count[m] > bc or (count[m] == bc and err[m] < be):
            bc, be, bi = int(count[m]), err[m], m
    plane = planes[bi] if bi >= 0 else np.zeros(4)
    return np.array(list(plane) + [bi, bc, be, 0.0], dtype=np.float64)


# ----------------------------------------------------------------------------------- P6
def inlier_flags(xyz, result, distance_threshold):
    if result[4] < 0:
        return np.zeros(len(xyz), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        return (distances(xyz, result[None, :4])[0] < np.float64(distance_threshold)).astype(np.int32)


def segment(point_cloud, samples, distance_threshold):
    """P1-P6 -> dict of every stage: planes, count, err, result, flags."""
    xyz = xyz_of(point_cloud)
    planes, skipped = hypotheses(xyz, samples)
    count, err = score(xyz, planes, skipped, distance_threshold)
    result = best(planes, count, err)
    return dict(planes=planes, count=count, err=err, result=result,
                flags=inlier_flags(xyz, result, distance_threshold))


# ----------------------------------------------------------------------------------- P7
def chunked_sum(values, flagged):
    """The flagged values: one chain per chunk in ascending index, the chunk sums one chain."""
    total = np.float64(0.0)
    for c0 in range(0, len(values), CHUNK):
        total = total + chain_sum(values[c0:c0 + CHUNK][flagged[c0:c0 + CHUNK]])
    return total


def refit(point_cloud, flags):
    """-> float64 [4]"""
    xyz = xyz_of(point_cloud)
    flagged = np.asarray(flags) != 0
    n = np.float64(np.count_nonzero(flagged))
    if n == 0:
        return np.zeros(4)
    with np.errstate(all="ignore"):
        centroid = np.array([chunked_sum(xyz[:, k], flagged) for k in range(3)]) / n
        r = xyz - centroid[None, :]
        moments = [np.array([chunked_sum(r[:, i] * r[:, j], flagged)])
                   for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        return planes_of_moments(*moments, centroid[None, :])[0][0]


# ------------------------------------------------------------------------ the two functions
def _check(N, distance_threshold, ransac_n, num_iterations):
    if ransac_n < 3 or N < ransac_n or num_iterations < 1 or not 0 < distance_threshold < np.inf:
        raise ValueError("ransac_n >= 3, N >= ransac_n, num_iterations >= 1, a finite distance_threshold > 0")


def segment_plane(point_cloud, distance_threshold, ransac_n, num_iterations, samples=None):
    """-> (plane_model float64 [4], inliers int64 [K] ascending)"""
    _check(len(point_cloud), distance_threshold, ransac_n, num_iterations)
    if samples is None:
        samples = draw_samples(len(point_cloud), ransac_n, num_iterations)
    flags = segment(point_cloud, samples, distance_threshold)["flags"]
    return refit(point_cloud, flags), np.flatnonzero(flags).astype(np.int64)


def delete_plane(point_cloud, distance_threshold=0.006, ransac_n=20, num_iterations=1000, samples=None):
    _check(len(point_cloud), distance_threshold, ransac_n, num_iterations)
    if samples is None:
        samples = draw_samples(len(point_cloud), ransac_n, num_iterations)
    return point_cloud[segment(point_cloud, samples, distance_threshold)["flags"] == 0]


# --------------------------------------------------------------------------------- fixtures
def table_cloud():
    """A 0.6 x 0.6 table 4 mm thick at z = 0.8 (3000 points) and two boxes above it (500 and 400
    points), shuffled: float64 [3900, 3].  is_table() tells the rows apart."""
    rng = np.random.RandomState(0)
    table = np.stack([rng.uniform(-.3, .3, 3000), rng.uniform(-.3, .3, 3000), 0.8 + rng.uniform(-.002, .002, 3000)], 1)
    box1 = rng.uniform(0, .08, (500, 3)) + [0, 0, .70]
    box2 = rng.uniform(0, .06, (400, 3)) + [-.2, .1, .72]
    pc = np.vstack([table, box1, box2])
    return pc[rng.permutation(len(pc))]


def is_table(point_cloud):
    return np.asarray(point_cloud)[:, 2] > 0.79  # the boxes end at z = 0.78, the table starts at 0.798


# P1 tables for a cloud whose rows 0, 1, 2 are collinear and 0, 1, 3 are not (degenerate_cloud)
def degenerate_cloud(dtype=np.float64):
    """Rows 0..2 on one line, row 3 off it, then twelve rows of a square grid in the plane z = 1."""
    g = np.stack(np.meshgrid(np.arange(4) * 0.25, np.arange(3) * 0.25), -1).reshape(-1, 2)
    xyz = np.vstack([[[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1], [0, 1, 0.25]], np.hstack([g, np.ones((12, 1))])])
    return xyz.astype(dtype)


DEGENERATE_N3 = np.array([[0, 1, 2],      # collinear: zero plane, skipped
                          [5, 5, 5],      # one index three times: zero plane, skipped
                          [4, 5, 8],      # the grid's plane z = 1
                          [2, 1, 0]])     # collinear again
DEGENERATE_N4 = np.array([[0, 1, 2, 2],   # collinear with a duplicate: rank 1, zero plane
                          [4, 5, 8, 8],   # a duplicate inside the row counts twice: still z = 1
                          [7, 7, 7, 7]])  # one index four times: every moment 0
ALL_ZERO_N3 = np.array([[0, 1, 2], [3, 3, 3], [2, 0, 1], [1, 1, 0]])

"""The camera-cloud front end restated in numpy (include/pn2.h, "camera-cloud front end", rules
1 to 5): clip_distance, delet_outlier_radius, dbscan_labels and cluster_point of
point_collect/collect.py, with Open3D's radius search and DBSCAN written out.

dbscan_labels is the SEQUENTIAL algorithm -- points visited in index order, a cluster grown
breadth first from each unvisited core point, a noise point claimed by the first cluster that
reaches it -- not rule 4's closed form, which is labels_closed_form below: the tests check that
the two agree, and the GPU against the first.

FIXTURES are the clouds tests/test_gpu_collect.py runs, built here so that the CPU test can check
them too.  Every fixture is seeded and its point order shuffled: the smallest index of a cluster
means nothing spatially."""
import collections

import numpy as np

import downsample_ref


# ------------------------------------------------------------------------------------ rules
def clip_distance(point_cloud, dis=(0, 2), axis=2):
    """Rule 1, as the reference's two np.where passes."""
    point_cloud = point_cloud[np.where(point_cloud[:, axis] >= dis[0])]
    return point_cloud[np.where(point_cloud[:, axis] <= dis[1])]


def neighbour_matrix(point_cloud, radius, rows=slice(None)):
    """Rule 2: [N, N] bool (or the given rows of it), d2 = ((dx*dx) + (dy*dy)) + (dz*dz) < r*r in
    float64, every operation a numpy ufunc of its own (rounded once, nothing contracted)."""
    xyz = point_cloud[:, :3].astype(np.float64)
    d = xyz[rows, None, :] - xyz[None, :, :]
    s = d * d
    d2 = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
    r = np.float64(radius)
    return d2 < r * r


def radius_counts(point_cloud, radius):
    return neighbour_matrix(point_cloud, radius).sum(1).astype(np.int32)


def delet_outlier_radius(point_cloud, nb_points=200, radius=0.05):
    """Rule 3."""
    return point_cloud[radius_counts(point_cloud, radius) > nb_points]


def dbscan_labels(point_cloud, eps, min_points):
    """Rule 4 as the sequential visit-order algorithm."""
    nbr = neighbour_matrix(point_cloud, eps)
    N = len(point_cloud)
    UNVISITED, NOISE = -2, -1
    labels = np.full(N, UNVISITED, dtype=np.int32)
    cluster = 0
    for i in range(N):
        if labels[i] != UNVISITED:
            continue
        mine = np.flatnonzero(nbr[i])
        if len(mine) < min_points:
            labels[i] = NOISE
            continue
        labels[i] = cluster
        queue = collections.deque(mine.tolist())
        seen = set(mine.tolist())
        while queue:
            j = queue.popleft()
            if labels[j] == NOISE:
                labels[j] = cluster  # a border point: claimed, never expanded
            if labels[j] != UNVISITED:
                continue
            labels[j] = cluster
            theirs = np.flatnonzero(nbr[j])
            if len(theirs) >= min_points:
                for k in theirs.tolist():
                    if k not in seen:
                        seen.add(k)
                        queue.append(k)
        cluster += 1
    return labels


def labels_closed_form(point_cloud, eps, min_points):
    """Rule 4 as stated: components of core points, numbered by smallest core index; a non-core
    point takes the smallest label among its core neighbours."""
    nbr = neighbour_matrix(point_cloud, eps)
    N = len(point_cloud)
    core = nbr.sum(1) >= min_points
    comp = np.arange(N)
    changed = True
    while changed:  # min-label propagation over core-core edges to a fixed point
        changed = False
        for i in np.flatnonzero(core):
            m = comp[np.flatnonzero(nbr[i] & core)].min()
            if m < comp[i]:
                comp[i] = m
                changed = True
    roots = sorted(set(comp[core].tolist()))
    rank = {r: l for l, r in enumerate(roots)}
    labels = np.full(N, -1, dtype=np.int32)
    for i in range(N):
        if core[i]:
            labels[i] = rank[comp[i]]
        else:
            cn = np.flatnonzero(nbr[i] & core)
            if len(cn):
                labels[i] = min(rank[comp[j]] for j in cn)
    return labels


def cluster_point(point_cloud, eps=0.03, min_points=500):
    """Rule 5, in the reference's own order of operations."""
    label = dbscan_labels(point_cloud, eps, min_points)
    number_label = np.max(label) if len(label) else -1
    if number_label == -1:
        print('Null point')
        return None
    point_class = [np.where(label == i) for i in range(number_label + 1)]
    min_number = min(len(t[0]) for t in point_class)
    cluster = np.zeros((number_label + 1, min_number, point_cloud.shape[1]))
    for i in range(number_label + 1):
        point = point_cloud[point_class[i], :].squeeze()
        if point.ndim != 2:
            raise ValueError("not enough values to unpack (expected 2, got 1)")
        cluster[i, :, :] = downsample_ref.farthest_point_sample(point, min_number)
    return cluster


# --------------------------------------------------------------------------------- fixtures
def _finish(xyz, seed, C, dtype):
    """Shuffle the order, append C - 3 varying columns, cast."""
    rng = np.random.RandomState(seed)
    xyz = np.asarray(xyz, dtype=np.float64)[rng.permutation(len(xyz))]
    extra = rng.uniform(0, 1, (len(xyz), C - 3))
    return np.hstack([xyz, extra]).astype(dtype)


def blob(rng, centre, n, spread):
    return np.asarray(centre) + rng.uniform(-spread, spread, (n, 3))


def uniform_cloud(N, seed=0, C=3, dtype=np.float64):
    rng = np.random.RandomState(1000 + seed)
    return _finish(rng.uniform(0, 1, (N, 3)), seed, C, dtype)


def lattice_cloud(side=7, r=0.125, seed=1, C=3, dtype=np.float64):
    """Spacing exactly r (a power of two: every coordinate and d2 exact), so every axis
    neighbour sits ON the boundary d2 == r*r."""
    g = np.arange(side) * r
    return _finish(np.stack(np.meshgrid(g, g, g), -1).reshape(-1, 3), seed, C, dtype)


def copies_cloud(n=300, seed=2, C=3, dtype=np.float64):
    return _finish(np.tile([[0.3, -0.7, 1.1]], (n, 1)), seed, C, dtype)


EPS = 0.1


def border_cloud(swap, seed=3, C=3, dtype=np.float64):
    """Two blobs of 40 points and one point between them that is within EPS of one core point of
    each and has too few neighbours to be core (min_points = 10)."""
    rng = np.random.RandomState(seed)
    a = blob(rng, [0, 0, 0], 40, 0.02)
    b = blob(rng, [0.17, 0, 0], 40, 0.02)
    a[0], b[0] = [0.0, 0, 0], [0.17, 0, 0]
    a[1:, 0] -= 0.05  # only a[0] / b[0] reach the middle point
    b[1:, 0] += 0.05
    xyz = np.vstack([a, b, [[0.085, 0, 0]]])
    if swap:  # mirrored in x under the same shuffle: the other blob now holds the smallest index
        xyz[:, 0] = 0.17 - xyz[:, 0]
    return _finish(xyz, seed, C, dtype)


def line_cloud(n=600, seed=4, C=3, dtype=np.float64):
    """Spacing 0.6 * EPS, min_points = 2: one cluster, carried link by link."""
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.arange(n) * (0.6 * EPS)
    return _finish(xyz, seed, C, dtype)


def five_cloud(seed=5, C=3, dtype=np.float64):
    """Five blobs of unequal size along x; the shuffle decides which holds the smallest index."""
    rng = np.random.RandomState(seed)
    parts = [blob(rng, [k * 1.0, 0, 0], 20 + 7 * k, 0.03) for k in range(5)]
    noise = rng.uniform(-5, -1, (15, 3))
    return _finish(np.vstack(parts + [noise]), seed, C, dtype)


def noise_cloud(n=200, seed=6, C=3, dtype=np.float64):
    rng = np.random.RandomState(seed)
    return _finish(rng.uniform(0, 100, (n, 3)), seed, C, dtype)


# name -> (builder(C, dtype), eps, min_points)
LABEL_FIXTURES = {
    "border": (lambda C, dt: border_cloud(False, C=C, dtype=dt), EPS, 10),
    "border_swapped": (lambda C, dt: border_cloud(True, C=C, dtype=dt), EPS, 10),
    "line": (lambda C, dt: line_cloud(C=C, dtype=dt), EPS, 2),
    "five": (lambda C, dt: five_cloud(C=C, dtype=dt), EPS, 10),
    "noise": (lambda C, dt: noise_cloud(C=C, dtype=dt), EPS, 3),
}

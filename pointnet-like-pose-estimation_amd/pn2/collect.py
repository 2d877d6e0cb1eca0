"""The camera-cloud front end of the reference's capture scripts on the GPU
(point_collect/collect.py:30-102, its copy colledt_data_structure/collect.py, and
camera_test/camera.py:131): a frame's cloud is cut to a depth range (clip_distance), cleaned of
sparse points (delet_outlier_radius) and split into objects that are FPS-sampled to a common size
(cluster_point); delet_outlier_statistical (collect.py:80-90) is the file's other outlier filter,
and delete_plane (collect.py:6-28) takes the table out between the clip and the filters.
The reference runs them as numpy masks and Open3D kd-tree and RANSAC calls on the host; here they
are the kernels of csrc/collect.hip, csrc/knn.hip and csrc/plane.hip plus the existing numpy-rule
FPS (csrc/fps_points.hip), by the rules include/pn2.h states.  Names, misspellings included,
defaults and return shapes are the reference's; the `visualize` flags are not carried.

Input is [N, C], 3 <= C <= 64, float64 or float32: a numpy array (the result is a numpy array) or a
torch tensor (the result is a tensor on the device it ran on), with the optional device= of
pn2.provider.farthest_point_sample_batch.  Rows are carried whole; distances use columns 0..2.
There is no CPU path."""
import numpy as np
import torch

from . import _lib
from .ops import _stream
from .provider import _DOWNSAMPLE_DTYPES, _pick_device


def _cloud(who, point_cloud, device):
    """-> (rows on the device with unit column stride, whether the input was a host array)"""
    host = not isinstance(point_cloud, torch.Tensor)
    if host:
        a = np.ascontiguousarray(np.asarray(point_cloud))
        point_cloud = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = point_cloud
    if t.dim() != 2:
        raise ValueError("pn2.collect.%s: point_cloud must be [N, C], got shape %s" % (who, tuple(t.shape)))
    if t.dtype not in _DOWNSAMPLE_DTYPES:
        raise TypeError("pn2.collect.%s: point_cloud must be float64 or float32, got %s" % (who, t.dtype))
    N, C = t.shape
    if C < 3 or C > 64:
        raise ValueError("pn2.collect.%s: needs 3 <= C <= 64, got C = %d" % (who, C))
    limit = _lib.load().pn2_collect_max_points()
    if N > limit:
        raise ValueError("pn2.collect.%s: %d points, above the %d the kernels take" % (who, N, limit))
    dev = _pick_device(who, t, device)
    t = t.to(dev, non_blocking=True)
    if N and (t.stride(1) != 1 or (N > 1 and t.stride(0) < C)):
        t = t.contiguous()
    return t, host


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _result(t, host):
    return t.cpu().numpy() if host else t


def _compact(t, keys, mode, thresh=0, L=1, src=None):
    """pn2_compact_rows -> (rows [N, C] of which the first offsets[L] are written, offsets [L+1]);
    src: an int32 [N] tensor that receives the kept rows' input indices (out_src)"""
    N, C = t.shape
    lib = _lib.load()
    with torch.cuda.device(t.device):
        out = torch.empty(N, C, dtype=t.dtype, device=t.device)
        offsets = torch.zeros(L + 1, dtype=torch.int64, device=t.device)
        need = lib.pn2_compact_rows_workspace_bytes(N, L)
        if need < 0:
            raise ValueError("pn2.collect: %d rows in %d buckets are more than one compaction takes" % (N, L))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=t.device)
        _lib.check(lib.pn2_compact_rows(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), keys.data_ptr(),
                                        mode, thresh, L, out.data_ptr(), None if src is None else src.data_ptr(),
                                        offsets.data_ptr(), ws.data_ptr(),
                                        need, _stream(out)), "pn2_compact_rows")
    return out, offsets


def _counts(t, radius):
    N, C = t.shape
    with torch.cuda.device(t.device):
        counts = torch.empty(N, dtype=torch.int32, device=t.device)
        _lib.check(_lib.load().pn2_radius_count_f64(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t),
                                                    float(radius), counts.data_ptr(), _stream(counts)),
                   "pn2_radius_count_f64")
    return counts


def _labels(t, eps, min_points):
    """-> (labels int32 [N], number of clusters as a device int64 [1]); no host read"""
    N, C = t.shape
    lib = _lib.load()
    counts = _counts(t, eps)
    with torch.cuda.device(t.device):
        labels = torch.empty(N, dtype=torch.int32, device=t.device)
        ncl = torch.zeros(1, dtype=torch.int64, device=t.device)
        need = lib.pn2_dbscan_labels_workspace_bytes(N)
        ws = torch.empty(need, dtype=torch.uint8, device=t.device)
        _lib.check(lib.pn2_dbscan_labels(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), float(eps),
                                         int(min_points), counts.data_ptr(), labels.data_ptr(), ncl.data_ptr(),
                                         ws.data_ptr(), need, _stream(labels)), "pn2_dbscan_labels")
    return labels, ncl


def _bound(x, dtype):
    """A bound as numpy's comparison sees it: a Python number takes the cloud's dtype, a numpy
    value promotes with it.  Either way it is exact in float64, where the kernel compares."""
    b = np.asarray(x)
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    b = b.astype(np_dtype if type(x) in (int, float) else np.result_type(np_dtype, b.dtype))
    return float(b)


def clip_distance(point_cloud, dis=[0, 2], axis=2, device=None):
    """Keep the rows with dis[0] <= point_cloud[:, axis] <= dis[1], in input order."""
    t, host = _cloud("clip_distance", point_cloud, device)
    N, C = t.shape
    axis = int(axis)
    if not -C <= axis < C:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (axis, C))
    if N == 0:
        return _result(t, host)
    with torch.cuda.device(t.device):
        flags = torch.empty(N, dtype=torch.int32, device=t.device)
        _lib.check(_lib.load().pn2_clip_flags(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), axis % C,
                                              _bound(dis[0], t.dtype), _bound(dis[1], t.dtype), flags.data_ptr(),
                                              _stream(flags)), "pn2_clip_flags")
    out, offsets = _compact(t, flags, _lib.COMPACT_FLAG_GT)
    return _result(out[:int(offsets[1].item())], host)  # the one host read: the result's length


def delet_outlier_radius(point_cloud, nb_points=200, radius=0.05, device=None):
    """Keep the rows with more than nb_points points (themselves included) within radius."""
    t, host = _cloud("delet_outlier_radius", point_cloud, device)
    if t.shape[0] == 0:
        return _result(t, host)
    out, offsets = _compact(t, _counts(t, radius), _lib.COMPACT_FLAG_GT, int(nb_points))
    return _result(out[:int(offsets[1].item())], host)


def dbscan_labels(point_cloud, eps, min_points, device=None):
    """The labels cluster_point uses (include/pn2.h rule 4): int32 [N], -1 for noise."""
    t, host = _cloud("dbscan_labels", point_cloud, device)
    if t.shape[0] == 0:
        return _result(torch.empty(0, dtype=torch.int32, device=t.device), host)
    return _result(_labels(t, eps, min_points)[0], host)


def cluster_point(point_cloud, eps=0.03, min_points=500, device=None):
    """DBSCAN, then every cluster FPS-sampled to the smallest cluster's size: [L, min_number, C]
    float64, or None (and the reference's printed line) when no cluster is found.  One
    np.random.randint(0, n_i) is drawn per cluster, in label order, from numpy's global
    generator.  The host reads the number of clusters and their sizes; the rest stays on the
    device."""
    from .provider import _fps_points_launch
    t, host = _cloud("cluster_point", point_cloud, device)
    N, C = t.shape
    L = 0
    if N:
        labels, ncl = _labels(t, eps, min_points)
        L = int(ncl.item())
    if L == 0:
        print('Null point')
        return None
    rows, offsets = _compact(t, labels, _lib.COMPACT_LABEL, 0, L)
    offsets = offsets.cpu().numpy()
    sizes = np.diff(offsets).tolist()
    starts = np.zeros(L, dtype=np.int64)
    for i, n in enumerate(sizes):
        if n == 1:  # the reference's squeeze() leaves a [C] vector that its FPS cannot unpack
            raise ValueError("not enough values to unpack (expected 2, got 1)")
        starts[i] = np.random.randint(0, n)
    min_number = min(sizes)
    _, out = _fps_points_launch(rows, C, C, offsets, starts, int(offsets[L]), max(sizes), min_number)
    return _result(out.double(), host)


def _neighbours(who, nb_neighbors):
    k = int(nb_neighbors)
    if k < 1:
        raise ValueError("pn2.collect.%s: nb_neighbors must be >= 1, got %d" % (who, k))
    limit = _lib.load().pn2_knn_max_k()
    if k > limit:
        raise ValueError("pn2.collect.%s: nb_neighbors = %d, above the %d the kernel takes" % (who, k, limit))
    return k


def _knn_mean(t, k):
    """pn2_knn_mean_dist_f64 -> float64 [N] (include/pn2.h S1-S3); no host read"""
    N, C = t.shape
    lib = _lib.load()
    with torch.cuda.device(t.device):
        mean = torch.empty(N, dtype=torch.float64, device=t.device)
        need = lib.pn2_knn_mean_dist_workspace_bytes(N, k)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=t.device)
        _lib.check(lib.pn2_knn_mean_dist_f64(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), k,
                                             mean.data_ptr(), ws.data_ptr(), need, _stream(mean)),
                   "pn2_knn_mean_dist_f64")
    return mean


def _stat_flags(mean, std_ratio):
    """pn2_stat_outlier_flags -> (flags int32 [N], stats float64 [4] = cloud_mean, std, threshold,
    valid), both on the device; no host read"""
    N = mean.shape[0]
    with torch.cuda.device(mean.device):
        flags = torch.empty(N, dtype=torch.int32, device=mean.device)
        stats = torch.empty(4, dtype=torch.float64, device=mean.device)
        _lib.check(_lib.load().pn2_stat_outlier_flags(mean.data_ptr(), N, float(std_ratio), flags.data_ptr(),
                                                      stats.data_ptr(), _stream(flags)), "pn2_stat_outlier_flags")
    return flags, stats


def knn_mean_distance(point_cloud, nb_neighbors, device=None):
    """The mean distances delet_outlier_statistical thresholds (include/pn2.h S3): float64 [N], the
    mean distance from each row to its nb_neighbors nearest rows, itself included; -1 for a row
    with a non-finite coordinate."""
    k = _neighbours("knn_mean_distance", nb_neighbors)
    t, host = _cloud("knn_mean_distance", point_cloud, device)
    if t.shape[0] == 0:
        return _result(torch.empty(0, dtype=torch.float64, device=t.device), host)
    return _result(_knn_mean(t, k), host)


def delet_outlier_statistical(point_cloud, nb_neighbors=120, std_ratio=0.1, device=None):
    """Keep the rows whose mean distance to their nb_neighbors nearest rows is below the cloud's
    mean of those plus std_ratio standard deviations (include/pn2.h S1-S5), in input order.  Rows
    keep the input's dtype (the reference returns float64, because Open3D converts)."""
    k = _neighbours("delet_outlier_statistical", nb_neighbors)
    if not float(std_ratio) > 0:
        raise ValueError("pn2.collect.delet_outlier_statistical: std_ratio must be > 0, got %r" % (std_ratio,))
    t, host = _cloud("delet_outlier_statistical", point_cloud, device)
    if t.shape[0] == 0:
        return _result(t, host)
    flags, _ = _stat_flags(_knn_mean(t, k), std_ratio)
    out, offsets = _compact(t, flags, _lib.COMPACT_FLAG_GT)
    return _result(out[:int(offsets[1].item())], host)  # the one host read: the result's length


_SAMPLE_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def _plane_args(who, point_cloud, distance_threshold, ransac_n, num_iterations, samples):
    """The checks that need no device -> (threshold, n, M); ValueError as Open3D raises."""
    lib = _lib.load()
    thr, n, M = float(distance_threshold), int(ransac_n), int(num_iterations)
    if n < 3:
        raise ValueError("pn2.collect.%s: ransac_n must be >= 3, got %d" % (who, n))
    if n > lib.pn2_plane_max_ransac_n():
        raise ValueError("pn2.collect.%s: ransac_n = %d, above the %d the kernel takes"
                         % (who, n, lib.pn2_plane_max_ransac_n()))
    if M < 1:
        raise ValueError("pn2.collect.%s: num_iterations must be >= 1, got %d" % (who, M))
    if M > lib.pn2_plane_max_iterations():
        raise ValueError("pn2.collect.%s: num_iterations = %d, above the %d the kernel takes"
                         % (who, M, lib.pn2_plane_max_iterations()))
    if not (thr > 0 and thr < float("inf")):
        raise ValueError("pn2.collect.%s: distance_threshold must be finite and > 0, got %r"
                         % (who, distance_threshold))
    shape = tuple(point_cloud.shape) if isinstance(point_cloud, torch.Tensor) else np.shape(point_cloud)
    if len(shape) == 2 and shape[0] < n:
        raise ValueError("pn2.collect.%s: %d points, fewer than ransac_n = %d" % (who, shape[0], n))
    if samples is not None:
        tensor = isinstance(samples, torch.Tensor)
        if not tensor:
            samples = np.asarray(samples)
        if tuple(samples.shape) != (M, n):
            raise ValueError("pn2.collect.%s: samples must be [num_iterations, ransac_n] = [%d, %d], got shape %s"
                             % (who, M, n, tuple(samples.shape)))
        if (samples.dtype not in _SAMPLE_DTYPES) if tensor else (samples.dtype.kind not in "iu"):
            raise ValueError("pn2.collect.%s: samples must be integers, got %s" % (who, samples.dtype))
    return thr, n, M


def _samples(samples, N, M, n, device):
    """include/pn2.h P1 -> int32 [M, n] on the device.  None: one np.random.randint(0, N, (M, n))
    from numpy's global generator.  A caller's entry outside [0, N) stays outside it (-1 or N)
    through the cast, so the kernel skips its row and raises PN2_DEVERR_INDEX."""
    if samples is None:
        samples = np.random.randint(0, N, size=(M, n))
    if isinstance(samples, torch.Tensor):
        return samples.to(device).long().clamp(-1, N).to(torch.int32).contiguous()
    return torch.from_numpy(np.clip(np.asarray(samples).astype(np.int64), -1, N).astype(np.int32)).to(device)


def _plane_segment(t, samples, thr, stages=False, ws=None):
    """pn2_plane_segment -> (flags int32 [N], result float64 [8]) by include/pn2.h P1-P6, and with
    stages also (planes float64 [M, 4], count int32 [M], err float64 [M]); all on the device, no
    host read.  ws: a caller's uint8 workspace of pn2_plane_segment_workspace_bytes(N, M), which
    then holds the float64 rows, the hypotheses and the partials after the call."""
    N, C = t.shape
    M, n = samples.shape
    lib = _lib.load()
    with torch.cuda.device(t.device):
        flags = torch.empty(N, dtype=torch.int32, device=t.device)
        result = torch.empty(8, dtype=torch.float64, device=t.device)
        outs = ()
        if stages:
            outs = (torch.empty(M, 4, dtype=torch.float64, device=t.device),
                    torch.empty(M, dtype=torch.int32, device=t.device),
                    torch.empty(M, dtype=torch.float64, device=t.device))
        need = lib.pn2_plane_segment_workspace_bytes(N, M)
        if ws is None:
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=t.device)
        _lib.check(lib.pn2_plane_segment(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), samples.data_ptr(),
                                         M, n, thr, flags.data_ptr(), result.data_ptr(),
                                         *([o.data_ptr() for o in outs] or [None, None, None]), ws.data_ptr(),
                                         ws.numel(), _stream(flags)), "pn2_plane_segment")
    return (flags, result) + outs


def _plane_refit(t, flags):
    """pn2_plane_refit -> float64 [4] on the device (include/pn2.h P7); no host read"""
    N, C = t.shape
    lib = _lib.load()
    with torch.cuda.device(t.device):
        plane = torch.zeros(4, dtype=torch.float64, device=t.device)
        need = lib.pn2_plane_refit_workspace_bytes(N)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=t.device)
        _lib.check(lib.pn2_plane_refit(t.data_ptr(), _DOWNSAMPLE_DTYPES[t.dtype], N, C, _ld(t), flags.data_ptr(),
                                       plane.data_ptr(), ws.data_ptr(), need, _stream(plane)), "pn2_plane_refit")
    return plane


def segment_plane(point_cloud, distance_threshold, ransac_n, num_iterations, samples=None, device=None):
    """Open3D's PointCloud.segment_plane by include/pn2.h P1-P7: (plane_model float64 [4] = a, b,
    c, d of the plane refitted to the inliers, inliers int64 [K] ascending).  samples: the int
    [num_iterations, ransac_n] table of row indices to draw the hypotheses from; None draws it
    with one np.random.randint(0, N, (num_iterations, ransac_n)) from numpy's global generator
    (Open3D draws from its own).  Every hypothesis is scored: there is no early exit."""
    thr, n, M = _plane_args("segment_plane", point_cloud, distance_threshold, ransac_n, num_iterations, samples)
    t, host = _cloud("segment_plane", point_cloud, device)
    flags, _ = _plane_segment(t, _samples(samples, t.shape[0], M, n, t.device), thr)
    plane = _plane_refit(t, flags)
    src = torch.empty(t.shape[0], dtype=torch.int32, device=t.device)
    _, offsets = _compact(t, flags, _lib.COMPACT_FLAG_GT, src=src)
    inliers = src[:int(offsets[1].item())].long()  # the one host read: the result's length
    return _result(plane, host), _result(inliers, host)


def delete_plane(point_cloud, distance_threshold=0.006, ransac_n=20, num_iterations=1000, samples=None, device=None):
    """Remove the dominant plane (the table): the rows that are not inliers of the best RANSAC
    plane (include/pn2.h P1-P6), in input order and in the input's dtype.  samples as in
    segment_plane.  The reference's `visualize` flag is not carried, and the refitted model, which
    the reference discards, is not computed."""
    thr, n, M = _plane_args("delete_plane", point_cloud, distance_threshold, ransac_n, num_iterations, samples)
    t, host = _cloud("delete_plane", point_cloud, device)
    flags, _ = _plane_segment(t, _samples(samples, t.shape[0], M, n, t.device), thr)
    out, offsets = _compact(t, flags, _lib.COMPACT_FLAG_LE)
    return _result(out[:int(offsets[1].item())], host)  # the one host read: the result's length


# knn_mean_distance, delet_outlier_statistical, segment_plane and delete_plane are public but not
# in __all__, which tests/test_abi_collect.py pins to its four names: the collect.py shim imports
# them by name
__all__ = ["clip_distance", "delet_outlier_radius", "cluster_point", "dbscan_labels"]

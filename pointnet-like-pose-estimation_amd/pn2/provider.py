"""Input preparation on the GPU: the host-side steps the reference's
scripts run on every batch before the forward, as one kernel (csrc/preprocess.hip).

The reference does, per batch (test_translation.py:72-84; test_rotation.py:71-80 and
test_sign.py:69-76 without the mean; test_classification.py:71-78 without the splice):

    points = points.data.numpy()                                  # float64 [B,N,C]
    mean = torch.Tensor(np.mean(points[:,:3,:], axis=1))          # translation heads
    points[:, :, 0:3] = provider.normalization(points[:, :, 0:3]) # per-cloud numpy loop
    points = provider.splice_torch(torch.Tensor(points), label)   # per-cloud python loop
    points = points.transpose(2, 1).cuda()

``prepare_batch`` returns the same model input (bit-identical: float64 arithmetic in numpy's
operation order, one rounding to float32) and the same ``mean``, computed on the device from
the float64 batch (host or device tensor, or numpy array).  The points come back as the
reference's [B, C+K, N] view of [B, N, C+K] storage -- the layout its models receive, which
the SA path's FPS / ball-query sum orders depend on.

The training loops (train_translation.py:109-119; train_rotation.py:108-116 and
train_sign.py:107-115 without the mean; train_classification.py:107-112 without the splice)
augment the batch first, on the host, in place:

    points = provider.random_point_dropout(points)                            # per-cloud loop
    points[:, :, 0:3] = provider.random_scale_point_cloud(points[:, :, 0:3])  # per-cloud loop
    points[:, :, 0:3] = provider.shift_point_cloud(points[:, :, 0:3])         # per-cloud loop

``prepare_train_batch`` is that whole sequence as one launch: ``draw_augmentation`` makes the
random draws on the host, consuming numpy's generator exactly as the three functions do, and
the kernel applies them while it reads the batch.  For the same generator state the model
input and the mean are the reference's, bit for bit.
"""
import collections

import numpy as np
import torch

from . import _lib
from .ops import _stream


def _check_batch(who, points, label, num_category, normalize):
    """The input rules both entries share -> (points tensor, int64 labels or None, K)."""
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(points)
    if points.dtype != torch.float64:
        raise TypeError("pn2.provider.%s: points must be float64 (np.loadtxt rows), "
                        "got %s" % (who, points.dtype))
    if points.dim() != 3:
        raise ValueError("pn2.provider.%s: points must be [B, N, C]" % who)
    B, N, C = points.shape
    if normalize and C < 3:
        raise ValueError("pn2.provider.%s: normalising needs C >= 3" % who)
    K = 0
    lab = None
    if label is not None:
        lab = torch.as_tensor(label).reshape(-1).to(torch.int64)
        if lab.numel() != B:
            raise ValueError("pn2.provider.%s: %d labels for %d clouds" % (who, lab.numel(), B))
        # host labels (the DataLoader's) are range-checked like the reference; device labels
        # are not (that would synchronise): an out-of-range one gets an all-zero one-hot
        lab_host = lab if not lab.is_cuda else None
        if B and lab_host is not None and (int(lab_host.min()) < 0 or int(lab_host.max()) >= num_category):
            raise IndexError("index %d is out of bounds for dimension 1 with size %d" % (
                int(lab_host.max()) if int(lab_host.max()) >= num_category else int(lab_host.min()),
                num_category))
        K = int(num_category)
    return points, lab, K


def _pick_device(who, points, device):
    if device is not None:
        dev = torch.device(device)
    elif points.is_cuda:
        dev = points.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")
    if dev.type != "cuda":
        raise RuntimeError("pn2.provider.%s: runs on ROCm devices only (got %s); "
                           "there is no CPU path" % (who, dev))
    return dev


def prepare_batch(points, label=None, num_category=7, with_mean=False, normalize=True,
                  device=None):
    """points: float64 [B, N, C] (torch tensor on any device, or numpy), C >= 3.
    label: [B] class indices (one-hot spliced after the C channels when given; values must be
    in [0, num_category) -- the reference raises IndexError otherwise).
    Returns (model input [B, C+K, N] float32 on the device, mean [B, C] float32 or None)."""
    points, lab, K = _check_batch("prepare_batch", points, label, num_category, normalize)
    B, N, C = points.shape
    dev = _pick_device("prepare_batch", points, device)
    if lab is not None:
        lab = lab.to(dev, non_blocking=True)
    pts = points.to(dev, non_blocking=True)
    out = torch.empty(B, N, C + K, dtype=torch.float32, device=dev)
    mean = torch.empty(B, C, dtype=torch.float32, device=dev) if with_mean else None
    if B and N:
        L = _lib.load()
        _lib.check(L.pn2_prepare_points_f64(
            pts.data_ptr(), B, N, C, pts.stride(0), pts.stride(1), pts.stride(2),
            1 if normalize else 0, 0 if lab is None else lab.data_ptr(), K, out.data_ptr(),
            0 if mean is None else mean.data_ptr(), _stream(out)), "pn2_prepare_points_f64")
    return out.transpose(2, 1), mean


# One batch's random draws.  drop: bool [B, N] (True = the point is replaced by point 0),
# scale: float64 [B], shift: float64 [B, 3]; None = that augmentation is off.
Augmentation = collections.namedtuple("Augmentation", ["drop", "scale", "shift"])


def draw_augmentation(B, N, dropout=True, scale=True, shift=True, max_dropout_ratio=0.875,
                      scale_low=0.8, scale_high=1.25, shift_range=0.1, rng=None):
    """The draws of random_point_dropout, random_scale_point_cloud and shift_point_cloud
    (provider.py:157-164, 144-155, 131-142) for a [B, N, .] batch, from the global np.random
    (rng=None) or an np.random.RandomState, consumed exactly as those functions consume it:
      1. per cloud, random() then random(N);  drop = u <= random() * max_dropout_ratio
         (float64 comparison).  Drawn as one random((B, N + 1)): the same doubles in the same
         order, and the same generator state afterwards
      2. uniform(scale_low, scale_high, B)
      3. uniform(-shift_range, shift_range, (B, 3))
    A stage switched off draws nothing and is None in the result."""
    rs = np.random if rng is None else rng
    drop = sc = sh = None
    if dropout:
        u = rs.random_sample((B, N + 1))
        drop = u[:, 1:] <= u[:, :1] * max_dropout_ratio
    if scale:
        sc = rs.uniform(scale_low, scale_high, B)
    if shift:
        sh = rs.uniform(-shift_range, shift_range, (B, 3))
    return Augmentation(drop, sc, sh)


def _check_augmentation(aug, B, N):
    """-> (drop uint8 [B,N], scale f64 [B], shift f64 [B,3]) host arrays, None where off."""
    parts = []
    for name, dtype, shape in (("drop", np.bool_, (B, N)), ("scale", np.float64, (B,)),
                               ("shift", np.float64, (B, 3))):
        v = getattr(aug, name)
        if v is not None:
            v = np.asarray(v)
            if v.shape != shape:
                raise ValueError("pn2.provider.prepare_train_batch: aug.%s has shape %s, the "
                                 "batch needs %s" % (name, tuple(v.shape), shape))
            v = np.ascontiguousarray(v, dtype=dtype)
        parts.append(v)
    return parts


def prepare_train_batch(points, label=None, num_category=7, with_mean=False, normalize=True,
                        aug=None, device=None, **draw_kwargs):
    """prepare_batch after the training scripts' augmentations (train_translation.py:109-119),
    in one launch.  points / label / num_category / with_mean / normalize / device and the
    errors are prepare_batch's.

    aug: an Augmentation to use as it is (shape-checked; a caller can draw the next batch's
    while the GPU works), or None to call draw_augmentation(B, N, **draw_kwargs) here.  The
    draws reach the device in one non-blocking copy from pinned memory on the kernel's stream.

    The reference augments its numpy batch in place; this never writes to `points` -- the
    augmented float64 batch exists only inside the kernel.
    Returns (model input [B, C+K, N] float32 on the device, mean [B, C] float32 or None); the
    mean is of the first 3 augmented points, as train_translation.py:113 takes it."""
    who = "prepare_train_batch"
    points, lab, K = _check_batch(who, points, label, num_category, normalize)
    B, N, C = points.shape
    if aug is not None:
        if draw_kwargs:
            raise TypeError("pn2.provider.prepare_train_batch: draw options %s given with an "
                            "explicit aug" % sorted(draw_kwargs))
        parts = _check_augmentation(aug, B, N)
    dev = _pick_device(who, points, device)
    if aug is None:
        parts = _check_augmentation(draw_augmentation(B, N, **draw_kwargs), B, N)
    if lab is not None:
        lab = lab.to(dev, non_blocking=True)
    pts = points.to(dev, non_blocking=True)
    out = torch.empty(B, N, C + K, dtype=torch.float32, device=dev)
    mean = torch.empty(B, C, dtype=torch.float32, device=dev) if with_mean else None
    if B and N:
        # one pinned staging buffer [scale | shift | drop] (the float64 parts first: aligned)
        drop, sc, sh = parts
        blobs = [v.reshape(-1).view(np.uint8) for v in (sc, sh, drop) if v is not None]
        ptr = {}
        if blobs:
            total = sum(v.size for v in blobs)
            stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            np.concatenate(blobs, out=stage.numpy())
            with torch.cuda.device(dev):
                d_stage = stage.to(dev, non_blocking=True)
            off = 0
            for name, v in (("scale", sc), ("shift", sh), ("drop", drop)):
                if v is not None:
                    ptr[name] = d_stage.data_ptr() + off
                    off += v.nbytes
        L = _lib.load()
        _lib.check(L.pn2_prepare_train_points_f64(
            pts.data_ptr(), B, N, C, pts.stride(0), pts.stride(1), pts.stride(2),
            1 if normalize else 0, 0 if lab is None else lab.data_ptr(), K,
            ptr.get("drop", 0), ptr.get("scale", 0), ptr.get("shift", 0), out.data_ptr(),
            0 if mean is None else mean.data_ptr(), _stream(out)), "pn2_prepare_train_points_f64")
    return out.transpose(2, 1), mean


# ------------------------------------------------------------- farthest-point downsampling
# The reference's numpy farthest_point_sample(point_cloud, number) (provider.py:183-204, the same
# function in data_utils/ModelNetDataLoader.py:25-46, point_collect/transformer.py:120-141 and
# data_build/*.py), which every cloud passes through before it reaches a model: one launch of
# csrc/fps_points.hip for a whole ragged batch, in the clouds' own dtype, bit for bit.
_DOWNSAMPLE_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float64: _lib.DTYPE_F64}


def _host_clouds(who, clouds):
    """A list of [N_i, C] arrays (or one [B, N, C] array) -> (rows [sum N_i, C], sizes)."""
    if isinstance(clouds, np.ndarray):
        if clouds.ndim != 3:
            raise ValueError("pn2.provider.%s: an array of clouds must be [B, N, C]" % who)
        clouds = list(clouds)
    clouds = [np.asarray(c) for c in clouds]
    if not clouds:
        raise ValueError("pn2.provider.%s: no clouds" % who)
    first = clouds[0]
    for c in clouds:
        if c.ndim != 2:
            raise ValueError("pn2.provider.%s: every cloud must be [N, C]" % who)
        if c.dtype != first.dtype or c.shape[1] != first.shape[1]:
            raise ValueError("pn2.provider.%s: the clouds of one batch share dtype and C" % who)
    if first.dtype not in (np.float32, np.float64):
        raise TypeError("pn2.provider.%s: clouds must be float64 or float32, got %s" % (who, first.dtype))
    if first.shape[1] < 3:
        raise ValueError("pn2.provider.%s: needs C >= 3 (xyz), got C = %d" % (who, first.shape[1]))
    return clouds


def _draw_starts(who, sizes, starts):
    """starts=None: one np.random.randint(0, N) per cloud in list order (an empty cloud raises
    numpy's ValueError there, as in the reference).  Given starts are range-checked here."""
    if starts is None:
        return np.array([np.random.randint(0, n) for n in sizes], dtype=np.int64)
    st = np.asarray(starts).reshape(-1)
    if st.size != len(sizes):
        raise ValueError("pn2.provider.%s: %d starts for %d clouds" % (who, st.size, len(sizes)))
    st = st.astype(np.int64)
    for b, (s, n) in enumerate(zip(st.tolist(), sizes)):
        if s < 0 or s >= n:
            raise IndexError("pn2.provider.%s: start %d of cloud %d is out of bounds for %d points"
                             % (who, s, b, n))
    return st


def _fps_points_launch(rows, ld, C, offsets, starts, total_rows, max_n, number):
    """rows: a device tensor whose data_ptr is row 0.  -> (idx [B, number], pts [B, number, C])."""
    dev = rows.device
    B = len(starts)
    with torch.cuda.device(dev):
        table = torch.from_numpy(np.concatenate([offsets, starts])).pin_memory().to(dev, non_blocking=True)
        idx = torch.empty(B, number, dtype=torch.int64, device=dev)
        out = torch.empty(B, number, C, dtype=rows.dtype, device=dev)
        if B and number:
            L = _lib.load()
            code = _DOWNSAMPLE_DTYPES[rows.dtype]
            need = L.pn2_fps_points_workspace_bytes(code, total_rows, max_n)
            if need < 0:
                raise ValueError("pn2.provider.farthest_point_sample_batch: bad batch shape")
            ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
            _lib.check(L.pn2_fps_points(
                rows.data_ptr(), code, B, table.data_ptr(), table.data_ptr() + 8 * (B + 1), total_rows,
                max_n, C, ld, number, idx.data_ptr(), out.data_ptr(), 0 if ws is None else ws.data_ptr(),
                need, _stream(out)), "pn2_fps_points")
    return idx, out


def farthest_point_sample_batch(clouds, number=1024, starts=None, return_index=False, device=None):
    """The reference's farthest_point_sample for a whole batch in one launch.

    clouds: a list of [N_i, C] numpy arrays (ragged), one [B, N, C] numpy array, or a [B, N, C]
    torch tensor on a ROCm device; float64 or float32, C >= 3.  Only columns 0..2 are measured;
    every column is carried into the result.
    starts: None draws one np.random.randint(0, N_i) per cloud, in order -- what calling the
    reference in a loop consumes; else [B] start rows, checked on the host (IndexError before
    any launch).
    Returns point_cloud[idx] per cloud as [B, number, C] in the input's dtype (with
    return_index, also the int64 [B, number] rows picked): numpy arrays for host input, device
    tensors for a device tensor -- no host round trip, ready for prepare_batch.
    Host coordinates must be finite (ValueError): the kernel orders distances by their bit
    patterns, which differs from numpy on NaN.  A device tensor is not checked (that would
    synchronise)."""
    who = "farthest_point_sample_batch"
    number = int(number)
    if number < 0:
        raise ValueError("negative dimensions are not allowed")
    if isinstance(clouds, torch.Tensor):
        t = clouds
        if t.dim() != 3:
            raise ValueError("pn2.provider.%s: a tensor of clouds must be [B, N, C]" % who)
        if t.dtype not in _DOWNSAMPLE_DTYPES:
            raise TypeError("pn2.provider.%s: clouds must be float64 or float32, got %s" % (who, t.dtype))
        B, N, C = t.shape
        if C < 3:
            raise ValueError("pn2.provider.%s: needs C >= 3 (xyz), got C = %d" % (who, C))
        st = _draw_starts(who, [N] * B, starts)
        dev = _pick_device(who, t, device)
        t = t.to(dev, non_blocking=True)
        # rows of one stride, clouds a whole number of rows apart; else one packed copy
        if B and N and not (t.stride(2) == 1 and t.stride(1) >= C and t.stride(0) % t.stride(1) == 0
                            and t.stride(0) >= N * t.stride(1)):
            t = t.contiguous()
        if B == 0 or N == 0:
            idx = torch.empty(B, number, dtype=torch.int64, device=dev)
            out = torch.empty(B, number, C, dtype=t.dtype, device=dev)
        else:
            ld, step = t.stride(1), t.stride(0) // t.stride(1)
            offsets = np.arange(B + 1, dtype=np.int64) * step
            offsets[B] = (B - 1) * step + N
            idx, out = _fps_points_launch(t, ld, C, offsets, st, int(offsets[B]), N, number)
        return (out, idx) if return_index else out
    clouds = _host_clouds(who, clouds)
    sizes = [len(c) for c in clouds]
    st = _draw_starts(who, sizes, starts)
    C = clouds[0].shape[1]
    for b, c in enumerate(clouds):
        if not np.isfinite(c[:, :3]).all():
            raise ValueError("pn2.provider.%s: cloud %d has a NaN or infinite coordinate" % (who, b))
    dev = _pick_device(who, torch.empty(0), device)
    offsets = np.zeros(len(clouds) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    total = int(offsets[-1])
    stage = torch.empty(total, C, dtype=torch.from_numpy(clouds[0][:0]).dtype, pin_memory=True)
    np.concatenate(clouds, 0, out=stage.numpy())
    with torch.cuda.device(dev):
        rows = stage.to(dev, non_blocking=True)
    idx, out = _fps_points_launch(rows, C, C, offsets, st, total, max(sizes), number)
    out = out.cpu().numpy()
    return (out, idx.cpu().numpy()) if return_index else out


def farthest_point_sample(point_cloud, number=1024):
    """The reference's farthest_point_sample(point_cloud, number) (provider.py:183-204;
    ModelNetDataLoader's (point, npoint) works positionally): point_cloud [N, C] numpy, float64
    or float32 -> point_cloud[idx], [number, C] in the same dtype, for the same state of numpy's
    global generator, of which it consumes exactly one np.random.randint(0, N)."""
    point_cloud = np.asarray(point_cloud)
    if point_cloud.ndim != 2:
        raise ValueError("pn2.provider.farthest_point_sample: point_cloud must be [N, C], got shape %s"
                         % (tuple(point_cloud.shape),))
    C = point_cloud.shape[1]
    if C < 3:
        raise ValueError("pn2.provider.farthest_point_sample: needs C >= 3 (xyz), got C = %d" % C)
    return farthest_point_sample_batch([point_cloud], number)[0]


__all__ = ["prepare_batch", "prepare_train_batch", "draw_augmentation", "Augmentation",
           "farthest_point_sample", "farthest_point_sample_batch"]

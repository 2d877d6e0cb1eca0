"""pn2.collect (csrc/collect.hip) against its numpy restatement tests/collect_ref.py: counts,
kept rows, labels and sampled clusters bit for bit (np.array_equal), generator consumption
included."""
import functools

import numpy as np
import pytest
import torch

import collect_ref as ref

pytestmark = pytest.mark.gpu

TILE = 1024  # candidates per LDS tile of collect_pair_kernel
SLAB = 512   # queries per workgroup
DTYPES = [np.float64, np.float32]


def _collect():
    from pn2 import collect
    return collect


def _gpu_counts(pc, radius):
    from pn2 import _lib
    L = _lib.load()
    t = torch.from_numpy(np.array(pc)).cuda()
    counts = torch.full((len(pc),), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.pn2_radius_count_f64(t.data_ptr(), _lib.DTYPE_F64 if pc.dtype == np.float64 else _lib.DTYPE_F32,
                                      len(pc), pc.shape[1], pc.shape[1], radius, counts.data_ptr(),
                                      _lib.stream_ptr(t.device)), "pn2_radius_count_f64")
    return counts.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _uniform(N, C, dtype):
    pc = ref.uniform_cloud(N, seed=N % 97, C=C, dtype=dtype)
    pc.setflags(write=False)
    return pc


# ------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("N,C", [(1, 3), (255, 6), (256, 3), (257, 3), (1000, 6), (SLAB + 1, 3), (TILE + 1, 3),
                                 (2 * TILE + 1, 6)])
def test_counts(N, C, dtype):
    pc = _uniform(N, C, dtype)
    r = 0.15
    want = ref.radius_counts(pc, r)
    if N >= 255:
        assert want.min() < want.max()
    assert np.array_equal(_gpu_counts(pc, r), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_counts_on_the_boundary_and_duplicates(dtype):
    lattice = ref.lattice_cloud(dtype=dtype)
    for r in (0.125, 0.126, 0.125 * np.sqrt(2.0), 0.25):  # pairs exactly at r, at r*sqrt(2)..., at 2r
        assert np.array_equal(_gpu_counts(lattice, float(r)), ref.radius_counts(lattice, float(r))), r
    assert (_gpu_counts(lattice, 0.125) == 1).all()
    copies = ref.copies_cloud(300, dtype=dtype)
    assert _gpu_counts(copies, 1e-9).tolist() == [300] * 300
    # a row with a NaN coordinate is nobody's neighbour, itself included
    pc = np.array(_uniform(257, 3, dtype))
    pc[5, 1] = np.nan
    got = _gpu_counts(pc, 0.3)
    assert got[5] == 0 and np.array_equal(got, ref.radius_counts(pc, 0.3))


# -------------------------------------------------------------------------------------- clip
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 6, 4])
def test_clip(C, dtype):
    c = _collect()
    pc = np.array(_uniform(1000, C, dtype))
    pc[17, :3] = np.nan
    for axis in (0, 1, 2):
        lo, hi = np.sort(pc[[3, 900], axis])  # bounds equal to stored values: inclusive
        got = c.clip_distance(pc, [lo, hi], axis)
        want = ref.clip_distance(pc, [lo, hi], axis)
        assert got.dtype == pc.dtype and np.array_equal(got, want)
        assert 2 <= len(want) < 999 and lo in got[:, axis] and hi in got[:, axis]
        got = c.clip_distance(pc, [float(lo), float(hi)], axis)  # Python numbers, as the scripts pass
        assert np.array_equal(got, ref.clip_distance(pc, [float(lo), float(hi)], axis))
    assert np.array_equal(c.clip_distance(pc), ref.clip_distance(pc))  # the defaults: the NaN row goes
    assert len(c.clip_distance(pc)) == 999
    assert c.clip_distance(pc, [5, 6]).shape == (0, C)  # everything dropped
    clean = _uniform(257, C, dtype)
    assert np.array_equal(c.clip_distance(clean, [-1, 2]), clean)  # nothing dropped


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_clip_device_tensor_unaligned_and_strided(dtype):
    c = _collect()
    pc = _uniform(1000, 4, dtype)  # rows of 16 or 32 bytes: the 16-byte scatter when aligned
    want = ref.clip_distance(pc, [0.25, 0.75], 0)
    flat = torch.zeros(1 + pc.size, dtype=torch.from_numpy(pc).dtype, device="cuda")
    flat[1:] = torch.from_numpy(pc).cuda().reshape(-1)
    view = flat[1:].view(1000, 4)  # base pointer one element off 16 bytes: the scalar scatter
    assert view.data_ptr() % 16 != 0
    got = c.clip_distance(view, [0.25, 0.75], 0)
    assert isinstance(got, torch.Tensor) and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = torch.zeros(1000, 8, dtype=flat.dtype, device="cuda")
    wide[:, :4] = torch.from_numpy(pc).cuda()
    got = c.clip_distance(wide[:, :4], [0.25, 0.75], 0)  # ld = 8 > C = 4
    assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------------------- radius filter
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 6])
def test_radius_filter(C, dtype):
    c = _collect()
    pc = _uniform(1000, C, dtype)
    r = 0.15
    counts = ref.radius_counts(pc, r)
    nb = int(np.median(counts))  # a measured count: rows AT it go, rows one above stay
    assert (counts == nb).any() and (counts == nb + 1).any()
    for nb_points in (nb - 1, nb, nb + 1, 0, int(counts.max())):
        got = c.delet_outlier_radius(pc, nb_points, r)
        want = ref.delet_outlier_radius(pc, nb_points, r)
        assert got.dtype == pc.dtype and np.array_equal(got, want), nb_points
    assert len(c.delet_outlier_radius(pc, int(counts.max()), r)) == 0
    t = c.delet_outlier_radius(torch.from_numpy(pc).cuda(), nb, r)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), ref.delet_outlier_radius(pc, nb, r))


# ------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("name", sorted(ref.LABEL_FIXTURES))
def test_labels(name, C, dtype):
    c = _collect()
    build, eps, mp = ref.LABEL_FIXTURES[name]
    pc = build(C, dtype)
    want = ref.dbscan_labels(pc, eps, mp)
    first = c.dbscan_labels(pc, eps, mp)
    second = c.dbscan_labels(pc, eps, mp)
    assert first.dtype == np.int32 and first.tobytes() == second.tobytes()
    assert np.array_equal(first, want)


def test_labels_more_than_one_slab():
    """Clusters that span workgroups and candidate tiles of the union pass."""
    c = _collect()
    rng = np.random.RandomState(11)
    parts = [ref.blob(rng, [k * 1.0, 0, 0], 450, 0.04) for k in range(3)]
    pc = ref._finish(np.vstack(parts + [rng.uniform(-9, -1, (50, 3))]), 11, 3, np.float64)
    want = ref.dbscan_labels(pc, 0.03, 20)
    assert want.max() >= 2 and (want == -1).any()
    got = c.dbscan_labels(pc, 0.03, 20)
    assert np.array_equal(got, want) and got.tobytes() == c.dbscan_labels(pc, 0.03, 20).tobytes()


# ----------------------------------------------------------------------------- cluster_point
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 6])
def test_cluster_point(C, dtype):
    c = _collect()
    pc = ref.five_cloud(C=C, dtype=dtype)  # five clusters of unequal size: min_number truncates
    np.random.seed(123)
    want = ref.cluster_point(pc, ref.EPS, 10)
    state_ref = np.random.get_state()
    np.random.seed(123)
    got = c.cluster_point(pc, ref.EPS, 10)
    state = np.random.get_state()
    labels = ref.dbscan_labels(pc, ref.EPS, 10)
    sizes = np.bincount(labels[labels >= 0])
    assert want.shape == (5, sizes.min(), C) and sizes.min() < sizes.max()
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    assert state[0] == state_ref[0] and np.array_equal(state[1], state_ref[1]) and state[2:] == state_ref[2:]
    t = c.cluster_point(torch.from_numpy(pc).cuda(), ref.EPS, 10)
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == want.shape


def test_cluster_point_null_and_one_row(capsys):
    c = _collect()
    assert c.cluster_point(ref.noise_cloud(), ref.EPS, 3) is None
    assert capsys.readouterr().out == "Null point\n"
    one_row = np.array([[0.0, 0, 0], [5, 5, 5], [5, 5, 5.01]])
    with pytest.raises(ValueError):
        ref.cluster_point(one_row, 0.1, 1)
    with pytest.raises(ValueError):
        c.cluster_point(one_row, 0.1, 1)


def test_shim_and_limits():
    import collect
    c = _collect()
    assert collect.clip_distance is c.clip_distance
    with pytest.raises(ValueError):
        c.clip_distance(np.zeros((4, 2)))
    with pytest.raises(TypeError):
        c.clip_distance(np.zeros((4, 3), dtype=np.int64))
    assert c.clip_distance(np.zeros((0, 3))).shape == (0, 3)
    assert c.dbscan_labels(np.zeros((0, 3)), 0.1, 2).shape == (0,)

"""pn2.provider.farthest_point_sample / farthest_point_sample_batch (csrc/fps_points.hip) against
the reference's goldens and its restatement (tests/downsample_ref.py): indices and gathered rows
bit for bit, generator consumption included."""
import numpy as np
import pytest
import torch

import downsample_ref
from conftest import golden_names, load_golden
from test_abi_downsample import F32, F64, lds_limit

pytestmark = pytest.mark.gpu

THREADS = 1024  # the workgroup of fps_points_kernel (include/pn2.h: one 1024-thread workgroup per cloud)


def _provider():
    from pn2 import provider
    return provider


def _cloud(N, C, dtype, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (N, C)).astype(dtype)


def _check(clouds, number, starts):
    """One batched call with given starts == the restatement, cloud by cloud."""
    out, idx = _provider().farthest_point_sample_batch(clouds, number, starts=starts, return_index=True)
    assert out.dtype == clouds[0].dtype and idx.dtype == np.int64
    assert out.shape == (len(clouds), number, clouds[0].shape[1]) and idx.shape == (len(clouds), number)
    for b, (c, s) in enumerate(zip(clouds, starts)):
        want = downsample_ref.sample_indices(c, number, s)
        np.testing.assert_array_equal(idx[b], want, err_msg="cloud %d" % b)
        np.testing.assert_array_equal(out[b], c[want], err_msg="cloud %d" % b)
    return out, idx


@pytest.mark.parametrize("name", golden_names("downsample_"))
def test_goldens(name):
    """ties (lattice, lattice32, dup), float32 vs float64 arithmetic (wide32), contraction (fma32,
    fma64), the 1e10 rule (far), carried columns (c4, c6), number > N (one, five)."""
    g = load_golden("downsample_%s.npz" % name)
    cloud, number = g["cloud"], int(g["number"])
    np.random.seed(int(g["seed"]))
    rows = _provider().farthest_point_sample(cloud, number)
    assert np.random.random() == float(g["next_draw"])
    assert rows.dtype == cloud.dtype and rows.shape == g["rows"].shape
    np.testing.assert_array_equal(rows, g["rows"])
    _, idx = _provider().farthest_point_sample_batch([cloud], number, starts=[g["idx"][0]], return_index=True)
    np.testing.assert_array_equal(idx[0], g["idx"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_small_sizes_and_wave_boundaries(dtype):
    one = _cloud(1, 3, dtype, 1)
    _check([one], 1, [0])
    _check([one], 4, [0])
    five = np.array([[0, 0, 0], [9, 0, 0], [1, 0, 0], [3, 0, 0], [6, 0, 0]], dtype=dtype)
    _, idx = _check([five], 9, [2])
    assert idx[0, 5:].tolist() == [0, 0, 0, 0]
    sizes = (63, 64, 65, THREADS - 1, THREADS, THREADS + 1)
    clouds = [_cloud(n, 3, dtype, 10 + n) for n in sizes]
    _check(clouds, 24, [n - 1 for n in sizes])
    # ties at every size: lattice coordinates (multiples of 1/8)
    clouds = [np.round(c * 4) / 8 for c in clouds]
    _check(clouds, 24, [n // 2 for n in sizes])


@pytest.mark.parametrize("dtype,code", [(np.float64, F64), (np.float32, F32)])
def test_dispatch_boundary(dtype, code):
    """Either side of the LDS / workspace boundary the workspace query reports, alone and in one
    ragged launch (which the larger cloud puts on the workspace path as a whole)."""
    from pn2 import _lib
    L = _lib.load()
    lim = lds_limit(L, code)
    assert L.pn2_fps_points_workspace_bytes(code, lim, lim) == 0
    assert L.pn2_fps_points_workspace_bytes(code, lim + 1, lim + 1) > 0
    below, above = _cloud(lim, 3, dtype, 5), _cloud(lim + 1, 3, dtype, 6)
    _check([below], 8, [lim - 1])
    _check([above], 8, [lim])
    _check([below, above, below[:70]], 8, [3, 0, 69])


def test_duplicated_rows_in_a_batch():
    g = load_golden("downsample_dup.npz")
    cloud = g["cloud"]
    _check([cloud, cloud[::-1].copy(), cloud.astype(np.float32).astype(np.float64)], 48, [0, 299, 7])


def test_far_cloud_is_never_updated():
    """Scaled by 1e6: every distance exceeds the initial 1e10, so only a centroid's own distance
    (0) is ever written and the walk is the first index still at 1e10 -- 0, 1, 2, ... around the
    start -- not the farthest point."""
    g = load_golden("downsample_far.npz")
    cloud = g["cloud"]
    _, idx = _check([cloud], 16, [5])
    assert idx[0].tolist() == [5, 0, 1, 2, 3, 4] + list(range(6, 16))


@pytest.mark.parametrize("C", [3, 4, 6])
def test_columns_and_row_stride(C):
    """Columns past the third are carried, not measured; a device tensor whose rows are wider than
    C is read in place."""
    pv = _provider()
    dev = torch.device("cuda:0")
    host = np.random.RandomState(40 + C).uniform(-1, 1, (3, 300, C + 2))
    host[..., 3:] *= 100.0  # would dominate the distances if measured
    starts = [0, 150, 299]
    wide = torch.from_numpy(host).to(dev)
    view = wide[:, :, :C]
    assert view.stride(1) == C + 2
    out, idx = pv.farthest_point_sample_batch(view, 32, starts=starts, return_index=True)
    assert out.is_cuda and idx.is_cuda and out.dtype == torch.float64 and idx.dtype == torch.int64
    want_out, want_idx = _check(list(np.ascontiguousarray(host[:, :, :C])), 32, starts)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(out.cpu().numpy(), want_out)
    # the same rows whatever the extra columns hold
    _, idx3 = pv.farthest_point_sample_batch(list(np.ascontiguousarray(host[:, :, :3])), 32, starts=starts,
                                             return_index=True)
    np.testing.assert_array_equal(idx3, want_idx)


def test_ragged_batch_and_generator():
    pv = _provider()
    sizes = (1, 65, 300, 1025)
    clouds = [_cloud(n, 3, np.float64, 70 + n) for n in sizes]
    np.random.seed(77)
    want = downsample_ref.farthest_point_sample_loop(clouds, 20)
    want_next = np.random.random()
    np.random.seed(77)
    got = pv.farthest_point_sample_batch(clouds, 20)
    assert np.random.random() == want_next
    np.random.seed(77)
    singles = [pv.farthest_point_sample(c, 20) for c in clouds]
    assert np.random.random() == want_next
    for b in range(len(clouds)):
        np.testing.assert_array_equal(got[b], want[b])
        np.testing.assert_array_equal(singles[b], want[b])
    # given starts are honoured, and consume nothing
    np.random.seed(78)
    _check(clouds, 20, [0, 64, 123, 1024])
    np.random.seed(78)
    state = np.random.random()
    np.random.seed(78)
    pv.farthest_point_sample_batch(clouds, 20, starts=[0, 0, 0, 0])
    assert np.random.random() == state
    # one [B, N, C] host array is a batch of equal clouds
    same = np.stack([_cloud(130, 4, np.float32, s) for s in (1, 2, 3)])
    _check(list(same), 16, [1, 2, 3])
    out = pv.farthest_point_sample_batch(same, 16, starts=[1, 2, 3])
    np.testing.assert_array_equal(out, _check(list(same), 16, [1, 2, 3])[0])


def test_errors_before_any_launch():
    pv = _provider()
    cloud = _cloud(10, 3, np.float64, 3)
    with pytest.raises(IndexError):
        pv.farthest_point_sample_batch([cloud], 4, starts=[10])
    with pytest.raises(IndexError):
        pv.farthest_point_sample_batch([cloud], 4, starts=[-1])
    with pytest.raises(IndexError):
        pv.farthest_point_sample_batch(torch.from_numpy(cloud[None]).cuda(), 4, starts=[10])
    with pytest.raises(ValueError):
        pv.farthest_point_sample(cloud[:, :2], 4)
    with pytest.raises(ValueError):
        pv.farthest_point_sample(cloud[:0], 4)  # numpy's own: randint(0, 0)
    with pytest.raises(TypeError):
        pv.farthest_point_sample(cloud.astype(np.float16), 4)
    for bad in (np.nan, np.inf):
        c = cloud.copy()
        c[4, 1] = bad
        with pytest.raises(ValueError):
            pv.farthest_point_sample(c, 4)
    c = np.concatenate([cloud, np.full((10, 1), np.nan)], 1)  # a NaN in a carried column is legal
    np.random.seed(5)
    rows = pv.farthest_point_sample(c, 4)
    assert rows.shape == (4, 4) and np.isnan(rows[:, 3]).all()
    np.random.seed(5)
    assert pv.farthest_point_sample(cloud, 0).shape == (0, 3)
    assert np.random.random() != np.random.RandomState(5).random_sample()  # the draw was still made
    from pn2 import _lib
    _lib.check_device_errors()


def test_device_chaining_into_prepare_batch():
    """Device tensor in, device tensors out; the sampled clouds fed to prepare_batch equal the
    host route (numpy sampling, then prepare_batch of the host batch)."""
    pv = _provider()
    host = np.random.RandomState(9).uniform(-1, 1, (4, 700, 3))
    starts = [0, 10, 699, 350]
    dev_out = pv.farthest_point_sample_batch(torch.from_numpy(host).cuda(), 128, starts=starts)
    assert isinstance(dev_out, torch.Tensor) and dev_out.is_cuda and dev_out.shape == (4, 128, 3)
    sampled = np.stack([c[downsample_ref.sample_indices(c, 128, s)] for c, s in zip(host, starts)])
    np.testing.assert_array_equal(dev_out.cpu().numpy(), sampled)
    labels = torch.tensor([0, 3, 6, 2])
    a, am = pv.prepare_batch(dev_out, labels, with_mean=True)
    b, bm = pv.prepare_batch(sampled, labels, with_mean=True)
    assert torch.equal(a, b) and torch.equal(am, bm)

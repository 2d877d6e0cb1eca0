"""pn2.collect.segment_plane / delete_plane (csrc/plane.hip) against the numpy restatement
tests/plane_ref.py: every hypothesis' plane, count and err, the best of them, the inlier flags, the
refitted model and the rows that remain, bit for bit (a NaN equals a NaN:
stat_outlier_ref.same_bits), for float64 and float32 clouds."""
import functools

import numpy as np
import pytest
import torch

import collect_ref
import plane_ref as ref
from stat_outlier_ref import same_bits

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def _collect():
    from pn2 import collect
    return collect


def _nmax():
    from pn2 import _lib
    return int(_lib.load().pn2_plane_max_ransac_n())


@functools.lru_cache(maxsize=None)
def _uniform(N, C, dtype):
    pc = collect_ref.uniform_cloud(N, seed=N % 97, C=C, dtype=dtype)
    pc.setflags(write=False)
    return pc


@functools.lru_cache(maxsize=None)
def _table(dtype):
    pc = ref.table_cloud().astype(dtype)
    pc.setflags(write=False)
    return pc


def _run(dev, samples, thr):
    s = torch.from_numpy(np.asarray(samples).astype(np.int32)).cuda()
    return [o.cpu().numpy() for o in _collect()._plane_segment(dev, s, float(thr), stages=True)]


def check(pc, samples, thr, dev=None):
    """Every stage of the GPU against the rule, twice; then the refit, segment_plane's pair and
    delete_plane's rows with the same table.  -> the rule's stages"""
    c = _collect()
    want = ref.segment(pc, samples, thr)
    dev = torch.from_numpy(np.array(pc)).cuda() if dev is None else dev
    flags, result, planes, count, err = _run(dev, samples, thr)
    assert same_bits(planes, want["planes"]), np.flatnonzero((planes != want["planes"]).any(1))[:8]
    assert count.dtype == np.int32 and np.array_equal(count, want["count"])
    assert same_bits(err, want["err"]), np.flatnonzero(err != want["err"])[:8]
    assert same_bits(result[:7], want["result"][:7]), (result, want["result"])
    assert flags.dtype == np.int32 and np.array_equal(flags, want["flags"])
    for a, b in zip(_run(dev, samples, thr), (flags, result, planes, count, err)):
        assert a.tobytes() == b.tobytes()  # two runs, the same bits
    model = c._plane_refit(dev, torch.from_numpy(flags).cuda()).cpu().numpy()  # the GPU's flags, equal to the rule's
    want_model = ref.refit(pc, want["flags"])
    assert same_bits(model, want_model), (model, want_model)
    M, n = np.shape(samples)
    got_model, inliers = c.segment_plane(dev, thr, n, M, samples=samples)
    assert inliers.dtype == torch.int64 and inliers.is_cuda and got_model.dtype == torch.float64
    assert same_bits(got_model.cpu().numpy(), want_model)
    assert np.array_equal(inliers.cpu().numpy(), np.flatnonzero(want["flags"]))
    kept = c.delete_plane(dev, thr, n, M, samples=samples)
    assert kept.dtype == dev.dtype and kept.is_cuda
    assert kept.cpu().numpy().tobytes() == np.asarray(pc)[want["flags"] == 0].tobytes()
    return want


# ------------------------------------------------------------------------------------- sizes
# N: one chunk, a chunk's edge, three chunks; M: one hypothesis, the score kernel's 128-thread and
# 256-hypothesis blocks and the select kernel's stride; n: both fits, the default and the cap
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N,M,n,C", [(3, 1, 3, 3), (3, 64, 3, 3), (20, 63, 20, 3), (20, 64, 4, 6), (1023, 65, 3, 3),
                                     (1024, 257, 4, 3), (1025, 64, None, 6), (1025, 1, 20, 3), (2500, 1000, 20, 3),
                                     (2500, 257, 3, 6), (2500, 65, None, 3)])
def test_sizes(N, M, n, C, dtype):
    n = _nmax() if n is None else n
    pc = _uniform(N, C, dtype)
    samples = np.random.RandomState(N + M).randint(0, N, size=(M, n))
    want = check(pc, samples, 0.05)
    if N >= 1023 and n == 3 and M > 1:
        assert want["result"][5] > 3 and len(set(want["count"].tolist())) > 5  # a real contest


# ------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_table_at_the_defaults(dtype):
    pc = _table(dtype)
    samples = np.random.RandomState(1).randint(0, len(pc), size=(1000, 20))
    want = check(pc, samples, 0.006)
    assert 0 < want["result"][5] <= 3000 and not (want["flags"] != 0)[~ref.is_table(pc)].any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_table_is_removed_whole_with_three_point_samples(dtype):
    pc = _table(dtype)
    np.random.seed(1)
    want = check(pc, ref.draw_samples(len(pc), 3, 64), 0.006)
    assert want["result"][5] == 3000 and np.array_equal(want["flags"] != 0, ref.is_table(pc))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lattice_ties_go_to_the_lowest_index(dtype):
    pc = collect_ref.lattice_cloud(dtype=dtype)
    np.random.seed(2)
    want = check(pc, ref.draw_samples(len(pc), 3, 200), 1e-3)
    assert want["result"][4] == 5 and want["result"][5] == 49 and want["result"][6] == 0.0
    assert ((want["count"] == 49) & (want["err"] == 0.0)).sum() == 13


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_sample_rows(dtype):
    pc = ref.degenerate_cloud(dtype)
    want = check(pc, ref.DEGENERATE_N3, 0.01)
    assert not want["planes"][[0, 1, 3]].any() and want["result"][4] == 2
    want = check(pc, ref.DEGENERATE_N4, 0.01)
    assert want["count"].tolist() == [0, 13, 0]
    want = check(pc, ref.ALL_ZERO_N3, 0.01)  # nothing but zero planes: index -1, no inlier, the cloud unchanged
    assert want["result"].tolist() == [0, 0, 0, 0, -1, 0, 0, 0] and not want["flags"].any()
    assert np.array_equal(_collect().delete_plane(pc, 0.01, 3, 4, samples=ref.ALL_ZERO_N3), pc)
    model, inliers = _collect().segment_plane(pc, 0.01, 3, 4, samples=ref.ALL_ZERO_N3)
    assert isinstance(model, np.ndarray) and not model.any() and inliers.shape == (0,) and inliers.dtype == np.int64


# ------------------------------------------------------------------------ indices out of range
@pytest.mark.parametrize("n", [3, 4])
def test_out_of_range_sample_is_skipped_and_reported(n):
    from pn2 import _lib
    pc = _uniform(1025, 3, np.float64)
    N = len(pc)
    samples = np.random.RandomState(5).randint(0, N, size=(65, n))
    clean = ref.segment(pc, samples, 0.05)
    _lib.device_errors()  # nothing pending from earlier tests
    check(pc, samples, 0.05)
    assert _lib.device_errors() == 0
    bad = samples.copy()
    bad[0, 0], bad[7, n - 1], bad[64, 1] = N, -1, 1 << 30
    want = check(pc, bad, 0.05)
    assert _lib.device_errors() == _lib.DEVERR_INDEX
    assert _lib.device_errors() == 0  # taken
    rest = np.delete(np.arange(65), [0, 7, 64])
    assert not want["planes"][[0, 7, 64]].any() and not want["count"][[0, 7, 64]].any()
    assert same_bits(want["planes"][rest], clean["planes"][rest]) and same_bits(want["err"][rest], clean["err"][rest])
    # through the public call, where an entry of any size stays out of range through the int32 cast
    wide = bad.astype(np.int64)
    wide[64, 1] = (1 << 32) + 5
    got = _collect().delete_plane(pc, 0.05, n, 65, samples=wide)
    assert _lib.device_errors() == _lib.DEVERR_INDEX
    assert np.array_equal(got, pc[want["flags"] == 0])


# ----------------------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [3, 20])
def test_nan_and_inf_rows(n, dtype):
    pc = np.array(_table(dtype)[:2000])
    table = ref.is_table(pc)
    bad = np.array([0, 63, 1023, 1024, 1999])
    pc[bad[0], 0], pc[bad[1], 1], pc[bad[2], 2], pc[bad[3], 0], pc[bad[4]] = np.nan, np.inf, -np.inf, np.inf, np.nan
    samples = np.random.RandomState(6).randint(0, len(pc), size=(64, n))
    samples[3, 0], samples[10, n - 1], samples[11, 1] = bad[0], bad[1], bad[4]  # as sample members
    want = check(pc, samples, 0.006)
    assert not want["count"][[3, 10, 11]].any() and want["result"][4] not in (3, 10, 11)  # a NaN plane never wins
    assert want["result"][5] > 0 and not want["flags"][bad].any()  # never inliers
    kept = _collect().delete_plane(pc, 0.006, n, 64, samples=samples)
    assert isinstance(kept, np.ndarray) and kept.dtype == pc.dtype
    assert (~np.isfinite(kept)).any(1).sum() == 5  # and so they stay
    assert np.isfinite(kept).all(1).sum() == len(pc) - 5 - int(want["result"][5])
    assert table[want["flags"] != 0].all()


# ------------------------------------------------------------------------ layouts, return types
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padded_rows_and_tensors(dtype):
    c = _collect()
    pc = _uniform(1025, 6, dtype)
    samples = np.random.RandomState(7).randint(0, len(pc), size=(65, 4))
    wide = torch.zeros(len(pc), 8, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    wide[:, :6] = torch.from_numpy(np.array(pc)).cuda()
    view = wide[:, :6]  # C = 6, ld = 8
    assert view.stride() == (8, 1)
    want = check(pc, samples, 0.05, dev=view)
    kept = pc[want["flags"] == 0]
    host = c.delete_plane(torch.from_numpy(np.array(pc)), 0.05, 4, 65, samples=torch.from_numpy(samples))
    assert isinstance(host, torch.Tensor) and np.array_equal(host.cpu().numpy(), kept)  # a host tensor: a tensor back
    got = c.delete_plane(pc, 0.05, 4, 65, samples=samples.tolist())  # an array: an array back
    assert isinstance(got, np.ndarray) and got.dtype == pc.dtype and np.array_equal(got, kept)
    model, inliers = c.segment_plane(pc, 0.05, 4, 65, samples=samples.astype(np.int16))
    assert isinstance(model, np.ndarray) and model.dtype == np.float64 and model.shape == (4,)
    assert inliers.dtype == np.int64 and np.array_equal(inliers, np.flatnonzero(want["flags"]))


def test_score_entry_repeats_the_score_launch():
    """pn2_plane_score on the workspace a segment call filled writes the same partials again."""
    from pn2 import _lib
    lib = _lib.load()
    pc = _uniform(2500, 3, np.float64)
    dev = torch.from_numpy(np.array(pc)).cuda()
    samples = torch.from_numpy(np.random.RandomState(8).randint(0, 2500, size=(257, 3)).astype(np.int32)).cuda()
    need = lib.pn2_plane_segment_workspace_bytes(2500, 257)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    _collect()._plane_segment(dev, samples, 0.05, ws=ws)
    filled = ws.clone()
    stream = _lib.stream_ptr(dev.device)
    _lib.check(lib.pn2_plane_score(2500, 257, 0.01, ws.data_ptr(), need, stream), "pn2_plane_score")
    assert not torch.equal(ws, filled)  # another threshold, other partials
    _lib.check(lib.pn2_plane_score(2500, 257, 0.05, ws.data_ptr(), need, stream), "pn2_plane_score")
    assert torch.equal(ws, filled)


# ------------------------------------------------------------------------------------ the draw
def test_default_path_draws_once_from_numpys_generator():
    c = _collect()
    pc = _table(np.float64)
    table = ref.is_table(pc)
    np.random.seed(1)
    kept = c.delete_plane(pc, 0.006, 3, 64)
    after = np.random.get_state()
    np.random.seed(1)
    samples = np.random.randint(0, len(pc), size=(64, 3))
    expect = np.random.get_state()
    assert after[0] == expect[0] and np.array_equal(after[1], expect[1]) and after[2:] == expect[2:]
    assert np.array_equal(kept, ref.delete_plane(pc, 0.006, 3, 64, samples=samples)) and np.array_equal(kept, pc[~table])
    np.random.seed(1)
    model, inliers = c.segment_plane(pc, 0.006, 3, 64)
    assert np.array_equal(np.random.get_state()[1], expect[1]) and np.random.get_state()[2] == expect[2]
    np.random.seed(1)
    want_model, want_inliers = ref.segment_plane(pc, 0.006, 3, 64)
    assert same_bits(model, want_model) and np.array_equal(inliers, want_inliers)
    np.random.seed(3)
    got = c.delete_plane(pc)  # distance_threshold = 0.006, ransac_n = 20, num_iterations = 1000
    np.random.seed(3)
    assert np.array_equal(got, ref.delete_plane(pc)) and 900 <= len(got) < 3900


# --------------------------------------------------------------------------------- end to end
def test_chain_clip_plane_filter_labels_on_device_tensors():
    import collect
    rng = np.random.RandomState(11)
    far = rng.uniform([-1, -1, 2.0001], [1, 1, 4], (300, 3))
    xyz = np.vstack([ref.table_cloud(), far])[rng.permutation(4200)]
    pc = np.hstack([xyz, rng.uniform(0, 1, (4200, 3))])
    dev = torch.from_numpy(pc).cuda()
    np.random.seed(4)
    clipped = collect.clip_distance(dev)
    rest = collect.delete_plane(clipped, 0.006, 3, 64)
    dense = collect.delet_outlier_radius(rest, 10, 0.02)
    labels = collect.dbscan_labels(dense, 0.02, 5)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (clipped, rest, dense, labels))
    np.random.seed(4)
    w_clipped = collect_ref.clip_distance(pc)
    w_rest = ref.delete_plane(w_clipped, 0.006, 3, 64)
    w_dense = collect_ref.delet_outlier_radius(w_rest, 10, 0.02)
    w_labels = collect_ref.dbscan_labels(w_dense, 0.02, 5)
    assert len(w_clipped) == 3900 and len(w_rest) == 900 and 0 < len(w_dense) <= 900
    assert np.array_equal(clipped.cpu().numpy(), w_clipped) and np.array_equal(rest.cpu().numpy(), w_rest)
    assert np.array_equal(dense.cpu().numpy(), w_dense) and np.array_equal(labels.cpu().numpy(), w_labels)
    assert w_labels.max() == 1  # the two boxes

"""The statistical outlier removal's entry points (csrc/knn.hip; additive to ABI 19).  Argument
validation happens before any device call, so these run without a GPU; pointers are dummy non-null
values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null, 16-byte aligned pointer
F32, F64 = 0, 1
EINVAL, EUNSUPPORTED = -1, -2
LIMIT = 1 << 20

SYMBOLS = ("pn2_knn_max_k", "pn2_knn_mean_dist_workspace_bytes", "pn2_knn_mean_dist_f64", "pn2_stat_outlier_flags")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_symbols_and_header():
    lib, L = _L()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert L.pn2_knn_max_k() >= 256
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    start = header.index("statistical outlier removal")
    assert start > header.index("int pn2_dbscan_labels(")  # a block of its own, after the front end's
    block = header[start:header.index("int pn2_stat_outlier_flags(")]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
    for text in ("S1 Candidates", "S2 Distance", "S3 Mean distance", "S4 Cloud statistics", "S5 Selection",
                 "k_eff = min(k, F)", "((dx*dx) + (dy*dy)) + (dz*dz)", "correctly rounded sqrt",
                 "mean[i] = -1.0", "std = sqrt(sq_sum / (valid - 1))", "cloud_mean + std_ratio * std",
                 "mean[i] > 0 && mean[i] < threshold"):
        assert text in block, text


def test_shim_resolves_the_new_names_and_all_is_unchanged():
    import collect
    import pn2.collect
    assert collect.delet_outlier_statistical is pn2.collect.delet_outlier_statistical
    assert collect.knn_mean_distance is pn2.collect.knn_mean_distance
    names = ["clip_distance", "cluster_point", "dbscan_labels", "delet_outlier_radius"]
    assert sorted(collect.__all__) == names and sorted(pn2.collect.__all__) == names


def _knn(L, pts=P, dtype=F64, N=10, C=3, ld=3, k=4, mean=P, ws=P, ws_bytes=1 << 30):
    return L.pn2_knn_mean_dist_f64(pts, dtype, N, C, ld, k, mean, ws, ws_bytes, None)


def _stat(L, mean=P, N=10, std_ratio=0.1, flags=P, stats=P):
    return L.pn2_stat_outlier_flags(mean, N, std_ratio, flags, stats, None)


def test_knn_validation():
    _, L = _L()
    who = b"pn2_knn_mean_dist_f64"
    for p in ("pts", "mean"):
        assert _knn(L, **{p: None}) == EINVAL, p
        assert who + b": null pointer" in L.pn2_last_error()
    for dtype in (-1, 2, 8):
        assert _knn(L, dtype=dtype) == EINVAL and who + b": unknown dtype" in L.pn2_last_error()
    for kw in (dict(C=2, ld=2), dict(C=0), dict(C=65, ld=65), dict(C=4, ld=3), dict(N=-1)):
        assert _knn(L, **kw) == EINVAL, kw
        assert who + b": bad shape" in L.pn2_last_error()
    assert _knn(L, N=LIMIT + 1) == EUNSUPPORTED
    assert b"pn2_collect_max_points" in L.pn2_last_error()
    for k in (0, -1, -(1 << 40)):
        assert _knn(L, k=k) == EINVAL and who + b": nb_neighbors" in L.pn2_last_error(), k
    kmax = L.pn2_knn_max_k()
    for k in (kmax + 1, 1 << 40):
        assert _knn(L, k=k) == EUNSUPPORTED, k
        assert who in L.pn2_last_error() and b"pn2_knn_max_k" in L.pn2_last_error()
    # nothing to do: no launch, no device and no workspace needed; the arguments are still checked
    assert _knn(L, N=0) == 0 and _knn(L, N=0, C=64, ld=64, k=kmax, ws=None, ws_bytes=0) == 0
    assert _knn(L, N=0, k=0) == EINVAL and _knn(L, N=0, k=kmax + 1) == EUNSUPPORTED


def test_knn_workspace():
    _, L = _L()
    q = L.pn2_knn_mean_dist_workspace_bytes
    kmax = L.pn2_knn_max_k()
    for bad in ((-1, 4), (LIMIT + 1, 4), (10, 0), (10, -1), (10, kmax + 1)):
        assert q(*bad) == -1, bad
    sizes = [q(n, 120) for n in (0, 1, 2, 3, 1000, LIMIT)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes)
    assert q(1, 1) == 48 and q(3, kmax) == 96 and q(LIMIT, 120) == 3 * 8 * LIMIT  # three float64 per row
    need = q(1000, 120)
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=P, ws_bytes=need - 1), dict(ws=P + 8, ws_bytes=need),
               dict(ws=P, ws_bytes=0)):
        assert _knn(L, N=1000, k=120, **kw) == EINVAL, kw
        assert b"pn2_knn_mean_dist_f64: workspace too small" in L.pn2_last_error()


def test_stat_flags_validation():
    _, L = _L()
    who = b"pn2_stat_outlier_flags"
    for p in ("mean", "flags", "stats"):
        assert _stat(L, **{p: None}) == EINVAL, p
        assert who + b": null pointer" in L.pn2_last_error()
    assert _stat(L, N=-1) == EINVAL and who + b": bad shape" in L.pn2_last_error()
    assert _stat(L, N=LIMIT + 1) == EUNSUPPORTED and b"pn2_collect_max_points" in L.pn2_last_error()
    for r in (0.0, -0.1, float("-inf"), float("nan")):
        assert _stat(L, std_ratio=r) == EINVAL and who + b": std_ratio" in L.pn2_last_error(), r
    assert _stat(L, N=0) == 0
    assert _stat(L, N=0, std_ratio=0.0) == EINVAL


def test_python_arguments():
    """ValueError before any device work, as Open3D raises."""
    import numpy as np
    from pn2 import collect
    pc = np.zeros((5, 3))
    for k in (0, -3):
        with pytest.raises(ValueError):
            collect.delet_outlier_statistical(pc, k, 1.0)
        with pytest.raises(ValueError):
            collect.knn_mean_distance(pc, k)
    with pytest.raises(ValueError):
        collect.knn_mean_distance(pc, _L()[1].pn2_knn_max_k() + 1)
    for r in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            collect.delet_outlier_statistical(pc, 4, r)

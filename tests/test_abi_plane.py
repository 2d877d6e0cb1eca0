"""The plane segmentation's entry points (csrc/plane.hip; additive to ABI 19).  Argument validation
happens before any device call, so these run without a GPU; pointers are dummy non-null values that
are never dereferenced."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

P = 16  # a non-null, 16-byte aligned pointer
F32, F64 = 0, 1
EINVAL, EUNSUPPORTED = -1, -2
LIMIT = 1 << 20

SYMBOLS = ("pn2_plane_max_ransac_n", "pn2_plane_max_iterations", "pn2_plane_segment_workspace_bytes",
           "pn2_plane_segment", "pn2_plane_score", "pn2_plane_refit_workspace_bytes", "pn2_plane_refit")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_symbols_and_header():
    lib, L = _L()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert L.pn2_plane_max_ransac_n() >= 64 and L.pn2_plane_max_iterations() >= 4096
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    start = header.index("plane segmentation: delete_plane (point_collect/collect.py:6-28; csrc/plane.hip)")
    assert start > header.index("int pn2_stat_outlier_flags(")  # a block of its own, after the statistical one
    block = header[start:header.index("int pn2_plane_refit(")]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    assert re.search(r"#define PN2_PLANE_CHUNK 1024\b", block)
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
    for text in ("P1 Samples", "P2 Hypothesis, n > 3", "P3 Hypothesis, n == 3", "P4 Score", "P5 Best", "P6 Inliers",
                 "P7 Refit", "np.random.randint(0, N, size=(M, n))", "PN2_DEVERR_INDEX",
                 "det_x = yy*zz - yz*yz", "det_y = xx*zz - xz*xz", "det_z = xx*yy - xy*xy",
                 "abc = (det_x, xz*yz - xy*zz, xy*yz - xz*yy)", "abc = (xz*yz - xy*zz, det_y, xy*xz - yz*xx)",
                 "abc = (xy*yz - xz*yy, xy*xz - yz*xx, det_z)", "norm = sqrt((a*a + b*b) + c*c)",
                 "d = -((a*cx + b*cy) + c*cz)", "abc = (e0y*e1z - e0z*e1y, e0z*e1x - e0x*e1z, e0x*e1y - e0y*e1x)",
                 "d = -((a*p0x + b*p0y) + c*p0z)", "dist_i = |((a*x_i + b*y_i) + c*z_i) + d|",
                 "count_m > count || (count_m == count && err_m < err)", "early exit",
                 "none of it has been checked against an\n * Open3D build"):
        assert text in block, text


def test_shim_resolves_the_new_names_and_all_is_unchanged():
    import collect
    import pn2.collect
    assert collect.delete_plane is pn2.collect.delete_plane
    assert collect.segment_plane is pn2.collect.segment_plane
    names = ["clip_distance", "cluster_point", "dbscan_labels", "delet_outlier_radius"]
    assert sorted(collect.__all__) == names and sorted(pn2.collect.__all__) == names


def _seg(L, pts=P, dtype=F64, N=10, C=3, ld=3, samples=P, M=8, n=3, thr=0.006, flags=P, result=P, planes=None,
         count=None, err=None, ws=P, ws_bytes=1 << 40):
    return L.pn2_plane_segment(pts, dtype, N, C, ld, samples, M, n, thr, flags, result, planes, count, err, ws,
                               ws_bytes, None)


def _refit(L, pts=P, dtype=F64, N=10, C=3, ld=3, flags=P, plane=P, ws=P, ws_bytes=1 << 40):
    return L.pn2_plane_refit(pts, dtype, N, C, ld, flags, plane, ws, ws_bytes, None)


def _cloud_checks(L, call, who, pointers):
    for p in pointers:
        assert call(L, **{p: None}) == EINVAL, p
        assert who + b": null pointer" in L.pn2_last_error()
    for dtype in (-1, 2, 8):
        assert call(L, dtype=dtype) == EINVAL and who + b": unknown dtype" in L.pn2_last_error()
    for kw in (dict(C=2, ld=2), dict(C=0), dict(C=65, ld=65), dict(C=4, ld=3), dict(N=-1)):
        assert call(L, **kw) == EINVAL, kw
        assert who + b": bad shape" in L.pn2_last_error()
    assert call(L, N=LIMIT + 1) == EUNSUPPORTED
    assert who in L.pn2_last_error() and b"pn2_collect_max_points" in L.pn2_last_error()


def test_segment_validation():
    _, L = _L()
    who = b"pn2_plane_segment"
    _cloud_checks(L, _seg, who, ("pts", "samples", "flags", "result"))
    nmax, mmax = L.pn2_plane_max_ransac_n(), L.pn2_plane_max_iterations()
    for n in (2, 0, -1, -(1 << 40)):
        assert _seg(L, n=n) == EINVAL and who + b": ransac_n" in L.pn2_last_error(), n
    for n in (nmax + 1, 1 << 40):
        assert _seg(L, n=n) == EUNSUPPORTED, n
        assert who in L.pn2_last_error() and b"pn2_plane_max_ransac_n" in L.pn2_last_error()
    for M in (0, -1, -(1 << 40)):
        assert _seg(L, M=M) == EINVAL and who + b": num_iterations" in L.pn2_last_error(), M
    for M in (mmax + 1, 1 << 40):
        assert _seg(L, M=M) == EUNSUPPORTED, M
        assert who in L.pn2_last_error() and b"pn2_plane_max_iterations" in L.pn2_last_error()
    for thr in (0.0, -0.0, -0.006, float("nan"), float("inf"), float("-inf")):
        assert _seg(L, thr=thr) == EINVAL and who + b": distance_threshold" in L.pn2_last_error(), thr
    # nothing to do: no launch, no device and no workspace needed; the arguments are still checked
    assert _seg(L, N=0) == 0 and _seg(L, N=0, C=64, ld=64, n=nmax, M=mmax, ws=None, ws_bytes=0) == 0
    assert _seg(L, N=0, n=2) == EINVAL and _seg(L, N=0, M=0) == EINVAL and _seg(L, N=0, thr=0.0) == EINVAL
    assert _seg(L, N=0, n=nmax + 1) == EUNSUPPORTED and _seg(L, N=0, M=mmax + 1) == EUNSUPPORTED
    assert _seg(L, N=0, dtype=5) == EINVAL and _seg(L, N=0, samples=None) == EINVAL


def test_segment_workspace():
    _, L = _L()
    q = L.pn2_plane_segment_workspace_bytes
    mmax = L.pn2_plane_max_iterations()
    for bad in ((-1, 8), (LIMIT + 1, 8), (10, 0), (10, -1), (10, mmax + 1)):
        assert q(*bad) == -1, bad
    sizes = [q(n, 1000) for n in (0, 1, 2, 3, 1000, 1024, 1025, 307200, LIMIT)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes)
    sizes = [q(2500, m) for m in (1, 2, 63, 64, 65, 257, 1000, mmax)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and all(s % 16 == 0 for s in sizes)
    # three float64 per row, four per hypothesis, (int32, float64) per chunk and hypothesis
    assert q(1024, 4) == 3 * 8192 + 4 * 32 + 4 * 8 + 4 * 4 and q(1025, 4) == 3 * 8208 + 4 * 32 + 2 * 4 * 8 + 2 * 4 * 4
    need = q(1000, 64)
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=P, ws_bytes=need - 1), dict(ws=P + 8, ws_bytes=need),
               dict(ws=P, ws_bytes=0)):
        assert _seg(L, N=1000, M=64, **kw) == EINVAL, kw
        assert b"pn2_plane_segment: workspace too small" in L.pn2_last_error()


def test_score_validation():
    """The measurement entry: pn2_plane_segment's checks of N, M, the threshold and the workspace."""
    _, L = _L()
    who = b"pn2_plane_score"
    mmax = L.pn2_plane_max_iterations()

    def score(N=1000, M=64, thr=0.006, ws=P, ws_bytes=1 << 40):
        return L.pn2_plane_score(N, M, thr, ws, ws_bytes, None)

    for kw in (dict(N=-1), dict(M=0), dict(M=-3)):
        assert score(**kw) == EINVAL and who + b": bad shape" in L.pn2_last_error(), kw
    assert score(N=LIMIT + 1) == EUNSUPPORTED and b"pn2_collect_max_points" in L.pn2_last_error()
    assert score(M=mmax + 1) == EUNSUPPORTED and b"pn2_plane_max_iterations" in L.pn2_last_error()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert score(thr=thr) == EINVAL and who + b": distance_threshold" in L.pn2_last_error(), thr
    assert score(N=0, ws=None, ws_bytes=0) == 0
    need = L.pn2_plane_segment_workspace_bytes(1000, 64)
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=P, ws_bytes=need - 1), dict(ws=P + 8, ws_bytes=need)):
        assert score(**kw) == EINVAL and who + b": workspace too small" in L.pn2_last_error(), kw


def test_refit_validation_and_workspace():
    _, L = _L()
    who = b"pn2_plane_refit"
    _cloud_checks(L, _refit, who, ("pts", "flags", "plane"))
    assert _refit(L, N=0) == 0 and _refit(L, N=0, C=64, ld=64, ws=None, ws_bytes=0) == 0
    assert _refit(L, N=0, plane=None) == EINVAL
    q = L.pn2_plane_refit_workspace_bytes
    assert q(-1) == -1 and q(LIMIT + 1) == -1
    sizes = [q(n) for n in (0, 1, 1024, 1025, 2049, 307200, LIMIT)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes) and q(1024) < q(1025)
    need = q(3000)
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=P, ws_bytes=need - 1), dict(ws=P + 8, ws_bytes=need),
               dict(ws=P, ws_bytes=0)):
        assert _refit(L, N=3000, **kw) == EINVAL, kw
        assert who + b": workspace too small" in L.pn2_last_error()


def test_python_arguments():
    """ValueError before any device work, as Open3D raises."""
    from pn2 import collect
    _, L = _L()
    pc = np.zeros((30, 3))
    ok = dict(distance_threshold=0.006, ransac_n=3, num_iterations=8)
    bad = [dict(ransac_n=2), dict(ransac_n=0), dict(ransac_n=31),  # N < ransac_n
           dict(ransac_n=L.pn2_plane_max_ransac_n() + 1), dict(num_iterations=0), dict(num_iterations=-5),
           dict(num_iterations=L.pn2_plane_max_iterations() + 1), dict(distance_threshold=0),
           dict(distance_threshold=-0.006), dict(distance_threshold=float("nan")),
           dict(distance_threshold=float("inf")),
           dict(samples=np.zeros((8, 4), dtype=np.int64)), dict(samples=np.zeros((7, 3), dtype=np.int64)),
           dict(samples=np.zeros(24, dtype=np.int64)), dict(samples=np.zeros((8, 3), dtype=np.float64)),
           dict(samples=np.zeros((8, 3), dtype=bool))]
    for kw in bad:
        for fn in (collect.delete_plane, collect.segment_plane):
            with pytest.raises(ValueError):
                fn(pc, **{**ok, **kw})
    import torch
    for samples in (torch.zeros(8, 3), torch.zeros(8, 3, dtype=torch.bool), torch.zeros(3, 8, dtype=torch.int64)):
        with pytest.raises(ValueError):
            collect.delete_plane(pc, samples=samples, **ok)
    with pytest.raises(ValueError):
        collect.delete_plane(np.zeros((0, 3)))  # fewer points than ransac_n
    with pytest.raises(ValueError):
        collect.delete_plane(np.zeros((19, 6)))  # the defaults: ransac_n = 20

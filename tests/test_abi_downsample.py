"""pn2_fps_points / pn2_fps_points_workspace_bytes (the numpy-rule downsampling, additive to ABI
19).  Argument validation happens before any device call, so these run without a GPU; pointers
are dummy non-null values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null, 8-byte aligned pointer
F32, F64 = 0, 1
BIG = 1 << 40


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def lds_limit(L, dtype):
    """The largest cloud whose distances stay in LDS, found through the workspace query."""
    lo, hi = 1, 1 << 30
    assert L.pn2_fps_points_workspace_bytes(dtype, BIG, lo) == 0
    assert L.pn2_fps_points_workspace_bytes(dtype, BIG, hi) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if L.pn2_fps_points_workspace_bytes(dtype, BIG, mid) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def test_symbols_and_header():
    lib, L = _L()
    for s in ("pn2_fps_points", "pn2_fps_points_workspace_bytes"):
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert (lib.DTYPE_F32, lib.DTYPE_F64) == (F32, F64)
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_DTYPE_F32\s+0\b", header)
    assert re.search(r"#define\s+PN2_DTYPE_F64\s+1\b", header)
    assert "PN2_ABI_VERSION stays 19" in header


def _call(L, pts=P, dtype=F64, B=2, offsets=P, starts=P, rows=100, max_n=60, C=3, ld=3, S=8, out_idx=P,
          out_pts=P, ws=None, ws_bytes=0):
    return L.pn2_fps_points(pts, dtype, B, offsets, starts, rows, max_n, C, ld, S, out_idx, out_pts, ws,
                            ws_bytes, None)


def test_validation():
    _, L = _L()
    for name in ("pts", "offsets", "starts", "out_idx", "out_pts"):
        assert _call(L, **{name: None}) == -1, name
        assert b"pn2_fps_points: null pointer" in L.pn2_last_error()
    for dtype in (-1, 2, 8):
        assert _call(L, dtype=dtype) == -1 and b"unknown dtype" in L.pn2_last_error()
    for kw in (dict(C=2), dict(C=0), dict(ld=2), dict(C=4, ld=3), dict(B=-1), dict(S=-1), dict(max_n=0),
               dict(max_n=101), dict(S=1 << 31), dict(max_n=1 << 31, rows=1 << 32)):
        assert _call(L, **kw) == -1, kw
        assert b"pn2_fps_points: bad shape" in L.pn2_last_error()
    # nothing to do: no launch, no device needed
    assert _call(L, B=0) == 0
    assert _call(L, S=0) == 0


@pytest.mark.parametrize("dtype,size", [(F32, 4), (F64, 8)])
def test_workspace_query_and_boundary(dtype, size):
    _, L = _L()
    q = L.pn2_fps_points_workspace_bytes
    lim = lds_limit(L, dtype)
    # 160 KiB of LDS less the wave slots: the documented boundaries
    assert lim == (160 * 1024 - 384) // size
    # monotone in max_n across the boundary, and in total_rows past it
    rows = 4 * lim
    seq = [q(dtype, rows, n) for n in (1, 64, lim - 1, lim, lim + 1, lim + 2, 2 * lim, rows)]
    assert seq == sorted(seq) and seq[3] == 0 and seq[4] == rows * size == seq[-1]
    assert q(dtype, rows + 1, lim + 1) == (rows + 1) * size
    assert q(dtype, 10, 0) == 0
    for bad in ((dtype, -1, 0), (dtype, 5, 6), (dtype, 5, -1), (7, 5, 5)):
        assert q(*bad) == -1, bad
    # past the boundary the entry wants that workspace, aligned
    need = q(dtype, lim + 1, lim + 1)
    kw = dict(dtype=dtype, B=1, rows=lim + 1, max_n=lim + 1)
    assert _call(L, **kw) == -1 and b"workspace too small" in L.pn2_last_error()
    assert _call(L, ws=P, ws_bytes=need - 1, **kw) == -1 and b"workspace too small" in L.pn2_last_error()
    assert _call(L, ws=P + 4, ws_bytes=need, **kw) == -1 and b"workspace too small" in L.pn2_last_error()
    assert _call(L, ws=None, ws_bytes=need, **kw) == -1 and b"workspace too small" in L.pn2_last_error()

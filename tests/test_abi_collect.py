"""The camera-cloud front end's entry points (csrc/collect.hip; additive to ABI 19).  Argument
validation happens before any device call, so these run without a GPU; pointers are dummy
non-null values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null, 16-byte aligned pointer
F32, F64 = 0, 1
GT, LABEL, LE = 0, 1, 2
EINVAL, EUNSUPPORTED = -1, -2
LIMIT = 1 << 20

SYMBOLS = ("pn2_collect_max_points", "pn2_clip_flags", "pn2_radius_count_f64", "pn2_compact_rows_workspace_bytes",
           "pn2_compact_rows", "pn2_dbscan_labels_workspace_bytes", "pn2_dbscan_labels")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_symbols_and_header():
    lib, L = _L()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert L.pn2_collect_max_points() == LIMIT
    assert (lib.COMPACT_FLAG_GT, lib.COMPACT_LABEL, lib.COMPACT_FLAG_LE) == (GT, LABEL, LE)
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    block = header[header.index("camera-cloud front end"):header.index("int pn2_dbscan_labels(")]
    assert "PN2_ABI_VERSION stays 19" in block
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
    for name, value in (("FLAG_GT", GT), ("LABEL", LABEL), ("FLAG_LE", LE)):
        assert re.search(r"#define\s+PN2_COMPACT_%s\s+%d\b" % (name, value), header)
    # the rules are stated where the other entries state theirs
    for text in ("d2 = ((dx*dx) + (dy*dy)) + (dz*dz)", "d2 < r*r", "is > nb_points", ">= min_points",
                 "smallest core index", "smallest label among its core neighbours"):
        assert text in block, text
    import collect
    import pn2.collect
    assert collect.cluster_point is pn2.collect.cluster_point
    assert sorted(collect.__all__) == ["clip_distance", "cluster_point", "dbscan_labels", "delet_outlier_radius"]


def _clip(L, pts=P, dtype=F64, N=10, C=3, ld=3, axis=2, flags=P):
    return L.pn2_clip_flags(pts, dtype, N, C, ld, axis, 0.0, 2.0, flags, None)


def _count(L, pts=P, dtype=F64, N=10, C=3, ld=3, counts=P):
    return L.pn2_radius_count_f64(pts, dtype, N, C, ld, 0.05, counts, None)


def _compact(L, pts=P, dtype=F64, N=10, C=3, ld=3, keys=P, mode=GT, thresh=0, buckets=1, out_rows=P, out_src=None,
             offsets=P, ws=P, ws_bytes=1 << 30):
    return L.pn2_compact_rows(pts, dtype, N, C, ld, keys, mode, thresh, buckets, out_rows, out_src, offsets, ws,
                              ws_bytes, None)


def _dbscan(L, pts=P, dtype=F64, N=10, C=3, ld=3, min_points=5, counts=P, labels=P, nclusters=P, ws=P,
            ws_bytes=1 << 30):
    return L.pn2_dbscan_labels(pts, dtype, N, C, ld, 0.03, min_points, counts, labels, nclusters, ws, ws_bytes, None)


ENTRIES = [("pn2_clip_flags", _clip, ("pts", "flags")),
           ("pn2_radius_count_f64", _count, ("pts", "counts")),
           ("pn2_compact_rows", _compact, ("pts", "keys", "out_rows", "offsets")),
           ("pn2_dbscan_labels", _dbscan, ("pts", "counts", "labels", "nclusters"))]


@pytest.mark.parametrize("name,call,pointers", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_validation(name, call, pointers):
    _, L = _L()
    who = name.encode()
    for p in pointers:
        assert call(L, **{p: None}) == EINVAL, p
        assert who + b": null pointer" in L.pn2_last_error()
    for dtype in (-1, 2, 8):
        assert call(L, dtype=dtype) == EINVAL and who + b": unknown dtype" in L.pn2_last_error()
    for kw in (dict(C=2, ld=2), dict(C=0), dict(C=65, ld=65), dict(C=4, ld=3), dict(N=-1)):
        assert call(L, **kw) == EINVAL, kw
        assert who + b": bad shape" in L.pn2_last_error()
    assert call(L, C=64, ld=64, N=0) == 0
    # the documented size limit
    assert call(L, N=LIMIT + 1) == EUNSUPPORTED
    assert b"pn2_collect_max_points" in L.pn2_last_error()
    # nothing to do: no launch, no device needed
    assert call(L, N=0) == 0


def test_entry_specific_arguments():
    _, L = _L()
    for axis in (-1, 3):
        assert _clip(L, axis=axis) == EINVAL and b"axis" in L.pn2_last_error()
    assert _clip(L, C=6, ld=8, axis=5, N=0) == 0
    for kw in (dict(mode=3), dict(mode=-1)):
        assert _compact(L, **kw) == EINVAL and b"unknown mode" in L.pn2_last_error()
    for kw in (dict(buckets=0), dict(buckets=2), dict(mode=LE, buckets=2), dict(thresh=1 << 31),
               dict(mode=LABEL, buckets=-1)):
        assert _compact(L, **kw) == EINVAL and b"bad buckets" in L.pn2_last_error(), kw
    assert _dbscan(L, min_points=1 << 31) == EINVAL and b"min_points" in L.pn2_last_error()


def test_workspace_queries():
    _, L = _L()
    q = L.pn2_compact_rows_workspace_bytes
    # one int32 per (256-row chunk, bucket), rounded to 16 bytes
    assert q(0, 1) == 0 and q(1, 1) == 16 and q(256, 4) == 16 and q(257, 4) == 32 and q(LIMIT, 1) == 4096 * 4
    assert q(1000, 5) == 4 * 5 * 4
    for bad in ((-1, 1), (LIMIT + 1, 1), (10, 0), (10, -3)):
        assert q(*bad) == -1, bad
    # 2^26 table entries is the most one compaction takes
    assert q(LIMIT, 1 << 14) == (1 << 26) * 4 and q(LIMIT, (1 << 14) + 1) == -1
    assert _compact(L, N=LIMIT, mode=LABEL, buckets=(1 << 14) + 1) == EUNSUPPORTED
    assert b"table entries" in L.pn2_last_error()
    d = L.pn2_dbscan_labels_workspace_bytes
    assert d(-1) == -1 and d(LIMIT + 1) == -1
    sizes = [d(n) for n in (0, 1, 255, 256, 257, 1000, LIMIT)]
    assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes) and sizes[0] > 0
    assert 7 * 4 * LIMIT <= sizes[-1] <= 8 * 4 * LIMIT  # seven int32 arrays and the chunk table


@pytest.mark.parametrize("call,need", [(_compact, lambda L: L.pn2_compact_rows_workspace_bytes(1000, 1)),
                                       (_dbscan, lambda L: L.pn2_dbscan_labels_workspace_bytes(1000))],
                         ids=["pn2_compact_rows", "pn2_dbscan_labels"])
def test_short_or_misaligned_workspace(call, need):
    _, L = _L()
    need = need(L)
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=P, ws_bytes=need - 1), dict(ws=P + 8, ws_bytes=need),
               dict(ws=P, ws_bytes=0)):
        assert call(L, N=1000, **kw) == EINVAL, kw
        assert b"workspace too small" in L.pn2_last_error()

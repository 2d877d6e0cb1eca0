"""csrc/v1_transform.hip's entries (additive to ABI 19): the header block, the ctypes binding,
pn2_transform_slab_rows / pn2_transform_workspace_bytes, the argument validation of the four
entries, and the two host tuning keys.  Validation happens before any device call, so these run
without a GPU; pointers are dummy non-null values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null, 8-byte aligned pointer
EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = ("pn2_transform_points_f32", "pn2_transform_points_backward_f32", "pn2_orthogonality_forward_f32",
           "pn2_orthogonality_backward_f32")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_block():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    at = header.index("the PointNet-v1 per-cloud transforms and their orthogonality regulariser")
    block = header[at:header.index("int64_t pn2_transform_slab_rows", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    for word in ("ONE float32 chain", "ROW INDEPENDENCE", "THE dx RULE", "THE dT RULE", "ascending n", "ascending s",
                 "BITWISE SYMMETRIC", "row-major", "norm[b] == 0", "float atomics", "graph-capturable",
                 "pointnet_utils.py:140-147", "PN2_EUNSUPPORTED", "negative stride"):
        assert word in block, word
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19


def test_lib_exports_and_binds():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for name in ENTRIES + ("pn2_transform_slab_rows", "pn2_transform_workspace_bytes"):
        assert hasattr(L, name) and name in lib.SIGNATURES, name
        decl = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        nargs = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert len(lib.SIGNATURES[name][1]) == nargs, name
    from pn2 import ops, train
    import torch
    for fn in (ops.transform_points_direct, ops.transform_points_backward_direct, ops.orthogonality_forward_direct,
               ops.orthogonality_backward_direct, train.transform_points, train.orthogonality_loss,
               train.point_mlp_frozen):
        assert callable(fn)
    for op in ("transform_points", "transform_points_backward", "orthogonality_forward", "orthogonality_backward"):
        assert hasattr(torch.ops.pn2, op), op


def test_slab_rows_and_workspace_bytes():
    _, L = _L()
    R = L.pn2_transform_slab_rows()
    assert R >= 1 and all(L.pn2_transform_slab_rows() == R for _ in range(3))  # a function of nothing
    for B, N, k in ((1, 1, 1), (3, R - 1, 3), (3, R, 64), (2, R + 1, 5), (24, 1024, 64), (3, 10240, 3)):
        assert L.pn2_transform_workspace_bytes(B, N, k) == B * -(-N // R) * k * k * 8, (B, N, k)
    for B, N, k in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (2, 5, 65), (-1, 5, 3)):
        assert L.pn2_transform_workspace_bytes(B, N, k) == -1, (B, N, k)


def _fwd(L, x=P, xs=(15, 3, 1), T=P, ldt=3, y=P, ys=(15, 3, 1), B=2, N=5, k=3):
    return L.pn2_transform_points_f32(x, *xs, T, ldt, y, *ys, B, N, k, None)


def _bwd(L, dy=P, ds=(15, 3, 1), x=P, xs=(15, 3, 1), T=P, ldt=3, dx=P, gs=(15, 3, 1), dT=P, B=2, N=5, k=3, ws=P,
         wsb=1 << 20):
    return L.pn2_transform_points_backward_f32(dy, *ds, x, *xs, T, ldt, dx, *gs, dT, B, N, k, ws, wsb, None)


def _of(L, T=P, ldt=3, B=2, k=3, G=P, norm=P, loss=P):
    return L.pn2_orthogonality_forward_f32(T, ldt, B, k, G, norm, loss, None)


def _ob(L, T=P, ldt=3, norm=P, dloss=P, B=2, k=3, dT=P):
    return L.pn2_orthogonality_backward_f32(T, ldt, norm, dloss, B, k, dT, None)


CALLS = {
    "pn2_transform_points_f32": (_fwd, ("x", "T", "y"), ("xs", "ys"), ("B", "N", "k")),
    "pn2_transform_points_backward_f32": (_bwd, ("dy",), ("ds", "xs", "gs"), ("B", "N", "k")),
    "pn2_orthogonality_forward_f32": (_of, ("T", "norm", "loss"), (), ("B", "k")),
    "pn2_orthogonality_backward_f32": (_ob, ("T", "norm", "dloss", "dT"), (), ("B", "k")),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_validation(name):
    _, L = _L()
    call, ptrs, strides, dims = CALLS[name]

    def bad(code, text, **kw):
        assert call(L, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    for ptr in ptrs:
        bad(EINVAL, b"null pointer", **{ptr: None})
    for dim in dims:
        bad(EINVAL, b"bad shape", **{dim: 0})
        bad(EINVAL, b"bad shape", **{dim: -2})
    bad(EUNSUPPORTED, b"above 64", k=65, ldt=65)
    bad(EUNSUPPORTED, b"2^30", B=(1 << 30) + 1)
    bad(EINVAL, b"row stride", ldt=2)
    for s in strides:
        for pos in range(3):
            v = [15, 3, 1]
            v[pos] = -v[pos]
            bad(EINVAL, b"negative stride", **{s: tuple(v)})
    if "transform_points" in name:
        bad(EUNSUPPORTED, b"2^30", N=(1 << 30) + 1)


def test_backward_optional_outputs_and_workspace():
    _, L = _L()
    name = b"pn2_transform_points_backward_f32"

    def bad(text, **kw):
        assert _bwd(L, **kw) == EINVAL, kw
        msg = L.pn2_last_error()
        assert name in msg and text in msg, (kw, msg)

    bad(b"null pointer", dx=None, dT=None)          # nothing to compute
    bad(b"null pointer", T=None)                    # dx needs T
    bad(b"null pointer", x=None)                    # dT needs x
    bad(b"null pointer", ws=None)                   # ... and the workspace
    bad(b"workspace", wsb=2 * 1 * 9 * 8 - 1)        # one byte short
    bad(b"8-byte aligned", ws=P + 4)
    # what a skipped output alone reads is not required: the calls get as far as the next check
    bad(b"workspace", T=None, dx=None, ldt=0, gs=(-1, -1, -1), wsb=0)
    bad(b"row stride", x=None, dT=None, ws=None, wsb=0, xs=(-1, -1, -1), ldt=2)


def test_tuning_keys():
    from pn2 import tuning
    for key in ("v1_transform", "v1_eval_grad"):
        assert tuning.get(key) == 0 and tuning.V1_DEFAULTS[key] == 0 and tuning.V1_RANGES[key] == (0, 1)
        with tuning.override(**{key: 1}):
            assert tuning.get(key) == 1
        assert tuning.get(key) == 0
        for wrong in (2, -1):
            with pytest.raises(ValueError):
                with tuning.override(**{key: wrong}):
                    pass
            assert tuning.get(key) == 0
        assert key in tuning.__doc__
        assert key not in tuning.HOST_DEFAULTS  # the older keys' table keeps its contents
    assert tuning._parse("v1_transform=1, v1_eval_grad=1") == {"v1_transform": 1, "v1_eval_grad": 1}

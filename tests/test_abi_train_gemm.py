"""pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32 (additive to ABI 19): the header, the
ctypes binding, the entries' argument validation and the host tuning key train_gemm.
Validation happens before any device call, so these run without a GPU; pointers are dummy
non-null values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null pointer
BIG = 1 << 40
EINVAL, EUNSUPPORTED = -1, -2
NEW = ("pn2_gemm_nt_f32", "pn2_gemm_nn_f32", "pn2_gemm_tn_f32", "pn2_gemm_tn_workspace_bytes",
       "pn2_gemm_tn_slab_rows")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_declares_entries_and_abi_stays_19():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for s in NEW[:3]:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    for s in NEW[3:]:
        assert re.search(r"\bint64_t\s+%s\s*\(" % s, header), s
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    at = header.index("csrc/train_gemm.hip")
    block = header[at:header.index("int pn2_gemm_nt_f32", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    assert "THE ORDER RULE" in block and "ROW INDEPENDENCE" in block
    # the earlier blocks keep their sentence
    assert header.count("so PN2_ABI_VERSION stays 19.") >= 3
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19


def test_lib_exports_and_binds():
    lib, L = _L()
    for s in NEW:
        assert hasattr(L, s) and s in lib.SIGNATURES, s


def test_slab_rows_and_workspace_bytes():
    _, L = _L()
    R = L.pn2_gemm_tn_slab_rows()
    assert R > 0 and R % 32 == 0
    # the header documents exactly ceil(M/R) * N * K * 4 bytes, no rounding
    for M, N, K in ((1, 1, 1), (R, 13, 3), (2 * R + 37, 64, 131), (524288, 64, 3), (0, 5, 7)):
        assert L.pn2_gemm_tn_workspace_bytes(M, N, K) == -(-M // R) * N * K * 4, (M, N, K)
    for M, N, K in ((-1, 4, 4), (4, 0, 4), (4, 4, 0), (4, 4097, 4), (4, 4, 4097)):
        assert L.pn2_gemm_tn_workspace_bytes(M, N, K) == -1, (M, N, K)


def _nt(L, A=P, lda=9, B=P, ldb=9, bias=P, C=P, ldc=5, M=7, N=5, K=9):
    return L.pn2_gemm_nt_f32(A, lda, B, ldb, bias, C, ldc, M, N, K, None)


def _nn(L, A=P, lda=9, B=P, ldb=5, C=P, ldc=5, M=7, N=5, K=9):
    return L.pn2_gemm_nn_f32(A, lda, B, ldb, C, ldc, M, N, K, None)


def _tn(L, A=P, lda=5, B=P, ldb=9, C=P, ldc=9, M=7, N=5, K=9, ws=P, ws_bytes=BIG):
    return L.pn2_gemm_tn_f32(A, lda, B, ldb, C, ldc, M, N, K, ws, ws_bytes, None)


ENTRIES = (("pn2_gemm_nt_f32", _nt), ("pn2_gemm_nn_f32", _nn), ("pn2_gemm_tn_f32", _tn))


@pytest.mark.parametrize("name,call", ENTRIES)
def test_validation(name, call):
    _, L = _L()

    def bad(codes, text, **kw):
        assert call(L, **kw) in codes, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    for ptr in ("A", "B", "C"):
        bad((EINVAL,), b"null pointer", **{ptr: None})
    bad((EINVAL, EUNSUPPORTED), b"N=0", N=0)
    bad((EINVAL, EUNSUPPORTED), b"K=4097", K=4097, lda=5000, ldb=5000, ldc=5000)
    bad((EINVAL, EUNSUPPORTED), b"N=4097", N=4097, lda=5000, ldb=5000, ldc=5000)
    bad((EINVAL,), b"M=-1", M=-1)
    # lda below A's width: K for nt / nn, N for tn
    bad((EINVAL,), b"leading dimension", lda=4 if name == "pn2_gemm_tn_f32" else 8)
    bad((EINVAL,), b"leading dimension", ldc=4)
    assert call(L, M=0) == 0  # nothing to do: no launch
    if name == "pn2_gemm_nt_f32":
        assert call(L, M=0, bias=None) == 0


def test_tn_workspace_validation():
    _, L = _L()
    need = L.pn2_gemm_tn_workspace_bytes(7, 5, 9)
    assert need == 5 * 9 * 4
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None)):
        assert _tn(L, **kw) == EINVAL, kw
        assert b"pn2_gemm_tn_f32: workspace too small" in L.pn2_last_error()
    assert _tn(L, M=0, ws=None, ws_bytes=0) == 0


def test_train_gemm_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["train_gemm"] == 0 and tuning.get("train_gemm") == 0
    with tuning.override(train_gemm=1):
        assert tuning.get("train_gemm") == 1
    assert tuning.get("train_gemm") == 0
    for wrong in (2, -1):
        with pytest.raises(ValueError):
            with tuning.override(train_gemm=wrong):
                pass
        assert tuning.get("train_gemm") == 0
    assert "train_gemm" in tuning.__doc__

"""pn2_fc_train_max_rows / pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32 (additive to ABI 19):
the header, the ctypes binding, the entries' argument validation and the host tuning key
train_head.  Validation happens before any device call, so these run without a GPU; pointers
are dummy non-null values that are never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null pointer
EINVAL, EUNSUPPORTED = -1, -2
NO_RELU, FROZEN = 1, 2
NEW = ("pn2_fc_bn_forward_f32", "pn2_fc_bn_backward_f32", "pn2_fc_train_max_rows")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_declares_entries_and_abi_stays_19():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for s in NEW[:2]:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    assert re.search(r"\bint64_t\s+pn2_fc_train_max_rows\s*\(\s*void\s*\)", header)
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    at = header.index("csrc/fc_train.hip")
    block = header[at:header.index("int64_t pn2_fc_train_max_rows", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    assert "THE ORDER RULES" in block and "ROW INDEPENDENCE" in block
    for word in ("fma", "ascending row order", "No float atomics", "pn2_gemm_nn_f32"):
        assert word in block, word
    assert header.count("so PN2_ABI_VERSION stays 19.") >= 4
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert lib.LAYER_NO_RELU == NO_RELU and lib.LAYER_FROZEN_STATS == FROZEN


def test_lib_exports_and_binds():
    lib, L = _L()
    for s in NEW:
        assert hasattr(L, s) and s in lib.SIGNATURES, s
    from pn2 import ops, train
    assert callable(ops.fc_bn_forward_direct) and callable(ops.fc_bn_backward_direct)
    assert callable(train.linear_bn_train) and issubclass(train._FcBnTrain, __import__("torch").autograd.Function)


def test_max_rows():
    _, L = _L()
    assert L.pn2_fc_train_max_rows() >= 64
    from pn2 import ops
    assert ops.fc_train_max_rows() == L.pn2_fc_train_max_rows()


def _fwd(L, X=P, ldx=9, W=P, ldw=9, bias=P, B=7, N=5, K=9, eps=1e-5, momentum=0.1, rm=P, rv=P, gamma=P,
         beta=P, Y=P, ldy=5, A=P, lda=5, stats=P, flags=0):
    return L.pn2_fc_bn_forward_f32(X, ldx, W, ldw, bias, B, N, K, eps, momentum, rm, rv, gamma, beta, Y, ldy,
                                   A, lda, stats, flags, None)


def _bwd(L, dA=P, ldd=5, Y=P, ldy=5, X=P, ldx=9, stats=P, gamma=P, beta=P, B=7, N=5, K=9, dY=P, ldyy=5,
         dW=P, ldw=9, dbias=P, dgamma=P, dbeta=P, flags=0):
    return L.pn2_fc_bn_backward_f32(dA, ldd, Y, ldy, X, ldx, stats, gamma, beta, B, N, K, dY, ldyy, dW, ldw,
                                    dbias, dgamma, dbeta, flags, None)


ENTRIES = (("pn2_fc_bn_forward_f32", _fwd, ("X", "W", "bias", "Y", "A"), ("ldx", "ldw", "ldy", "lda")),
           ("pn2_fc_bn_backward_f32", _bwd, ("dA", "Y", "X", "dY", "dW", "dbias"),
            ("ldd", "ldy", "ldx", "ldyy", "ldw")))


@pytest.mark.parametrize("name,call,ptrs,lds", ENTRIES)
def test_validation(name, call, ptrs, lds):
    _, L = _L()
    big = L.pn2_fc_train_max_rows() + 1

    def bad(code, text, **kw):
        assert call(L, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    for flags in (0, NO_RELU, FROZEN, FROZEN | NO_RELU):
        for ptr in ptrs:
            bad(EINVAL, b"null pointer", flags=flags, **{ptr: None})
        for dim in ("B", "N", "K"):
            bad(EINVAL, b"bad shape", flags=flags, **{dim: 0})
            bad(EINVAL, b"bad shape", flags=flags, **{dim: -3})
        for ld in lds:
            bad(EINVAL, b"leading dimension", flags=flags, **{ld: 4})
        bad(EINVAL, b"null pointer", flags=flags, beta=None)  # gamma given without beta
        bad(EINVAL, b"null pointer", flags=flags, stats=None)
        bad(EUNSUPPORTED, b"rows", flags=flags, B=big)
        bad(EUNSUPPORTED, b"rows", flags=flags, B=big, gamma=None, beta=None, stats=None)
    bad(EINVAL, b"unknown flags", flags=4)
    # batch statistics of a single row (torch refuses it); frozen and no-BN single rows are
    # valid shapes and would launch, so they are not called here
    bad(EINVAL, b"B=1", B=1)
    bad(EINVAL, b"B=1", B=1, flags=NO_RELU)


def test_forward_running_statistics_pointers():
    _, L = _L()
    for kw in (dict(rm=None), dict(rv=None)):
        assert _fwd(L, flags=FROZEN, **kw) == EINVAL, kw
        assert b"running_mean" in L.pn2_last_error()
        assert _fwd(L, momentum=0.1, **kw) == EINVAL, kw
        assert b"running_mean" in L.pn2_last_error()


def test_backward_gradient_pointers():
    _, L = _L()
    for kw in (dict(dgamma=None), dict(dbeta=None)):
        assert _bwd(L, **kw) == EINVAL, kw
        assert b"null pointer" in L.pn2_last_error()


def test_train_head_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["train_head"] == 0 and tuning.get("train_head") == 0
    assert tuning.HOST_RANGES["train_head"] == (0, 1)
    with tuning.override(train_head=1):
        assert tuning.get("train_head") == 1
    assert tuning.get("train_head") == 0
    for wrong in (2, -1):
        with pytest.raises(ValueError):
            with tuning.override(train_head=wrong):
                pass
        assert tuning.get("train_head") == 0
    assert "train_head" in tuning.__doc__

"""pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32 (additive to ABI 19): the header,
the ctypes binding, the entries' argument validation -- every case of test_abi_fc_train.py
against the any-B entries -- and the host tuning key train_head_rows.  Validation happens before
any device call, so these run without a GPU; pointers are dummy non-null values that are never
dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null pointer
EINVAL, EUNSUPPORTED = -1, -2
NO_RELU, FROZEN = 1, 2
PAIRS = (("pn2_fc_bn_forward_rows_f32", "pn2_fc_bn_forward_f32"),
         ("pn2_fc_bn_backward_rows_f32", "pn2_fc_bn_backward_f32"))
MAX_B = 1 << 30


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def _arguments(header, name):
    """The declaration's argument list as [(type, name)], comments and spacing removed."""
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, name
    text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    out = []
    for arg in text.split(","):
        words = arg.replace("*", " * ").split()
        out.append((" ".join(words[:-1]), words[-1]))
    return out


def test_header_declares_entries_with_the_same_arguments():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for new, old in PAIRS:
        args = _arguments(header, new)
        assert args == _arguments(header, old), new
        assert len(args) == 21
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    at = header.index("the same layer for any number of rows")
    block = header[at:header.index("int pn2_fc_bn_forward_rows_f32", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    for word in ("THE ORDER RULES", "2^30", "PN2_EUNSUPPORTED", "bit for bit", "never split"):
        assert word in block, word


def test_lib_exports_and_binds():
    lib, L = _L()
    for new, old in PAIRS:
        assert hasattr(L, new) and new in lib.SIGNATURES, new
        assert lib.SIGNATURES[new] == lib.SIGNATURES[old], new
    from pn2 import ops
    assert callable(ops.fc_rows_forward_direct) and callable(ops.fc_rows_backward_direct)


def test_max_rows_is_still_64():
    _, L = _L()
    assert L.pn2_fc_train_max_rows() == 64
    from pn2 import ops
    assert ops.fc_train_max_rows() == 64


def _fwd(L, X=P, ldx=9, W=P, ldw=9, bias=P, B=7, N=5, K=9, eps=1e-5, momentum=0.1, rm=P, rv=P, gamma=P,
         beta=P, Y=P, ldy=5, A=P, lda=5, stats=P, flags=0):
    return L.pn2_fc_bn_forward_rows_f32(X, ldx, W, ldw, bias, B, N, K, eps, momentum, rm, rv, gamma, beta, Y,
                                        ldy, A, lda, stats, flags, None)


def _bwd(L, dA=P, ldd=5, Y=P, ldy=5, X=P, ldx=9, stats=P, gamma=P, beta=P, B=7, N=5, K=9, dY=P, ldyy=5,
         dW=P, ldw=9, dbias=P, dgamma=P, dbeta=P, flags=0):
    return L.pn2_fc_bn_backward_rows_f32(dA, ldd, Y, ldy, X, ldx, stats, gamma, beta, B, N, K, dY, ldyy, dW,
                                         ldw, dbias, dgamma, dbeta, flags, None)


ENTRIES = (("pn2_fc_bn_forward_rows_f32", _fwd, ("X", "W", "bias", "Y", "A"), ("ldx", "ldw", "ldy", "lda")),
           ("pn2_fc_bn_backward_rows_f32", _bwd, ("dA", "Y", "X", "dY", "dW", "dbias"),
            ("ldd", "ldy", "ldx", "ldyy", "ldw")))


@pytest.mark.parametrize("name,call,ptrs,lds", ENTRIES)
def test_validation(name, call, ptrs, lds):
    _, L = _L()

    def bad(code, text, **kw):
        assert call(L, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    for B in (7, 65, 200):  # the same answers below and above the 64-row kernels' limit
        for flags in (0, NO_RELU, FROZEN, FROZEN | NO_RELU):
            for ptr in ptrs:
                bad(EINVAL, b"null pointer", B=B, flags=flags, **{ptr: None})
            for dim in ("N", "K"):
                bad(EINVAL, b"bad shape", B=B, flags=flags, **{dim: 0})
                bad(EINVAL, b"bad shape", B=B, flags=flags, **{dim: -3})
            for ld in lds:
                bad(EINVAL, b"leading dimension", B=B, flags=flags, **{ld: 4})
            bad(EINVAL, b"null pointer", B=B, flags=flags, beta=None)  # gamma given without beta
            bad(EINVAL, b"null pointer", B=B, flags=flags, stats=None)
        bad(EINVAL, b"unknown flags", B=B, flags=4)
    for flags in (0, NO_RELU, FROZEN, FROZEN | NO_RELU):
        bad(EINVAL, b"bad shape", flags=flags, B=0)
        bad(EINVAL, b"bad shape", flags=flags, B=-3)
        # the only row limit: the kernels' int32 row counter
        bad(EUNSUPPORTED, b"rows", flags=flags, B=MAX_B + 1)
        bad(EUNSUPPORTED, b"rows", flags=flags, B=MAX_B + 1, gamma=None, beta=None, stats=None)
    # batch statistics of a single row (torch refuses it); frozen and no-BN single rows are
    # valid shapes and would launch, so they are not called here
    bad(EINVAL, b"B=1", B=1)
    bad(EINVAL, b"B=1", B=1, flags=NO_RELU)


@pytest.mark.parametrize("name,call,ptrs,lds", ENTRIES)
def test_65_rows_are_not_rejected_for_their_count(name, call, ptrs, lds):
    """The row count is checked before the leading dimensions (the 64-row entries answer
    PN2_EUNSUPPORTED here): at 65, 2^20 and 2^30 rows the any-B entries get as far as the
    leading dimension's PN2_EINVAL, so the row count passed."""
    _, L = _L()
    old = getattr(L, name.replace("_rows", ""))
    for B in (65, 1 << 20, MAX_B):
        assert call(L, B=B, **{lds[0]: 4}) == EINVAL, B
        msg = L.pn2_last_error()
        assert name.encode() in msg and b"leading dimension" in msg and b"rows" not in msg.replace(
            name.encode(), b""), msg
    # the 64-row entry on the same arguments
    if "forward" in name:
        rc = old(P, 4, P, 9, P, 65, 5, 9, 1e-5, 0.1, P, P, P, P, P, 5, P, 5, P, 0, None)
    else:
        rc = old(P, 4, P, 5, P, 9, P, P, P, 65, 5, 9, P, 5, P, 9, P, P, P, 0, None)
    assert rc == EUNSUPPORTED and b"rows" in L.pn2_last_error()


def test_forward_running_statistics_pointers():
    _, L = _L()
    for B in (7, 65):
        for kw in (dict(rm=None), dict(rv=None)):
            assert _fwd(L, B=B, flags=FROZEN, **kw) == EINVAL, kw
            assert b"running_mean" in L.pn2_last_error()
            assert _fwd(L, B=B, momentum=0.1, **kw) == EINVAL, kw
            assert b"running_mean" in L.pn2_last_error()


def test_backward_gradient_pointers():
    _, L = _L()
    for B in (7, 65):
        for kw in (dict(dgamma=None), dict(dbeta=None)):
            assert _bwd(L, B=B, **kw) == EINVAL, kw
            assert b"null pointer" in L.pn2_last_error()


def test_train_head_rows_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["train_head_rows"] == 0 and tuning.get("train_head_rows") == 0
    assert tuning.HOST_RANGES["train_head_rows"] == (0, 1)
    assert tuning.HOST_DEFAULTS["train_head"] == 0  # no default changes
    with tuning.override(train_head=1, train_head_rows=1):
        assert tuning.get("train_head_rows") == 1 and tuning.get("train_head") == 1
    assert tuning.get("train_head_rows") == 0 and tuning.get("train_head") == 0
    for wrong in (2, -1):
        with pytest.raises(ValueError):
            with tuning.override(train_head_rows=wrong):
                pass
        assert tuning.get("train_head_rows") == 0
    assert "train_head_rows" in tuning.__doc__

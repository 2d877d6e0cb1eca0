"""ABI 19: pn2_bn_relu_group_max_f32 and PN2_LAYER_FROZEN_STATS (the frozen-statistics backward
of pn2_bn_relu_backward_f32).  Argument validation happens before any device call, so these
run without a GPU; pointers are dummy non-null values that are never dereferenced."""
import os
import re

from conftest import ROOT

P = 16  # a non-null pointer


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_abi_19_symbol_and_flag():
    lib, L = _L()
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    assert hasattr(L, "pn2_bn_relu_group_max_f32") and "pn2_bn_relu_group_max_f32" in lib.SIGNATURES
    assert lib.LAYER_FROZEN_STATS == 2 and lib.LAYER_NO_RELU == 1
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_LAYER_FROZEN_STATS\s+2\b", header)
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)


def _max(L, Y=P, G=2, K=4, C=8, ld=8, mean=P, invstd=P, gamma=P, beta=P, out=P, ldo=8, arg=P, flags=0):
    return L.pn2_bn_relu_group_max_f32(Y, G, K, C, ld, mean, invstd, gamma, beta, out, ldo, arg, flags, None)


def test_group_max_validation():
    _, L = _L()
    for name in ("Y", "mean", "invstd", "gamma", "beta", "out", "arg"):
        assert _max(L, **{name: None}) == -1, name
        assert b"pn2_bn_relu_group_max_f32: null pointer" in L.pn2_last_error()
    for kw in (dict(ld=7), dict(ldo=7), dict(K=0), dict(K=-3), dict(C=0), dict(G=-1)):
        assert _max(L, **kw) == -1, kw
        assert b"pn2_bn_relu_group_max_f32: bad shape" in L.pn2_last_error()
    assert _max(L, flags=2) == -1 and b"unknown flags" in L.pn2_last_error()
    assert _max(L, flags=4) == -1 and b"unknown flags" in L.pn2_last_error()
    assert _max(L, G=0) == 0  # nothing to do: no launch


def _bwd(L, flags, sxhat, dbias, ws_bytes=0, K=0):
    """M = 8, C = 4, dense dA (or scattered with K); a workspace of ws_bytes."""
    dA = None if K else P
    return L.pn2_bn_relu_backward_f32(P, 8, 4, 4, P, P, P, P, dA, 4, P if K else None, 4, P if K else None, K,
                                      sxhat, P, 4, P, P, dbias, P, ws_bytes, flags, None)


def test_backward_frozen_flag_validation():
    """The null-pointer check is the entry's first, the workspace check comes after the shape
    checks: a call that reaches "workspace too small" has passed the pointer check."""
    _, L = _L()
    # without the flag a dbias needs the forward's sxhat
    assert _bwd(L, 0, None, P) == -1
    assert b"pn2_bn_relu_backward_f32: null pointer" in L.pn2_last_error()
    assert _bwd(L, 1, None, P) == -1
    assert b"pn2_bn_relu_backward_f32: null pointer" in L.pn2_last_error()
    # with it sxhat is not read: NULL is accepted, dense and scattered, with and without NO_RELU
    for flags in (2, 3):
        for K in (0, 2):
            assert _bwd(L, flags, None, P, K=K) == -1
            assert b"pn2_bn_relu_backward_f32: workspace too small" in L.pn2_last_error(), (flags, K)
    # no dbias: no sxhat needed either way
    assert _bwd(L, 0, None, None) == -1 and b"workspace too small" in L.pn2_last_error()
    # other bits stay unknown
    big = 1 << 20
    assert _bwd(L, 4, P, P, ws_bytes=big) == -1 and b"unknown flags" in L.pn2_last_error()
    assert _bwd(L, 6, None, P, ws_bytes=big) == -1 and b"unknown flags" in L.pn2_last_error()
    # the other pointers are still required with the flag
    rc = L.pn2_bn_relu_backward_f32(P, 8, 4, 4, None, P, P, P, P, 4, None, 4, None, 0, None, P, 4, P, P, P, P,
                                    big, 2, None)
    assert rc == -1 and b"null pointer" in L.pn2_last_error()


def test_eval_grad_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["eval_grad"] == 1 and tuning.get("eval_grad") == 1
    with tuning.override(eval_grad=0):
        assert tuning.get("eval_grad") == 0
    assert tuning.get("eval_grad") == 1

"""csrc/loss.hip's entries (additive to ABI 19): the header block, the ctypes binding, the
argument validation of pn2_log_softmax_rows_f32 / _backward_f32, pn2_criterion_forward_f32 /
_backward_f32 and pn2_meter_update, and the host tuning key train_loss.  Validation happens
before any device call, so these run without a GPU; pointers are dummy non-null values that are
never dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null pointer
EINVAL, EUNSUPPORTED = -1, -2
MAX_B = 1 << 30
ENTRIES = ("pn2_log_softmax_rows_f32", "pn2_log_softmax_rows_backward_f32", "pn2_criterion_forward_f32",
           "pn2_criterion_backward_f32", "pn2_meter_update")
NLL, MSE, L1, BCE = 0, 1, 2, 3
MEAN, SUM = 0, 1
CLS, SIGN, POSE = 0, 1, 2
# the host defaults of the parent commit: none of them moves
PARENT_HOST_DEFAULTS = {
    "pipe_profile": 1, "drain_heads": 2, "geometry_stream": 0, "fc_tail": 1, "force_gather": 0, "tail_streams": 1,
    "geometry_bq": 1, "pipe_fuse": 1, "bq_multi": 1, "eval_grad": 1, "group_backward": 0, "train_gemm": 0,
    "train_head": 0, "train_head_rows": 0,
}


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_block():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    at = header.index("the reductions after the heads' last layer")
    block = header[at:header.index("int pn2_log_softmax_rows_f32", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    for word in ("ONE float64 chain", "row-major", "ascending j", "No float atomics", "2^30", "PN2_EUNSUPPORTED",
                 "pointnet2_cls_ssg.py:40-47", "rotation_ssg.py:40-50", "sign_ssg.py:38-45",
                 "train_classification.py", "train_rotation.py", "train_sign.py:148-153", "invalid"):
        assert word in block, word
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19
    for name, value in (("PN2_LOSS_NLL", lib.LOSS_NLL), ("PN2_LOSS_MSE", lib.LOSS_MSE), ("PN2_LOSS_L1", lib.LOSS_L1),
                        ("PN2_LOSS_BCE", lib.LOSS_BCE), ("PN2_REDUCE_MEAN", lib.REDUCE_MEAN),
                        ("PN2_REDUCE_SUM", lib.REDUCE_SUM), ("PN2_METER_CLS", lib.METER_CLS),
                        ("PN2_METER_SIGN", lib.METER_SIGN), ("PN2_METER_POSE", lib.METER_POSE)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name


def test_lib_exports_and_binds():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in lib.SIGNATURES, name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    from pn2 import losses, metrics, ops
    for fn in (ops.log_softmax_rows_direct, ops.log_softmax_rows_backward_direct, ops.criterion_forward_direct,
               ops.criterion_backward_direct, ops.meter_update_direct, losses.log_softmax, losses.ClsLoss,
               losses.PoseLoss, losses.SignLoss, metrics.ClassificationMeter, metrics.SignMeter,
               metrics.PoseMeter):
        assert callable(fn)


def _ls(L, X=P, ldx=7, Y=P, ldy=7, B=5, K=7):
    return L.pn2_log_softmax_rows_f32(X, ldx, Y, ldy, B, K, None)


def _lsb(L, dY=P, ldd=7, Y=P, ldy=7, dX=P, ldx=7, B=5, K=7):
    return L.pn2_log_softmax_rows_backward_f32(dY, ldd, Y, ldy, dX, ldx, B, K, None)


def _cf(L, kind=MSE, reduction=MEAN, P_=P, ldp=7, T=P, ldt=7, B=5, K=7, loss=P):
    return L.pn2_criterion_forward_f32(kind, reduction, P_, ldp, T, ldt, B, K, loss, None)


def _cb(L, kind=MSE, reduction=MEAN, P_=P, ldp=7, T=P, ldt=7, g=P, B=5, K=7, dP=P, ldd=7):
    return L.pn2_criterion_backward_f32(kind, reduction, P_, ldp, T, ldt, g, B, K, dP, ldd, None)


def _mu(L, kind=POSE, pred=P, ldp=3, target=P, ldt=3, label=P, B=5, D=3, nc=7, acc=P, invalid=P, records=P, slot=0,
        slots=4):
    return L.pn2_meter_update(kind, pred, ldp, target, ldt, label, B, D, nc, acc, invalid, records, slot, slots,
                              None)


CALLS = {
    "pn2_log_softmax_rows_f32": (_ls, ("X", "Y"), ("ldx", "ldy")),
    "pn2_log_softmax_rows_backward_f32": (_lsb, ("dY", "Y", "dX"), ("ldd", "ldy", "ldx")),
    "pn2_criterion_forward_f32": (_cf, ("P_", "T", "loss"), ("ldp", "ldt")),
    "pn2_criterion_backward_f32": (_cb, ("P_", "T", "g", "dP"), ("ldp", "ldt", "ldd")),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_validation(name):
    _, L = _L()
    call, ptrs, lds = CALLS[name]

    def bad(code, text, **kw):
        assert call(L, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    variants = [{}] if "log_softmax" in name else [dict(kind=k, reduction=r) for k in (MSE, L1, BCE) for r in (MEAN, SUM)]
    for v in variants:
        for ptr in ptrs:
            bad(EINVAL, b"null pointer", **{ptr: None}, **v)
        for dim in ("B", "K"):
            bad(EINVAL, b"bad shape", **{dim: 0}, **v)
            bad(EINVAL, b"bad shape", **{dim: -3}, **v)
        for ld in lds:
            bad(EINVAL, b"leading dimension", **{ld: 6}, **v)
        bad(EUNSUPPORTED, b"2^30", B=MAX_B + 1, **v)
    if "log_softmax" in name:
        big = {ld: 2000 for ld in lds}
        bad(EUNSUPPORTED, b"1024", K=1025, **big)
        bad(EUNSUPPORTED, b"1024", K=2000, **big)
    else:
        for kind in (-1, 4):
            bad(EINVAL, b"unknown kind", kind=kind)
        for red in (-1, 2):
            bad(EINVAL, b"unknown reduction", reduction=red)
        # NLL: the target is a vector, its leading dimension is not read
        for red in (MEAN, SUM):
            bad(EINVAL, b"leading dimension", kind=NLL, reduction=red, ldp=6, ldt=0)
            bad(EINVAL, b"null pointer", kind=NLL, reduction=red, T=None, ldt=0)
            bad(EINVAL, b"bad shape", kind=NLL, reduction=red, B=0, ldt=0)
            bad(EUNSUPPORTED, b"2^30", kind=NLL, reduction=red, B=MAX_B + 1, ldt=0)


def test_row_limit_is_2_30():
    """2^30 rows pass the row check (the calls get as far as a leading dimension's PN2_EINVAL)."""
    _, L = _L()
    for name, (call, _, lds) in CALLS.items():
        assert call(L, B=MAX_B, **{lds[0]: 6}) == EINVAL, name
        assert b"leading dimension" in L.pn2_last_error()
    assert _mu(L, B=MAX_B, ldp=2) == EINVAL and b"leading dimension" in L.pn2_last_error()
    assert _ls(L, K=1024, ldx=1023, ldy=1024) == EINVAL and b"leading dimension" in L.pn2_last_error()


def test_meter_validation():
    _, L = _L()
    name = b"pn2_meter_update"

    def bad(code, text, **kw):
        assert _mu(L, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name in msg and text in msg, (kw, msg)

    for kind, D in ((CLS, 1), (SIGN, 1), (POSE, 3)):
        for ptr in ("pred", "target", "acc", "invalid", "records"):
            bad(EINVAL, b"null pointer", kind=kind, D=D, **{ptr: None})
        for dim in ("B", "D", "nc"):
            bad(EINVAL, b"bad shape", kind=kind, **{"D": D, dim: 0})
            bad(EINVAL, b"bad shape", kind=kind, **{"D": D, dim: -2})
        bad(EUNSUPPORTED, b"2^30", kind=kind, D=D, B=MAX_B + 1)
        bad(EUNSUPPORTED, b"num_category", kind=kind, D=D, nc=4097)
        for slot in (-1, 4, 9):
            bad(EINVAL, b"record slot", kind=kind, D=D, slot=slot)
        bad(EINVAL, b"record slot", kind=kind, D=D, slots=0)
    for kind in (SIGN, POSE):
        bad(EINVAL, b"null pointer", kind=kind, D=1 if kind == SIGN else 3, label=None)
    for kind in (CLS, SIGN):
        bad(EINVAL, b"bad shape", kind=kind, D=3)
    bad(EINVAL, b"leading dimension", kind=POSE, ldp=2)
    bad(EINVAL, b"leading dimension", kind=POSE, ldt=2)
    bad(EINVAL, b"leading dimension", kind=SIGN, D=1, ldp=0)
    bad(EUNSUPPORTED, b"D=17", kind=POSE, D=17, ldp=17, ldt=17)
    for kind in (-1, 3):
        bad(EINVAL, b"unknown kind", kind=kind)


def test_train_loss_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["train_loss"] == 0 and tuning.get("train_loss") == 0
    assert tuning.HOST_RANGES["train_loss"] == (0, 1)
    with tuning.override(train_loss=1):
        assert tuning.get("train_loss") == 1
    assert tuning.get("train_loss") == 0
    for wrong in (2, -1):
        with pytest.raises(ValueError):
            with tuning.override(train_loss=wrong):
                pass
        assert tuning.get("train_loss") == 0
    assert "train_loss" in tuning.__doc__
    rest = {k: v for k, v in tuning.HOST_DEFAULTS.items() if k != "train_loss"}
    assert rest == PARENT_HOST_DEFAULTS

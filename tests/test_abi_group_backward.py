"""pn2_group_backward_f32 (additive to ABI 19): the header, the ctypes binding, the entry's
argument validation and the host tuning key group_backward.  Validation happens before any
device call, so these run without a GPU; pointers are dummy non-null values that are never
dereferenced."""
import os
import re

import pytest

from conftest import ROOT

P = 16  # a non-null pointer
BIG = 1 << 30


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_declares_entry_and_abi_stays_19():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"\bint\s+pn2_group_backward_f32\s*\(", header)
    assert re.search(r"\bint64_t\s+pn2_group_backward_workspace_bytes\s*\(", header)
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    # the additive-entry note, in the block that documents this entry
    at = header.index("backward of the grouping")
    block = header[at:header.index("int pn2_group_backward_f32", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    assert re.search(r"#define\s+PN2_INDEX_I64\s+0\b", header) and re.search(r"#define\s+PN2_INDEX_I32\s+1\b", header)
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19


def test_lib_binds_entry():
    lib, L = _L()
    for s in ("pn2_group_backward_f32", "pn2_group_backward_workspace_bytes"):
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert lib.INDEX_I64 == 0 and lib.INDEX_I32 == 1
    # [cnt B*N | start B*N | pos B*S*K] int32, rounded up to 16 bytes
    assert L.pn2_group_backward_workspace_bytes(2, 37, 5, 7) == (4 * (2 * 2 * 37 + 2 * 5 * 7) + 15) // 16 * 16
    assert L.pn2_group_backward_workspace_bytes(2, 0, 5, 7) == -1
    assert L.pn2_group_backward_workspace_bytes(2, 37, 5, 0) == -1
    assert L.pn2_group_backward_workspace_bytes(-1, 37, 5, 7) == -1


def _bwd(L, dg=P, rs=8, off=3, idx=P, dtype=0, B=2, N=37, S=5, K=7, D=5, out=P, ws=P, ws_bytes=BIG):
    return L.pn2_group_backward_f32(dg, rs, off, idx, dtype, S * K, K, 1, B, N, S, K, D, out, ws, ws_bytes, None)


def test_validation():
    _, L = _L()
    for name in ("dg", "idx", "out", "ws"):
        assert _bwd(L, **{name: None}) == -1, name
        assert b"pn2_group_backward_f32: null pointer" in L.pn2_last_error()
    assert _bwd(L, D=0) == -1
    assert b"pn2_group_backward_f32: D == 0" in L.pn2_last_error()
    for kw in (dict(B=-1), dict(N=0), dict(N=-4), dict(S=-1), dict(K=0), dict(K=-2), dict(D=-1),
               dict(off=-1), dict(rs=7)):  # rs=7 < off + D
        assert _bwd(L, **kw) == -1, kw
        assert b"pn2_group_backward_f32: bad shape" in L.pn2_last_error(), kw
    assert _bwd(L, dtype=2) == -1
    assert b"pn2_group_backward_f32: unknown index dtype" in L.pn2_last_error()
    need = L.pn2_group_backward_workspace_bytes(2, 37, 5, 7)
    for short in (0, need - 1):
        assert _bwd(L, ws_bytes=short) == -1
        assert b"pn2_group_backward_f32: workspace too small" in L.pn2_last_error()
    assert _bwd(L, B=0) == 0  # nothing to do: no launch


def test_group_backward_tuning_key():
    from pn2 import tuning
    assert tuning.HOST_DEFAULTS["group_backward"] == 0 and tuning.get("group_backward") == 0
    with tuning.override(group_backward=1):
        assert tuning.get("group_backward") == 1
    assert tuning.get("group_backward") == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            with tuning.override(group_backward=bad):
                pass
        assert tuning.get("group_backward") == 0
    assert "group_backward" in tuning.__doc__

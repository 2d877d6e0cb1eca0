"""pn2_fps2_f32 / pn2_fps2_eligible (two sampling levels in one launch, additive to ABI 19): the
header, the ctypes binding, the eligibility rule and the argument checks -- all before any device
call, so these run without a GPU; pointers are dummy non-null values never dereferenced."""
import os
import re

from conftest import ROOT

P = 16


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def _call(L, pts=P, B=2, N=1024, C=3, start1=P, S1=512, start2=P, S2=128, idx1=P, idx2=P):
    return L.pn2_fps2_f32(pts, B, N, C, N * C, C, 1, start1, S1, start2, S2, idx1, P, P, P, idx2, P, P, P, None)


def test_symbols_and_header():
    lib, L = _L()
    for s in ("pn2_fps2_f32", "pn2_fps2_eligible"):
        assert hasattr(L, s) and s in lib.SIGNATURES
    assert len(lib.SIGNATURES["pn2_fps2_f32"][1]) == 20
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    block = header[header.index("two consecutive sampling levels"):header.index("int pn2_fps2_eligible(")]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19


def test_eligibility_rule():
    """xyz clouds of <= 1024 points, S1 <= 512 (level 2 on at most four waves of two points per
    lane, the records within the LDS budget), under the automatic block choice only."""
    from pn2 import tuning
    _, L = _L()
    e = L.pn2_fps2_eligible
    assert e(1024, 3, 512, 128) == 1 and e(64, 3, 16, 4) == 1 and e(130, 3, 65, 33) == 1
    assert e(1024, 3, 512, 1) == 1 and e(1, 3, 1, 1) == 1
    assert e(1024, 10, 512, 128) == 0      # the pose heads' one-hot clouds
    assert e(1024, 3, 513, 128) == 0       # S1 past the level-2 block / LDS cap
    assert e(1025, 3, 512, 128) == 0 and e(2048, 3, 512, 128) == 0
    assert e(1024, 3, 512, 0) == 0 and e(0, 3, 1, 1) == 0 and e(1024, 3, 0, 1) == 0
    assert e(1024, 3, 512, 8193) == 0
    for keys in (dict(fps_mid=256), dict(fps_threads=256, fps_ppt=4)):
        with tuning.override(**keys):
            assert e(1024, 3, 512, 128) == 0, keys
    assert e(1024, 3, 512, 128) == 1


def test_validation():
    _, L = _L()
    for name in ("pts", "start1", "start2", "idx1", "idx2"):
        assert _call(L, **{name: None}) == -1, name
        assert b"pn2_fps2_f32: null pointer" in L.pn2_last_error()
    for kw in (dict(B=-1), dict(N=0), dict(S1=0), dict(S2=0), dict(C=0)):
        assert _call(L, **kw) == -1, kw
        assert b"pn2_fps2_f32: bad shape" in L.pn2_last_error()
    # ineligible shapes are refused, never run on another kernel behind the caller's back
    for kw in (dict(C=10), dict(S1=513), dict(N=2048)):
        assert _call(L, **kw) == -2, kw
        assert b"not a two-level shape" in L.pn2_last_error()
    assert _call(L, B=0) == 0  # nothing to do: no launch

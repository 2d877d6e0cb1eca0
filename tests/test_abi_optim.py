"""csrc/optim.hip's entries (additive to ABI 19): the header block, the exports, the ctypes
binding, and the argument validation of pn2_adam_step_f32 / pn2_sgd_step_f32.  Validation happens
before any device call, so these run without a GPU; device pointers are dummy non-null values
that are never dereferenced (the host copy of the descriptor table is real host memory)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

P = 4096  # a non-null "device" pointer
EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = ("pn2_adam_step_f32", "pn2_sgd_step_f32")


def _L():
    from pn2 import _lib
    return _lib, _lib.load()


def test_header_block():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    at = header.index("the optimizer step of a train step as one launch")
    block = header[at:header.index("int pn2_adam_step_f32", at)]
    assert "Additive to ABI 19: no existing entry or struct changes, so PN2_ABI_VERSION stays 19." in block
    for word in ("THE SCALARS LIVE IN DEVICE MEMORY", "never in kernel arguments", "THE ARITHMETIC RULE",
                 "correctly rounded", "no contraction", "m  = m + omb1*(g' - m)", "v  = v*beta2",
                 "den = sqrt(v) / bc2_sqrt + eps", "p  = p + ss*(m / den)", "_single_tensor_sgd",
                 "16-byte", "No LDS, no atomics", "2^31", "PN2_EINVAL", "tests/optim_ref.py",
                 "train_classification.py:88-101"):
        assert word in block, word
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+PN2_ABI_VERSION\s+19\b", header)
    assert L.pn2_abi_version() == lib.ABI_VERSION == 19


def test_lib_exports_and_binds():
    lib, L = _L()
    header = open(os.path.join(ROOT, "include", "pn2.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in lib.SIGNATURES, name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    assert L.pn2_optim_chunk() == 2048 and L.pn2_optim_scalars() == 8
    # the descriptor is six 8-byte fields: the host builds the table as an int64 [n][6] array
    assert ctypes.sizeof(lib.OptimTensor) == 48
    assert [f[0] for f in lib.OptimTensor._fields_] == ["p", "g", "m", "v", "n", "scalars"]
    struct = header[header.index("typedef struct pn2_optim_tensor"):header.index("} pn2_optim_tensor;")]
    assert re.findall(r"\b(\w+);", struct) == ["p", "g", "m", "v", "n", "scalars"]
    from pn2 import optim
    assert issubclass(optim.Adam, __import__("torch").optim.Adam)
    assert issubclass(optim.SGD, __import__("torch").optim.SGD)


def _table(lib, rows):
    arr = (lib.OptimTensor * len(rows))()
    for a, r in zip(arr, rows):
        a.p, a.g, a.m, a.v, a.n, a.scalars = r
    return arr


def _call(L, lib, name, rows=((P, P, P, P, 5000, 0),), host=True, dev=P, ntensors=None, jobs=P, njobs=3,
          scalars=P, nblocks=1):
    arr = _table(lib, rows)
    host_ptr = ctypes.addressof(arr) if host else None
    return getattr(L, name)(host_ptr, dev, len(rows) if ntensors is None else ntensors, jobs, njobs, scalars,
                            nblocks, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_validation(name):
    lib, L = _L()
    adam = name == "pn2_adam_step_f32"

    def bad(code, text, **kw):
        assert _call(L, lib, name, **kw) == code, kw
        msg = L.pn2_last_error()
        assert name.encode() in msg and text in msg, (kw, msg)

    for kw in (dict(host=False), dict(dev=None), dict(jobs=None), dict(scalars=None)):
        bad(EINVAL, b"null pointer", **kw)
    for col in (0, 1) + ((2, 3) if adam else ()):
        row = [P, P, P, P, 5000, 0]
        row[col] = None
        bad(EINVAL, b"null pointer in tensor 0", rows=(tuple(row),))
    for n in (0, -1, 1 << 31, 1 << 40):
        bad(EINVAL, b"bad count", rows=((P, P, P, P, n, 0),))
    bad(EINVAL, b"bad count", rows=((P, P, P, P, 100, 0), (P, P, P, P, 0, 0)), njobs=1)
    for ntensors in (0, -2):
        bad(EINVAL, b"bad table length", ntensors=ntensors)
    for nblocks in (0, -1):
        bad(EINVAL, b"bad table length", nblocks=nblocks)
    for idx in (-1, 1, 7):
        bad(EINVAL, b"scalar index", rows=((P, P, P, P, 5000, idx),))
    bad(EINVAL, b"scalar index", rows=((P, P, P, P, 5000, 2),), nblocks=2)
    # 5000 elements are 3 chunks of 2048; 2048 + 2049 elements are 1 + 2
    for njobs in (0, 2, 4, -3):
        bad(EINVAL, b"does not match", njobs=njobs)
    bad(EINVAL, b"does not match", rows=((P, P, P, P, 2048, 0), (P, P, P, P, 2049, 0)), njobs=2)
    # 2^31 - 1 elements pass the count check (the call gets as far as the job table's length)
    bad(EINVAL, b"does not match", rows=((P, P, P, P, (1 << 31) - 1, 0),), njobs=1)


def test_sgd_tensor_without_buffer_is_valid_up_to_the_job_table():
    lib, L = _L()
    # m and v NULL: a tensor without momentum buffer; the check goes on to the table lengths
    assert _call(L, lib, "pn2_sgd_step_f32", rows=((P, P, None, None, 10, 0),), njobs=2) == EINVAL
    assert b"does not match" in L.pn2_last_error()

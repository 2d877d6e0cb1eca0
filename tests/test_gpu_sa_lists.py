"""The fused gather -> MLP -> max call (pn2_sa_mlp_max_f32 / _bf16: csrc/sa_chain.hip, with
sa_dense.hip's layer-0 pre-pass and sa_mlp.hip's fp32 kernels behind it) driven directly through
ops.sa_mlp_max_impl on the hand-built neighbour lists of tests/sa_lists.py, against
oracle.mlp_max(oracle.group(...)) in float64.  No FPS or ball query runs here: the lists put the
compact launch's bookkeeping (compact_scan_kernel's unit table, workgroup descriptors and
straddler zeroing; the chain's pool rows and atomicMax merges) where random geometry rarely
does -- every group at one unit, every group full, a 16-unit group aligned to a workgroup and
shifted by one unit, a group boundary at every offset of a workgroup, unit totals at and one
past a multiple of 16, S above the scan's thread count, shuffled and repeated lists, int64
lists, junk in `out` before the call, and centroids without a neighbour.

Tolerance as test_gpu_mlp.py: 1e-5 relative + 1e-5 of the output's max magnitude (fp32),
2e-2 of the max magnitude (bf16)."""
import copy
import functools

import numpy as np
import pytest
import torch

import sa_lists as sl

pytestmark = pytest.mark.gpu
DEV = "cuda"

_BASE = dict(compact=1, compact_stages=2, compact_pool=16, chain_prepass=1, mlp_f32=0)
# compact_pool = 0: automatic (8 rows where that buys a workgroup per CU); 8: groups past the
# 8th of a workgroup always merge through HBM atomics into rows the scan zeroed
VARIANTS = {
    "default": {},
    "stages3": dict(compact_stages=3),
    "autopool": dict(compact_pool=0),
    "stages3_autopool": dict(compact_stages=3, compact_pool=0),
    "pool8": dict(compact_pool=8),
    "noprepass": dict(chain_prepass=0),
    "noprepass_stages3_autopool": dict(chain_prepass=0, compact_stages=3, compact_pool=0),
    "full": dict(compact=0),
    "full_noprepass": dict(compact=0, chain_prepass=0),
    "f32": dict(mlp_f32=1),
}
COMPACT_VARIANTS = ("default", "stages3", "autopool", "stages3_autopool", "pool8")
WIDE = ("k128wide", "k32wide")  # first layers wide enough for the per-point pre-pass


def _variants_of(name):
    return [v for v in VARIANTS if "noprepass" not in v or name in WIDE]


def _close(got, want, rtol=1e-5):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    atol = rtol * max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


@functools.lru_cache(maxsize=None)
def _device(name, last_beta=None, plant=True):
    """The case's inputs and packed layers on the device."""
    from pn2.pointnet2_utils import _pack_chain
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    pts, feat, ctr = sl.inputs(name, plant)
    sa, convs, bns = sl.module(name, last_beta)
    sa = copy.deepcopy(sa).to(DEV).eval()
    if mode == 1:
        convs, bns = sa.conv_blocks[0], sa.bn_blocks[0]
        packed = _pack_chain(convs, bns, {}, 0, C, False)
    else:
        convs, bns = sa.mlp_convs, sa.mlp_bns
        packed = _pack_chain(convs, bns, {}, C if D else 0, C, True)
    return (pts.to(DEV), None if feat is None else feat.to(DEV), ctr.to(DEV), packed, sa)


def _expected_path(name, variant, with_cnt, precision):
    """What plan_chain decides: the chain serves a compact launch (counts given, 8 < K <= 128)
    and the K whose 32-row slabs stay inside one group; anything else falls to the fp32
    kernels (the dense layers take no grouped source)."""
    from pn2 import _lib
    K = sl.CASES[name][4]
    t = dict(_BASE, **VARIANTS[variant])
    if precision == "bf16":
        return _lib.PATH_BF16
    if t["mlp_f32"]:
        return _lib.PATH_F32
    if (t["compact"] and with_cnt and 8 < K <= 128) or sl.chainable(K):
        return _lib.PATH_SPLIT_BF16
    return _lib.PATH_F32


def _run(name, idx, cnt, variant, precision="fp32", out=None, last_beta=None, plant=True, fill=float("nan"),
         **keys):
    """One call -> out [B*S, cout] (numpy).  A fresh `out` is pre-filled with `fill`, so a row
    the call leaves unwritten, or merges into without zeroing, cannot pass.  keys: further
    tuning keys."""
    from pn2 import _lib, ops, tuning
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    pts, feat, ctr, (wts, als, bes, cins, splits), _ = _device(name, last_beta, plant)
    if out is None:
        out = torch.full((B * S, mlp[-1]), fill, device=DEV)
    with torch.no_grad(), tuning.override(**dict(_BASE, **VARIANTS[variant], **keys)):
        ops.sa_mlp_max_impl(out, mode, pts, feat, ctr, idx.to(DEV), wts, als, bes, cins, splits,
                            precision=precision, cnt=None if cnt is None else cnt.to(DEV))
        torch.cuda.synchronize()
        assert _lib.load().pn2_sa_mlp_last_path() == _expected_path(name, variant, cnt is not None, precision)
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


ALL = [(n, p) for n in sl.CASES for p in sl.patterns_of(n)]
CHAINABLE = [(n, p) for n, p in ALL if sl.chainable(sl.CASES[n][4])]


@pytest.mark.parametrize("name,pattern,variant", [(n, p, v) for n, p in ALL for v in _variants_of(n)])
def test_lists_vs_float64(name, pattern, variant):
    """Every units pattern x list order, under every launch choice (the pre-pass key only where
    the first layer is wide enough for it), against the float64 reference; the kernel family
    that ran is the one the plan predicts.  The "nohit" lists hold centroids without a
    neighbour (cnt = 0, indices N): the reference reads point 0 there."""
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    for order in sl.ORDERS if name in sl.MAIN else ("asc",):
        idx, cnt, want = sl.reference(name, pattern, order)
        got = _run(name, idx, cnt, variant)
        _close(got.reshape(B, S, -1), want)


@pytest.mark.parametrize("name,pattern", ALL)
def test_lists_bf16_vs_float64(name, pattern):
    """The bf16 entry on the same lists: within 2e-2 of the output's max magnitude."""
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    variants = ["default", "stages3_autopool", "pool8"] + (["full"] if sl.chainable(K) else [])
    for order in sl.ORDERS if name in sl.MAIN else ("asc",):
        idx, cnt, want = sl.reference(name, pattern, order)
        for variant in variants:
            got = _run(name, idx, cnt, variant, precision="bf16").reshape(B, S, -1)
            assert np.abs(got - want).max() <= 2e-2 * np.abs(want).max(), (order, variant)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,pattern", CHAINABLE)
def test_compact_bits_equal_full(name, pattern, prec):
    """Where the full launch is the chain kernel too (K = 16 or K % 32 == 0): the compact launch
    under every pool / ring choice, the full launch with the counts given (tuning compact = 0)
    and the call without counts give the same bits.

    This is what holds the split-fp16 activation scales to a row / an 8-row unit
    (sa_chain.hip row_act_scale, unit_act_scale).  With one scale per wave, a value more than
    2^17 below its wave's maximum had its low plane rounded as an fp16 subnormal, so a row's
    last bit depended on the rows sharing its wave -- and the compact launch packs other rows
    into a wave than the full one: k128wide-ramp-fp32 differed in 1 of 9728 elements and
    k32wide-nohit-fp32 in 2 of 10240, by 1 ulp, on the "dup" lists (the planted rows, 50-80x
    the others, widen a wave's range enough), while split bf16 (chain_f16 = 0) was bit-equal."""
    bad = []
    # fp32: the default split-fp16 products, and split bf16 (tuning chain_f16 = 0)
    for f16 in (1, 0) if prec == "fp32" else (1,):
        for order in sl.ORDERS if name in sl.MAIN else ("asc",):
            idx, cnt, _ = sl.reference(name, pattern, order)
            full = _run(name, idx, cnt, "full", prec, chain_f16=f16)
            runs = [("nocnt", _run(name, idx, None, "default", prec, chain_f16=f16))]
            runs += [(v, _run(name, idx, cnt, v, prec, chain_f16=f16)) for v in COMPACT_VARIANTS]
            for variant, got in runs:
                n = int((_bits(got) != _bits(full)).sum())
                if n:
                    ulp = int(np.abs(_bits(got).astype(np.int64) - _bits(full).astype(np.int64)).max())
                    print("%s %s %s f16=%d %s %s: %d of %d elements differ, by at most %d ulp"
                          % (name, pattern, prec, f16, order, variant, n, got.size, ulp))
                    bad.append((f16, order, variant, n, ulp))
    assert not bad, bad


@pytest.mark.parametrize("variant", ["default", "pool8", "full", "f32"])
@pytest.mark.parametrize("name", list(sl.CASES))
def test_int64_and_int32_lists_same_bits(name, variant):
    for pattern in ("ramp", "nohit") if name in sl.MAIN else ("ramp",):
        idx, cnt, _ = sl.reference(name, pattern, "perm" if name in sl.MAIN else "asc")
        assert idx.dtype == torch.int64
        a = _run(name, idx, cnt, variant)
        b = _run(name, idx.to(torch.int32), cnt, variant)
        np.testing.assert_array_equal(_bits(a), _bits(b))


DIRTY = [(n, p) for n, p in ALL if p in ("ones", "full", "ramp", "fill16", "plus1")]


@pytest.mark.parametrize("fill", [3e38, float("nan")])
@pytest.mark.parametrize("name,pattern", DIRTY)
def test_dirty_output_view(name, pattern, fill):
    """`out` as the [:, :cout] view of a buffer 32 columns wider, full of 3e38 / NaN before the
    call: the view gets the bits of a call into a clean buffer (a straddler or overflow row
    whose zeroing were skipped would keep the stale value under atomicMax), and the 32 columns
    beside it keep theirs."""
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    cout = mlp[-1]
    idx, cnt, _ = sl.reference(name, pattern, "asc")
    sentinel = torch.full((B * S, 32), fill).numpy()
    for variant in _variants_of(name):
        clean = torch.zeros(B * S, cout + 32, device=DEV)
        want = _run(name, idx, cnt, variant, out=clean[:, :cout])
        assert not clean[:, cout:].any()
        buf = torch.full((B * S, cout + 32), fill, device=DEV)
        got = _run(name, idx, cnt, variant, out=buf[:, :cout])
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=variant)
        np.testing.assert_array_equal(_bits(buf[:, cout:].cpu().numpy()), _bits(sentinel), err_msg=variant)


ZERO = [(n, p) for n, p in ALL if n in ("k12", "k72", "k128wide", "k32wide", "k16msg", "bigS")
        and p in ("ones", "full", "ramp", "fill16")]


@pytest.mark.parametrize("name,pattern", ZERO)
def test_all_zero_output(name, pattern):
    """The last BatchNorm's shift at -50 on every channel: every row's last activation is 0
    after the ReLU, so every pooled value is exactly 0 -- straddlers and groups past the pool
    rows included, over an `out` full of 3e38."""
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    idx, cnt, want = sl.reference(name, pattern, "asc", -50.0, False)
    assert want.max() == 0.0 and want.min() == 0.0
    for variant in _variants_of(name):
        got = _run(name, idx, cnt, variant, last_beta=-50.0, plant=False, fill=3e38)
        assert (got == 0.0).all(), variant


@pytest.mark.parametrize("name", sl.MAIN)
def test_no_neighbour_rows(name):
    """A centroid without a neighbour (cnt = 0, the ball query's row of N): every family reads
    point 0 of the cloud for an index outside [0, N) -- the chain compact and full, the chain
    behind the dense layer-0 pre-pass, and the fp32 kernels -- so the row's value is the MLP of
    (point 0 - centroid), as the reference with the index mapped to 0."""
    from pn2 import _lib
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    idx, cnt, want = sl.reference(name, "nohit", "asc")
    none = (cnt == 0).numpy()
    assert none.any() and (idx[torch.from_numpy(none)] == N).all()
    point0 = sl.rows_out(name, torch.zeros_like(idx))[:, :, 0]
    np.testing.assert_array_equal(want[none], point0[none])
    for variant in _variants_of(name):
        got = _run(name, idx, cnt, variant).reshape(B, S, -1)
        _close(got, want)
        tol = 1e-5 * np.abs(want[none]) + 1e-5 * np.abs(want).max()
        assert (np.abs(got[none] - want[none]) <= tol).all(), variant
    _lib.device_errors(DEV)  # (nothing here raises the no-neighbour bit; leave the word clean)

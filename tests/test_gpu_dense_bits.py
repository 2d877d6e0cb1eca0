"""Recorded bits of the dense SA layers (csrc/sa_dense.hip: dense_split_kernel, dense_lds_kernel,
dense_pair_kernel).  The three kernels must compute the same bits for the same layer;
tests/test_gpu_mlp.py asserts that they agree with each other, this file that each of them still
produces the bits recorded with the commit named in tests/golden/sa_dense_bits.json (written by
tools/record_sa_dense_bits.py), whatever has been moved into shared helpers since.

Every case is one pn2_sa_mlp_max call through ops.sa_mlp_max_impl under tuning.override, on the
smallest shapes at which a shared piece can go wrong (partial row blocks, every pool mode, slabs
that straddle groups, xyz padding, strided points, signed pooling, the raw pre-pass, a zero job
larger than its launch), at fp32 (tuning dense_f16 0 / 1 / 2) and bf16.  The CRC32 covers the
whole output buffer, its sentinel-filled padding columns included, and the zero side job's
tensor."""
import functools
import json
import os
import zlib

import pytest
import torch

import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sa_dense_bits.json")

# precision -> (entry, tuning dense_f16)
PREC = {"f16_0": ("fp32", 0), "f16_1": ("fp32", 1), "f16_2": ("fp32", 2), "bf16": ("bf16", 1)}
SPLIT = dict(dense_lds=0)


def _lds(tile, stages=3):
    return dict(dense_lds=1, dense_lds_mincin=0, dense_lds_tile=tile, dense_lds_stages=stages)


@functools.lru_cache(maxsize=None)
def _layers(cin, mlp, seed, xyz):
    """The packed layers of a group_all SA module's MLP (test_gpu_mlp.py's builders: module,
    cases.randomize_bn, _pack_chain); every third BN scale of the last layer negated, so that
    the pooled epilogue's row minimum is taken too."""
    import pn2
    from pn2.pointnet2_utils import _pack_chain
    torch.manual_seed(seed)
    sa = pn2.PointNetSetAbstraction(None, None, None, cin, list(mlp), True)
    cases.randomize_bn(sa, seed)
    with torch.no_grad():
        sa.mlp_bns[-1].weight[::3] *= -1
    sa = sa.to(DEV).eval()
    return _pack_chain(sa.mlp_convs, sa.mlp_bns, sa._pack_cache, xyz if cin > xyz else 0, xyz, True)


def _call(mode, mlp, cin, xyz, G, M, pool, flags, prec, seed, **src):
    """One call -> the bytes of the output buffer (32 sentinel columns past the last layer's) and
    of the zero side job's tensor."""
    from pn2 import _lib, ops
    wts, als, bes, cins, splits = _layers(cin, tuple(mlp), seed, xyz)
    buf = torch.full((G if pool else M, mlp[-1] + 32), 7.0, device=DEV)
    zero = src.pop("zero", None)
    ops.sa_mlp_max_impl(buf[:, :mlp[-1]], mode, src.get("points"), src.get("feature"), None, None, wts, als,
                        bes, cins, splits, PREC[prec][0], flags, src.get("rows"), pool, zero=zero)
    torch.cuda.synchronize()
    want = _lib.PATH_BF16 if prec == "bf16" else _lib.PATH_SPLIT_BF16
    assert _lib.load().pn2_sa_mlp_last_path() == want
    return buf.cpu().numpy().tobytes() + (b"" if zero is None else zero.cpu().numpy().tobytes())


def _rows(mlp, B, K, prec, norelu=False, pool=True):
    from pn2 import _lib
    rows = torch.randn(B, K, 64, generator=torch.Generator().manual_seed(B * 1000 + K)).to(DEV)
    flags = [0] * (len(mlp) - 1) + [_lib.LAYER_NO_RELU if norelu else 0]
    return _call(_lib.SRC_ROWS, mlp, 64, 0, B, B * K, pool, flags, prec, 31, rows=rows)


def _group_all(mlp, B, N, C, D, prec, strided=False, pool=True, scale=1.0):
    from pn2 import _lib
    pts = cases.as_layout(cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 40 + N + C),
                          "strided" if strided else "contig").to(DEV)
    feat = (torch.randn(B, N, D, generator=torch.Generator().manual_seed(50 + N + D)) * scale).to(DEV)
    zero = torch.ones(B, C, 1, device=DEV)
    return _call(_lib.SRC_GROUP_ALL, mlp, C + D, C, B, B * N, pool, None, prec, 32 + D, points=pts,
                 feature=feat, zero=zero)


def _prepass(prec):
    """CASES[6] of test_gpu_mlp.py, the smallest chain that takes the layer-0 pre-pass (an MSG
    layer, 99 -> 64 over 2 x 256 points): the raw rows (A.raw) feed the chain kernel."""
    import pn2
    import test_gpu_mlp as M
    from pn2 import _lib
    C, D, K, S, N, mlp, msg, _ = M.CASES[6]
    pts = cases.cloud("uniform3", 2, N, 106)
    feat = torch.randn(2, N, D, generator=torch.Generator().manual_seed(206))
    torch.manual_seed(6)
    sa = pn2.PointNetSetAbstractionMsg(S, [K], [0.35], D, [mlp])
    cases.randomize_bn(sa, 6)
    sa = sa.to(DEV).eval()
    torch.manual_seed(1006)
    with torch.no_grad():
        out = sa(pts.permute(0, 2, 1).contiguous().to(DEV), feat.permute(0, 2, 1).contiguous().to(DEV))[1]
    torch.cuda.synchronize()
    assert _lib.load().pn2_sa_mlp_last_path() == _lib.PATH_SPLIT_BF16
    return out.contiguous().cpu().numpy().tobytes()


# how the last layer of a rows / group_all case pools (sa_dense.hip dense_pool_mode and
# dense_lds_kernel's lds_pool; the kernel trace cannot show a run-time argument, its LDS bytes do)
def _split_pool(K, rows=128):
    if K in (8, 16):
        return "split kernel pool_mode 0: registers, %d register group(s) per output group" % (K // 8)
    if K % 32 == 0 and rows % K == 0:
        return "split kernel pool_mode 1: LDS pool (K %% 32 == 0 and K | %d rows)" % rows
    return "split kernel pool_mode 2: HBM atomics, %s" % (
        "whole slabs (K % 32 == 0)" if K % 32 == 0 else "slabs straddling groups (K % 32 != 0)")


def _lds_pool(K, tile):
    tr = 32 * (tile // 10)
    return "LDS-staged kernel: %s" % ("LDS pool (TR = %d, TR %% K == 0)" % tr if tr % K == 0
                                      else "HBM atomics (TR = %d, K %% TR == 0)" % tr)


POOL_NOTES = {}  # key -> the note, filled by golden_cases (the recorder's routing table)


def golden_cases():
    """[(key, tuning keys, thunk -> bytes)] in a fixed order.  Rows cases: 64 -> 64 -> 128 over M =
    160 rows (one full 128-row block and a partial one; K = 24: 168 rows, the next multiple),
    groups of K."""
    out = []

    def add(name, tune, fn, pool, precs=PREC, pool_bf16=None):
        for prec in precs:
            t = dict(chain_prepass=0, dense_f16=PREC[prec][1])
            t.update(tune)
            key = "%s %s" % (name, prec)
            POOL_NOTES[key] = pool_bf16 if (pool_bf16 and prec == "bf16") else pool
            out.append((key, t, functools.partial(fn, prec=prec)))

    # register-staged: registers (per = 1, 2), the LDS pool, HBM atomics with straddling slabs,
    # one group over two row blocks; hidden rows row-major and in fragment order
    for K in (8, 16, 32, 24, 160):
        for frag in (0, 1):
            add("rows split K%d frag%d" % (K, frag), dict(SPLIT, dense_frag=frag),
                functools.partial(_rows, [64, 128], (168 if K == 24 else 160) // K, K), _split_pool(K))
    # two column tiles per wave, and the 8-wave 256 x 128 tile (fp32 only: bf16 keeps 128 rows)
    for K in (32, 160):
        add("rows split K%d ntc2" % K, dict(SPLIT, dense_minwg=1), functools.partial(_rows, [64, 128], 160 // K, K),
            _split_pool(K))
        add("rows split K%d wide" % K, dict(SPLIT, dense_wide_minwg=1),
            functools.partial(_rows, [64, 128], 160 // K, K), _split_pool(K, 256), pool_bf16=_split_pool(K))
    # LDS-staged: every tile at 2 and 4 stages (44: 128-column tiles need cout % 128 == 0); K = 32
    # pools in LDS (TR % K == 0), K = 512 by HBM atomics (K % TR == 0)
    for tile in (22, 42, 44, 82):
        mlp = [128, 128] if tile == 44 else [64, 128]
        for stages in (2, 4):
            add("rows lds%d s%d K32" % (tile, stages), _lds(tile, stages), functools.partial(_rows, mlp, 5, 32),
                _lds_pool(32, tile))
            add("rows lds%d s%d K512" % (tile, stages), _lds(tile, stages), functools.partial(_rows, mlp, 2, 512),
                _lds_pool(512, tile))
    # an LDS-staged producer writing fragment-ordered rows for a register-staged consumer
    add("rows lds44 fragout K32", _lds(44), functools.partial(_rows, [128, 64], 5, 32), _split_pool(32))
    # group_all: 3 clouds of 50 points (M = 150: a partial last block, clouds straddle slabs); its
    # pooled layer (K = 50) is never eligible for the LDS-staged kernel
    for name, tune in (("split", SPLIT), ("lds22", _lds(22))):
        add("ga N50 " + name, tune, functools.partial(_group_all, [64, 128], 3, 50, 3, 64), _split_pool(50))
        add("ga N50 C10 " + name, tune, functools.partial(_group_all, [64, 128], 3, 50, 10, 64), _split_pool(50))
        add("ga N50 strided " + name, tune, functools.partial(_group_all, [64, 128], 3, 50, 3, 64, strided=True),
            _split_pool(50))
        # clouds of whole 32-row blocks: the first layer's own split-fp16 scale (dense_f16 = 2)
        add("ga N64 " + name, tune, functools.partial(_group_all, [64, 128], 3, 64, 3, 64, scale=30.0),
            _split_pool(64) if name == "split" else _lds_pool(64, 22))
    # signed pooling (the v1 encoder's last layer: BN without ReLU, then the max)
    add("norelu K32 split", SPLIT, functools.partial(_rows, [64, 128], 5, 32, norelu=True),
        _split_pool(32) + ", keys (fkey / funkey)")
    add("norelu K32 lds22", _lds(22), functools.partial(_rows, [64, 128], 5, 32, norelu=True),
        _lds_pool(32, 22) + ", keys (fkey / funkey)")
    add("norelu K160 split", SPLIT, functools.partial(_rows, [64, 128], 1, 160, norelu=True),
        _split_pool(160) + ", keys (fkey, unkey_kernel)")
    add("norelu K512 lds22", _lds(22), functools.partial(_rows, [64, 128], 2, 512, norelu=True),
        _lds_pool(512, 22) + ", keys (fkey, unkey_kernel)")
    # the raw pre-pass of a chain (fp32 chains only), on either dense kernel
    for lds in (0, 1):
        add("prepass lds%d" % lds, dict(chain_prepass=1, dense_lds=lds, dense_lds_mincin=0),
            _prepass, "none in the dense kernel: raw unpooled rows, the chain kernel pools",
            precs=("f16_0", "f16_1", "f16_2"))
    # the fused pair (fp32 only): 2 full 32-row blocks and a 16-row one; alone (rows out), with a
    # pooled third layer (the pair zeroes its pool and writes its maxima), clouds of whole blocks
    # (split fp16), D = 640, and few workgroups against the third layer's pool (N = 33, and N = 65
    # whose last share is clipped).  At bf16 there is no pair: the same layers one launch each.
    fp32 = ("f16_0", "f16_1", "f16_2")

    def pair(name, fn, pool):
        add("pair " + name, dict(dense_pair=1), fn, pool, precs=fp32)
        add("unfused " + name, dict(dense_pair=1), fn, pool, precs=("bf16",))

    pair("N40", functools.partial(_group_all, [256, 512], 2, 40, 3, 256, pool=False), "none: unpooled rows")
    pair("N40 pooled", functools.partial(_group_all, [256, 512, 1024], 2, 40, 3, 256), _split_pool(40))
    pair("N64 pooled", functools.partial(_group_all, [256, 512, 1024], 2, 64, 3, 256, scale=30.0), _lds_pool(64, 22))
    pair("N40 D640", functools.partial(_group_all, [256, 512], 2, 40, 3, 640, pool=False), "none: unpooled rows")
    pair("N33 zero", functools.partial(_group_all, [256, 512, 1024], 1, 33, 3, 256), _split_pool(33))
    pair("N65 zero", functools.partial(_group_all, [256, 512, 1024], 1, 65, 3, 256), _split_pool(65))
    return out


def golden_bits(between=None):
    """{key: CRC32 of the case's bytes}; `between` runs before every case (the recorder's trace
    markers)."""
    from pn2 import tuning
    out = {}
    for key, tune, fn in golden_cases():
        if between:
            between()
        with tuning.override(**tune):
            out[key] = "%08x" % zlib.crc32(fn())
    return out


def test_bits_are_the_recorded_ones():
    """Every case has the bits recorded with the kernels of the commit named in the file."""
    with open(GOLDEN) as f:
        want = json.load(f)["crc32"]
    got = golden_bits()
    assert got.keys() == want.keys()
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, "%d of %d cases differ: %s" % (len(bad), len(want), bad[:8])

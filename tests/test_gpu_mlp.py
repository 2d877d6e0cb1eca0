"""GPU parity of the grouped MLP + max (pn2_sa_mlp_max_f32 through the SA modules) against the
float64 oracle (oracle.mlp_max, pointnet2_utils.py:167-172 / 211-218), for both kernel
families: the split-bf16 register-resident chain (sa_chain.hip, default) and the fp32 MFMA
kernels (PN2_MLP_PATH=f32).  Cases cover every pooling mode of both (K = 8, 16, 32 in
registers; 64, 128 in LDS; 96 through HBM atomics), features absent / unaligned / aligned,
C = 3 and the 10-channel pose layout, SSG and MSG row orders, and a width chain with no chain
signature (served by the fp32 kernels).  Tolerance as test_gpu_sa.py: 1e-5 relative + 1e-5 of
the output's max magnitude."""
import numpy as np
import pytest
import torch

import cases
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (C, D, K, S, N, mlp, msg, chain kernel expected)
CASES = [
    (3, 0, 32, 64, 512, [64, 64, 128], False, True),      # SSG sa1 shape
    (3, 64, 64, 32, 256, [128, 128, 256], False, True),   # SSG sa2 shape, LDS pool
    (3, 13, 16, 32, 256, [32, 32, 64], True, True),       # MSG, unaligned D, K=16
    (3, 8, 8, 40, 256, [64, 96, 128], True, True),        # K=8
    (10, 0, 128, 16, 512, [64, 64, 128], False, True),    # pose layout, K=128
    (3, 4, 96, 8, 256, [64, 64, 128], False, True),       # K=96: HBM atomics
    (3, 96, 32, 32, 256, [64, 64, 128], True, True),      # MSG, wide layer 0 -> pre-pass (T0=2)
    (3, 16, 32, 16, 256, [96, 64, 64], False, False),     # no chain signature -> fp32
    (3, 0, 32, 8, 128, [64, 128], False, False),          # 2 layers -> fp32
]


def _close(got, want, rtol=1e-5):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    atol = rtol * max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


def _oracle_layers(convs, bns):
    out = []
    for conv, bn in zip(convs, bns):
        out.append(dict(W=conv.weight.detach().reshape(conv.weight.shape[0], -1).cpu().numpy(),
                        b=conv.bias.detach().cpu().numpy(), gamma=bn.weight.detach().cpu().numpy(),
                        beta=bn.bias.detach().cpu().numpy(), mean=bn.running_mean.cpu().numpy(),
                        var=bn.running_var.cpu().numpy(), eps=bn.eps))
    return out


@pytest.mark.parametrize("path", ["chain", "chain_noprepass", "f32"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_sa_mlp_vs_oracle(case, path):
    """chain: default dispatch (wide first layers take the per-point layer-0 pre-pass, cases 1,
    6); chain_noprepass: tuning chain_prepass = 0 (layer 0 on the gathered rows); f32: fp32
    MFMA (tuning mlp_f32 = 1)."""
    from pn2 import tuning
    with tuning.override(mlp_f32=int(path == "f32"), chain_prepass=int(path != "chain_noprepass")):
        _sa_mlp_vs_oracle(case, path)


def _sa_mlp_vs_oracle(case, path):
    import pn2
    from pn2 import _lib
    C, D, K, S, N, mlp, msg, chain_ok = CASES[case]
    B, radius = 2, 0.35
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 100 + case)
    gen = torch.Generator().manual_seed(200 + case)
    feat = torch.randn(B, N, D, generator=gen) if D else None
    torch.manual_seed(case)
    if msg:
        sa = pn2.PointNetSetAbstractionMsg(S, [K], [radius], D, [mlp])
        convs, bns = sa.conv_blocks[0], sa.bn_blocks[0]
    else:
        sa = pn2.PointNetSetAbstraction(S, K, radius, C + D, mlp)
        convs, bns = sa.mlp_convs, sa.mlp_bns
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous()
    f = feat.permute(0, 2, 1).contiguous() if D else None
    torch.manual_seed(1000 + case)
    with torch.no_grad():
        newp, newf = sa(x.to(DEV), None if f is None else f.to(DEV))
    torch.cuda.synchronize()
    want_path = _lib.PATH_SPLIT_BF16 if (chain_ok and path != "f32") else _lib.PATH_F32
    assert _lib.load().pn2_sa_mlp_last_path() == want_path

    ps = x.permute(0, 2, 1)  # the module's own (point-contiguous) view
    torch.manual_seed(1000 + case)
    start = torch.randint(0, N, (B,), dtype=torch.long)
    fi = oracle.farthest_point_sample(ps, S, start)
    ctr = oracle.index_points(ps, fi)
    np.testing.assert_array_equal(newp.permute(0, 2, 1).cpu().numpy(), ctr)
    idx = oracle.query_ball_point(radius, K, ps, ctr)
    grouped = oracle.group(ps, feat, idx, ctr, feature_first=msg)
    want = oracle.mlp_max(grouped, _oracle_layers(convs, bns))
    _close(newf.permute(0, 2, 1).cpu().numpy(), want)


@pytest.mark.parametrize("case", [0, 1, 2, 4])
def test_sa_mlp_deterministic(case):
    """Repeated calls on the same inputs give the same bits (no race in the kernels' staging)."""
    import pn2
    C, D, K, S, N, mlp, msg, _ = CASES[case]
    B, radius = 4, 0.35
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 300 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(case)) if D else None
    torch.manual_seed(case)
    if msg:
        sa = pn2.PointNetSetAbstractionMsg(S, [K], [radius], D, [mlp])
    else:
        sa = pn2.PointNetSetAbstraction(S, K, radius, C + D, mlp)
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV) if D else None
    outs = []
    for _ in range(6):
        torch.manual_seed(7)
        with torch.no_grad():
            outs.append(sa(x, f)[1].cpu().numpy())
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])


# compact neighbourhoods (sa_chain.hip pool_mode 3): (C, D, K, S, N, radius, mlp, msg)
COMPACT = [
    (3, 0, 32, 512, 1024, 0.2, [64, 64, 128], False),     # SSG sa1 (about half the rows)
    (3, 128, 64, 128, 512, 0.4, [128, 128, 256], False),  # SSG sa2: pre-pass + compact
    (3, 0, 12, 64, 512, 0.3, [64, 64, 128], False),       # K % 8 != 0
    (3, 0, 72, 40, 256, 2.0, [64, 64, 128], False),       # full groups of 9 units: straddling
    (3, 0, 128, 32, 512, 0.5, [64, 64, 128], False),      # up to 16 units per group
    (3, 13, 16, 64, 512, 0.1, [32, 32, 64], True),        # MSG row order, unaligned features
    (10, 0, 32, 256, 2048, 0.2, [64, 64, 128], False),    # pose layout
    # SSG sa2 shapes with small balls: one-unit groups, 16 groups per workgroup -- past the
    # 8-row LDS pool of the 3-stage-ring launch (PN2_COMPACT_KS=3; merged by HBM atomics into
    # zeroed rows)
    (3, 128, 64, 128, 512, 0.05, [128, 128, 256], False),
    (3, 128, 64, 128, 512, 0.15, [128, 128, 256], False),  # a mix of pooled and overflow groups
]


@pytest.mark.parametrize("pool", [16, 0])  # the full LDS pool (default), or automatic (8 rows where that buys a workgroup)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(COMPACT)))
def test_compact_neighbourhoods_bit_exact(case, prec, pool):
    """Computing only each group's distinct rows (8-row units, the padding repeats of the first
    neighbour dropped) gives the bits of the full K rows per group: every row's MLP is
    computed the same way, and the max is the same without repeats.  Covers K % 8 != 0, groups
    spanning two workgroups (merged by atomicMax into rows the scan zeroed), up to 16 units per
    group, MSG, the pose layout, groups past the LDS pool rows, and bf16; the fp32 result also
    against the float64 oracle."""
    import pn2
    from pn2 import tuning
    C, D, K, S, N, radius, mlp, msg = COMPACT[case]
    stages = 3 if case >= 7 else 2
    B = 3
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 500 + case)
    gen = torch.Generator().manual_seed(600 + case)
    feat = torch.randn(B, N, D, generator=gen) if D else None
    torch.manual_seed(case)
    if msg:
        sa = pn2.PointNetSetAbstractionMsg(S, [K], [radius], D, [mlp])
        convs, bns = sa.conv_blocks[0], sa.bn_blocks[0]
    else:
        sa = pn2.PointNetSetAbstraction(S, K, radius, C + D, mlp)
        convs, bns = sa.mlp_convs, sa.mlp_bns
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV) if D else None
    outs = {}
    chainable = K in (8, 16) or K % 32 == 0
    for mode in ("0", "1") if (chainable or prec == "fp32") else ("1",):
        torch.manual_seed(77)
        with torch.no_grad(), pn2.mlp_precision(prec), \
                tuning.override(compact=int(mode), compact_stages=stages, compact_pool=pool):
            outs[mode] = sa(x, f)[1].cpu().numpy()
    if chainable:  # else the full-row launch is not the chain kernel (no bf16 kernel at all)
        np.testing.assert_array_equal(outs["1"].view(np.uint32), outs["0"].view(np.uint32))
    if prec == "fp32" or not chainable:
        ps = pts.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        torch.manual_seed(77)
        start = torch.randint(0, N, (B,), dtype=torch.long)
        ctr = oracle.index_points(ps, oracle.farthest_point_sample(ps, S, start))
        idx = oracle.query_ball_point(radius, K, ps, ctr)
        want = oracle.mlp_max(oracle.group(ps, feat, idx, ctr, feature_first=msg),
                              _oracle_layers(convs, bns))
        for mode in outs:
            got = outs[mode].transpose(0, 2, 1)
            if prec == "fp32":
                _close(got, want)
            else:  # bf16 operands: 2e-2 of the output's max magnitude
                assert np.abs(got - want).max() <= 2e-2 * np.abs(want).max()


# group_all SA layers (sample_and_group_all + MLP + max over every point, pointnet2_utils.py
# :122-141, :163-172): (C, D, N points = K, mlp, split kernel expected)
GROUP_ALL = [
    (3, 256, 128, [256, 512, 1024], True),   # SSG sa3 (LDS pool)
    (10, 128, 512, [256, 512, 1024], True),  # translation_ssg sa2 (HBM atomics pool)
    (3, 13, 64, [64, 96], True),             # unaligned features, 2 layers
    (3, 0, 16, [64], True),                  # xyz only, one layer, register pool
]


@pytest.mark.parametrize("path", ["split", "f32", "wide"])
@pytest.mark.parametrize("case", range(len(GROUP_ALL)))
def test_group_all_vs_oracle(case, path):
    from pn2 import tuning
    # wide: the 256 x 128 (8-wave) dense tiles of large layers, at a small size
    with tuning.override(mlp_f32=int(path == "f32"), dense_wide_minwg=1 if path == "wide" else 512):
        _group_all_vs_oracle(case, "split" if path == "wide" else path)


def _group_all_vs_oracle(case, path):
    import pn2
    from pn2 import _lib
    C, D, N, mlp, split_ok = GROUP_ALL[case]
    B = 3
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 400 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(500 + case)) if D else None
    torch.manual_seed(case)
    sa = pn2.PointNetSetAbstraction(None, None, None, C + D, mlp, True)
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV) if D else None
    with torch.no_grad():
        newp, newf = sa(x, f)
    torch.cuda.synchronize()
    want_path = _lib.PATH_SPLIT_BF16 if (split_ok and path == "split") else _lib.PATH_F32
    assert _lib.load().pn2_sa_mlp_last_path() == want_path
    assert newp.shape == (B, C, 1) and float(newp.abs().sum()) == 0.0
    rows = pts.numpy() if feat is None else np.concatenate([pts.numpy(), feat.numpy()], -1)
    want = oracle.mlp_max(rows[:, None], _oracle_layers(sa.mlp_convs, sa.mlp_bns))  # [B, 1, cout]
    _close(newf.permute(0, 2, 1).cpu().numpy(), want)


# The LDS-staged dense kernel (sa_dense.hip dense_lds_kernel: 64x64, 128x64 and 128x128 tiles by
# the layer's size) vs dense_split_kernel: the same split, products and k order, so the same bits.
# (C, D, N, mlp, B): SSG sa3 at the metric's B = 32 takes all three tiles (259->256 64x64,
# 256->512 128x64, 512->1024 128x128 + LDS pool); translation_ssg's group_all pools over
# K = 512 > 128 rows through HBM atomics; the v1 encoder's rows source below.
DENSE_LDS = [
    (3, 256, 128, [256, 512, 1024], 32),
    (3, 256, 128, [256, 512, 1024], 5),
    (10, 128, 512, [256, 512, 1024], 4),
    (3, 64, 64, [64, 128], 3),
]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(DENSE_LDS)))
def test_dense_lds_matches_register_staged(case, prec):
    import pn2
    from pn2 import tuning
    C, D, N, mlp, B = DENSE_LDS[case]
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 700 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(800 + case))
    torch.manual_seed(case)
    sa = pn2.PointNetSetAbstraction(None, None, None, C + D, mlp, True)
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV)
    outs = []
    for lds in (1, 0):
        with torch.no_grad(), pn2.mlp_precision(prec), tuning.override(dense_lds=lds, dense_lds_mincin=0):
            outs.append(sa(x, f)[1].cpu().numpy())
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    if prec == "fp32":
        rows = np.concatenate([pts.numpy(), feat.numpy()], -1)
        want = oracle.mlp_max(rows[:, None], _oracle_layers(sa.mlp_convs, sa.mlp_bns))
        _close(outs[0].transpose(0, 2, 1), want)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", range(len(DENSE_LDS)))
def test_dense_frag_rows_bit_identical(case, prec):
    """Hidden rows in MFMA-fragment order (tuning dense_frag = 1, the register-staged kernel's
    default) vs row-major: the same values in another layout -- the same bits, fp32 and bf16,
    including partial 32-row blocks (B = 5 / 3 clouds)."""
    import pn2
    from pn2 import tuning
    C, D, N, mlp, B = DENSE_LDS[case]
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 900 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(910 + case))
    torch.manual_seed(case)
    sa = pn2.PointNetSetAbstraction(None, None, None, C + D, mlp, True)
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV)
    outs = []
    for frag in (1, 0):
        with torch.no_grad(), pn2.mlp_precision(prec), tuning.override(dense_lds=0, dense_frag=frag):
            outs.append(sa(x, f)[1].cpu().numpy())
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# group_all MLPs whose first two layers run as one dense_pair_kernel launch (256 outputs, then a
# multiple of 256): SSG / POSE sa3 (D = 256), MSG sa3 (D = 640), a partial last 32-row block with
# clouds that do not fill whole blocks (N = 40: split bf16 throughout)
DENSE_PAIR = [
    (3, 256, 128, [256, 512, 1024], 32),
    (3, 640, 128, [256, 512, 1024], 6),
    (10, 256, 64, [256, 256, 512], 3),
    (3, 256, 40, [256, 512, 1024], 3),
]


@pytest.mark.parametrize("f16", [2, 1, 0])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("case", range(len(DENSE_PAIR)))
def test_dense_pair_bit_identical(case, lds, f16):
    """The fused first two group_all layers (tuning dense_pair = 1) vs the layers one launch each:
    the same products, accumulation order, scales and epilogues -- the same bits, with the third
    layer on either dense kernel (rows or fragment order) and layer 1 split fp16 or bf16."""
    import pn2
    from pn2 import tuning
    C, D, N, mlp, B = DENSE_PAIR[case]
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 950 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(960 + case)) * (1 + 3 * case)
    torch.manual_seed(case)
    sa = pn2.PointNetSetAbstraction(None, None, None, C + D, mlp, True)
    cases.randomize_bn(sa, case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV)
    outs = []
    for pair in (1, 0):
        with torch.no_grad(), tuning.override(dense_pair=pair, dense_lds=lds, dense_f16=f16):
            outs.append(sa(x, f)[1].cpu().numpy())
    assert np.isfinite(outs[0]).all()
    np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_dense_lds_rows_source_v1():
    """PointNet-v1 encoder MLPs (rows source, unpooled and max over N = 1024 points, the last
    layer signed / without ReLU): LDS-staged == register-staged bits."""
    from pn2 import heads_v1, tuning
    torch.manual_seed(5)
    model = heads_v1.HEADS_V1["pointnet_cls"]()
    cases.randomize_bn(model, 5)
    model = model.to(DEV).eval()
    x = cases.cloud("uniform3", 8, 1024, 9).permute(0, 2, 1).contiguous().to(DEV)
    outs = []
    for lds in (1, 0):
        with torch.no_grad(), tuning.override(dense_lds=lds, dense_lds_mincin=0):
            o = model(x)
            outs.append([t.cpu().numpy() for t in (o if isinstance(o, tuple) else (o,)) if t is not None])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# split-fp16 chains (split_bf16.h NP = 2): accuracy against the float64 oracle, and the power-of-
# two scaling at extreme magnitudes.  (C, D, K, S, N, radius, mlp, msg, case)
F16 = [
    (3, 0, 32, 128, 512, 0.2, [64, 64, 128], False, "plain"),       # SSG sa1: resident layer 0
    (3, 128, 64, 64, 512, 0.4, [128, 128, 256], False, "plain"),    # SSG sa2: pre-pass layer 0
    (3, 0, 32, 64, 512, 0.2, [64, 64, 128], False, "coords_1e3"),   # xyz-ctr up to ~200
    (3, 0, 32, 64, 512, 0.2, [64, 64, 128], False, "coords_1e-4"),  # xyz-ctr ~2e-5
    (3, 0, 32, 64, 512, 0.2, [64, 64, 128], False, "tiny_row"),     # one weight row 1e-6, var 1e-12
    (3, 0, 32, 64, 512, 0.2, [64, 64, 128], False, "hidden_1e4"),   # layer-1 inputs ~1e4
    (3, 0, 32, 64, 512, 0.2, [64, 64, 128], False, "hidden_1e-5"),  # layer-1 inputs ~1e-5
    (3, 0, 16, 64, 512, 0.3, [32, 32, 64], True, "plain"),          # MSG row order (xyz only)
    (3, 96, 32, 32, 256, 0.35, [64, 64, 128], True, "plain"),       # MSG, wide layer 0 -> pre-pass
    (3, 16, 16, 64, 512, 0.3, [32, 32, 64], True, "streamed"),      # streamed layer 0: split bf16
    (3, 128, 64, 64, 512, 0.4, [128, 128, 256], False, "feat_1e4"),  # pre-pass rows ~1e4 (split fp16)
    (3, 128, 64, 64, 512, 0.4, [128, 128, 256], False, "feat_1e-5"),  # pre-pass rows ~1e-5
]


@pytest.mark.parametrize("f16", [2, 1, 0])
@pytest.mark.parametrize("case", range(len(F16)))
def test_chain_split_f16_vs_oracle(case, f16):
    """The fp32-accurate chains run split fp16 (3 MFMAs per product) by default: within 1e-5 of
    the float64 oracle with margin (the worst error stays below a tenth of the tolerance, as the
    6-MFMA split bf16 does), including inputs whose magnitudes leave fp16's range unless both
    operands are scaled: coordinates x1e3 / x1e-4, a weight row of 1e-6 whose BN scale is 1e6,
    hidden activations ~1e4 / ~1e-5.  f16 = 0: tuning chain_f16 = 0 (split bf16); f16 = 2: the
    layer-0 pre-pass in split fp16 as well."""
    import pn2
    from pn2 import _lib, tuning
    C, D, K, S, N, radius, mlp, msg, kind = F16[case]
    B = 2
    scale = {"coords_1e3": 1e3, "coords_1e-4": 1e-4}.get(kind, 1.0)
    pts = cases.cloud("uniform3", B, N, 500 + case) * scale
    radius = radius * scale
    gen = torch.Generator().manual_seed(600 + case)
    feat = torch.randn(B, N, D, generator=gen) if D else None
    if kind in ("feat_1e4", "feat_1e-5"):
        feat *= {"feat_1e4": 1e4, "feat_1e-5": 1e-5}[kind]
    torch.manual_seed(700 + case)
    if msg:
        sa = pn2.PointNetSetAbstractionMsg(S, [K], [radius], D, [mlp])
        convs, bns = sa.conv_blocks[0], sa.bn_blocks[0]
    else:
        sa = pn2.PointNetSetAbstraction(S, K, radius, C + D, mlp)
        convs, bns = sa.mlp_convs, sa.mlp_bns
    cases.randomize_bn(sa, 800 + case)
    with torch.no_grad():
        if kind == "tiny_row":
            convs[1].weight[5] *= 1e-6
            convs[1].bias[5] *= 1e-6
            bns[1].running_mean[5] *= 1e-6
            bns[1].running_var[5] = 1e-12
        if kind == "hidden_1e4":
            bns[0].bias.add_(1e4)
        if kind == "hidden_1e-5":
            bns[0].weight.mul_(1e-5)
            bns[0].bias.mul_(1e-5)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous()
    f = feat.permute(0, 2, 1).contiguous() if D else None
    # f16 = 2: also the layer-0 pre-pass in split fp16 (tuning dense_f16 = 2)
    with tuning.override(chain_f16=int(f16 > 0), dense_f16=2 if f16 == 2 else 1):
        torch.manual_seed(900 + case)
        with torch.no_grad():
            newp, newf = sa(x.to(DEV), None if f is None else f.to(DEV))
        torch.cuda.synchronize()
    assert _lib.load().pn2_sa_mlp_last_path() == _lib.PATH_SPLIT_BF16
    assert _lib.load().pn2_sa_mlp_last_planes() == (2 if f16 and kind != "streamed" else 3)
    ps = x.permute(0, 2, 1)
    torch.manual_seed(900 + case)
    start = torch.randint(0, N, (B,), dtype=torch.long)
    fi = oracle.farthest_point_sample(ps, S, start)
    ctr = oracle.index_points(ps, fi)
    idx = oracle.query_ball_point(radius, K, ps, ctr)
    grouped = oracle.group(ps, feat, idx, ctr, feature_first=msg)
    want = oracle.mlp_max(grouped, _oracle_layers(convs, bns))
    got = newf.permute(0, 2, 1).cpu().numpy().astype(np.float64)
    tol = 1e-5 * np.abs(want) + 1e-5 * np.abs(want).max()
    ratio = float((np.abs(got - want) / tol).max())
    print("case %d %s f16=%d: max err / tol %.4f" % (case, kind, f16, ratio))
    assert ratio < 0.1


# split-fp16 dense layers (sa_dense.hip, NP = 2 for the layers after the first, the activation
# scale from the producing layer's per-(32-row block, 32-column tile) maxima): group_all SA
# layers.  (C, D, N = K, mlp, B, case)
DENSE_F16 = [
    (3, 256, 128, [256, 512, 1024], 4, "plain"),       # SSG sa3 (LDS tiles, LDS pool)
    (10, 128, 512, [256, 512, 1024], 2, "plain"),      # translation_ssg sa2 (HBM atomics pool)
    (3, 64, 64, [64, 128], 3, "plain"),                # register-staged tiles
    (3, 64, 64, [64, 96, 128], 3, "hidden_1e4"),       # layer-1 inputs ~1e4
    (3, 64, 64, [64, 96, 128], 3, "hidden_1e-5"),      # layer-1 inputs ~1e-5
    (3, 64, 64, [64, 96, 128], 3, "tiny_row"),         # one layer-1 weight row 1e-6, var 1e-12
    (3, 64, 64, [64, 96, 128], 3, "cloud_1e4"),        # cloud 1's hidden values 1e4 x cloud 0's
    (3, 61, 64, [64, 128], 3, "K16"),                  # K = 16 points: split bf16 only
    (3, 64, 64, [64, 96, 128], 3, "coords_1e3"),       # layer-0 xyz ~1e3 (its own scale)
    (3, 64, 64, [64, 96, 128], 3, "feat_1e-5"),        # layer-0 features ~1e-5
    (3, 61, 64, [64, 128], 3, "feat_odd"),             # D % 4 != 0: scalar row reads for the scale
]


@pytest.mark.parametrize("f16", [2, 1, 0])
@pytest.mark.parametrize("case", range(len(DENSE_F16)))
def test_dense_split_f16_vs_oracle(case, f16):
    """The fp32-accurate dense layers run split fp16 by default (the first over points with the
    scale of its own rows when a cloud fills whole 32-row blocks, the later ones with the maxima
    their producer wrote): within a tenth
    of the 1e-5 tolerance of the float64 oracle, also at magnitudes outside fp16's range unless
    scaled; a cloud's scale never depends on the other clouds of the batch (cloud_1e4: cloud 0
    alone gives the same bits).  f16 = 0: tuning dense_f16 = 0 (split bf16)."""
    import pn2
    from pn2 import _lib, tuning
    C, D, N, mlp, B, kind = DENSE_F16[case]
    if kind == "K16":
        N = 16
    pts = cases.cloud("onehot10" if C == 10 else "uniform3", B, N, 1400 + case)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(1500 + case))
    if kind == "cloud_1e4":
        feat[1] *= 1e4
    if kind == "coords_1e3":
        pts *= 1e3
    if kind == "feat_1e-5":
        feat *= 1e-5
    torch.manual_seed(1600 + case)
    sa = pn2.PointNetSetAbstraction(None, None, None, C + D, mlp, True)
    cases.randomize_bn(sa, 1700 + case)
    with torch.no_grad():
        if kind == "tiny_row":
            sa.mlp_convs[1].weight[5] *= 1e-6
            sa.mlp_convs[1].bias[5] *= 1e-6
            sa.mlp_bns[1].running_mean[5] *= 1e-6
            sa.mlp_bns[1].running_var[5] = 1e-12
        if kind == "hidden_1e4":
            sa.mlp_bns[0].bias.add_(1e4)
        if kind == "hidden_1e-5":
            sa.mlp_bns[0].weight.mul_(1e-5)
            sa.mlp_bns[0].bias.mul_(1e-5)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV)
    with torch.no_grad(), tuning.override(dense_f16=f16):
        got = sa(x, f)[1].cpu().numpy()
        torch.cuda.synchronize()
        assert _lib.load().pn2_sa_mlp_last_path() == _lib.PATH_SPLIT_BF16
        assert _lib.load().pn2_sa_mlp_last_planes() == (2 if f16 and kind != "K16" else 3)
        if kind == "cloud_1e4":
            alone = sa(x[:1], f[:1])[1].cpu().numpy()
            np.testing.assert_array_equal(alone.view(np.uint32), got[:1].view(np.uint32))
    rows = np.concatenate([pts.numpy(), feat.numpy()], -1)
    want = oracle.mlp_max(rows[:, None], _oracle_layers(sa.mlp_convs, sa.mlp_bns))
    got = got.transpose(0, 2, 1).astype(np.float64)
    tol = 1e-5 * np.abs(want) + 1e-5 * np.abs(want).max(axis=(1, 2), keepdims=True)
    ratio = float((np.abs(got - want) / tol).max())
    print("case %d %s f16=%d: max err / tol %.4f" % (case, kind, f16, ratio))
    assert ratio < 0.1


# S*K not a multiple of the 32-row wave: a cloud's rows then start inside a wave, where a
# per-wave fp16 activation scale would mix two clouds -- those launches must fall back to an
# arithmetic that is batch-independent (VERDICT r05 "what's weak" 2).  Non-compact launches
# (tuning compact = 0) and the default compact ones.  (C, D, K, S, N, radius, mlp)
RAGGED = [
    (3, 0, 24, 50, 256, 0.3, [64, 64, 128]),       # S*K = 1200: 37.5 waves per cloud
    (3, 0, 40, 37, 256, 0.35, [64, 64, 128]),      # S*K = 1480
    (3, 16, 20, 45, 300, 0.4, [64, 64, 128]),      # features (layer 0 over xyz + 16 channels)
    (3, 128, 36, 29, 256, 0.45, [128, 128, 256]),  # wide layer 0 (the pre-pass chains)
]


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("case", range(len(RAGGED)))
def test_chain_ragged_rows_batch_independent(case, compact):
    """Within a tenth of the 1e-5 tolerance of the float64 oracle, and every cloud's output bit-
    equal to the same cloud run alone while its batch neighbour's features are 1e4x larger."""
    import pn2
    from pn2 import tuning
    C, D, K, S, N, radius, mlp = RAGGED[case]
    B = 2
    pts = cases.cloud("uniform3", B, N, 2100 + case)
    gen = torch.Generator().manual_seed(2200 + case)
    feat = torch.randn(B, N, D, generator=gen) if D else None
    if D:
        feat[1] *= 1e4
    torch.manual_seed(2300 + case)
    sa = pn2.PointNetSetAbstraction(S, K, radius, C + D, mlp)
    cases.randomize_bn(sa, 2400 + case)
    sa = sa.to(DEV).eval()
    x = pts.permute(0, 2, 1).contiguous().to(DEV)
    f = feat.permute(0, 2, 1).contiguous().to(DEV) if D else None
    with tuning.override(compact=compact), torch.no_grad():
        torch.manual_seed(2500 + case)
        start = torch.randint(0, N, (B,), dtype=torch.long)
        torch.manual_seed(2500 + case)
        got = sa(x, f)[1]
        torch.cuda.synchronize()
        # cloud 0 alone, with its own start draw (the batch's first)
        from pn2 import shard
        with shard.batch_shard(B, 0):
            torch.manual_seed(2500 + case)
            alone = sa(x[:1], None if f is None else f[:1])[1]
    np.testing.assert_array_equal(alone.cpu().numpy().view(np.uint32), got[:1].cpu().numpy().view(np.uint32))
    ps = pts.permute(0, 2, 1).contiguous().permute(0, 2, 1)  # the module's strided view
    fi = oracle.farthest_point_sample(ps, S, start)
    ctr = oracle.index_points(ps, fi)
    idx = oracle.query_ball_point(radius, K, ps, ctr)
    grouped = oracle.group(ps, None if feat is None else feat.numpy(), idx, ctr, feature_first=False)
    want = oracle.mlp_max(grouped, _oracle_layers(sa.mlp_convs, sa.mlp_bns))
    gotn = got.permute(0, 2, 1).cpu().numpy().astype(np.float64)
    for b in range(B):  # per cloud: cloud 1's magnitude must not set cloud 0's tolerance
        tol = 1e-5 * np.abs(want[b]) + 1e-5 * np.abs(want[b]).max()
        ratio = float((np.abs(gotn[b] - want[b]) / tol).max())
        print("case %d compact %d cloud %d: max err / tol %.4f" % (case, compact, b, ratio))
        assert ratio < 0.1


def test_report_is_per_call():
    """pn2_sa_mlp_last_path / _planes / _fps_side describe the thread's last successful call,
    whichever kernel family ran it: nothing of an earlier call's report leaks into the next, and
    a call that fails validation leaves the report alone."""
    import pn2
    from pn2 import _lib, ops
    from pn2.pointnet2_utils import _pack_chain
    L = _lib.load()

    def report():
        return L.pn2_sa_mlp_last_path(), L.pn2_sa_mlp_last_planes(), L.pn2_sa_mlp_last_fps_side()

    torch.manual_seed(4)
    sa = pn2.PointNetSetAbstraction(16, 16, 0.4, 3, [64, 64, 128])
    cases.randomize_bn(sa, 4)
    sa = sa.to(DEV).eval()
    B, N, S, K = 2, 64, 16, 16
    pts = cases.cloud("uniform3", B, N, 7).to(DEV)
    with torch.no_grad():
        s0 = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(1))
        _, newp, cpk, ppk = ops.fps_direct(pts, S, s0)
        idx, cnt = ops.ball_query_direct(ppk, cpk, 3, 0.4, K, True)
        wts, als, bes, cins, splits = _pack_chain(sa.mlp_convs, sa.mlp_bns, sa._pack_cache, 0, 3, True)
        ref = torch.empty(B * S, 128, device=DEV)
        ops.sa_mlp_max_impl(ref, 0, pts, None, newp, idx, wts, als, bes, cins, splits, cnt=cnt)
        # (a) the chain with an FPS side job that fits its launch
        st = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(2))
        job, outs = ops.fps_side_job(newp, 8, st)
        out = torch.empty_like(ref)
        ops.sa_mlp_max_impl(out, 0, pts, None, newp, idx, wts, als, bes, cins, splits, cnt=cnt, fps_side=job)
        a = report()
        assert (a[0], a[2]) == (_lib.PATH_SPLIT_BF16, 1)
        assert torch.equal(out, ref)
        assert torch.equal(outs[0], ops.fps_direct(newp, 8, st)[0])
        # (b) group_all on a tiny cloud: the dense layers, no side job
        ga = pn2.PointNetSetAbstraction(None, None, None, 3 + 13, [64, 96], True)
        cases.randomize_bn(ga, 5)
        ga = ga.to(DEV).eval()
        feat = torch.randn(B, 13, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
        ga(cases.cloud("uniform3", B, 32, 8).permute(0, 2, 1).contiguous().to(DEV), feat)
        b = report()
        assert (b[0], b[2]) == (_lib.PATH_SPLIT_BF16, -1)
        # (c) no split images: the fp32 kernels
        ops.sa_mlp_max_impl(out, 0, pts, None, newp, idx, wts, als, bes, cins, [], cnt=cnt)
        assert report() == (_lib.PATH_F32, 0, -1)
        # (d) a call that fails validation (output rows narrower than the last layer)
        with pytest.raises(RuntimeError, match="ostride"):
            ops.sa_mlp_max_impl(torch.empty(B * S, 64, device=DEV), 0, pts, None, newp, idx, wts, als, bes,
                                cins, splits, cnt=cnt, fps_side=job)
        assert report() == (_lib.PATH_F32, 0, -1)
        # (e) the bf16 entry on (a)'s shape
        ops.sa_mlp_max_impl(out, 0, pts, None, newp, idx, wts, als, bes, cins, splits, precision="bf16", cnt=cnt)
        assert report() == (_lib.PATH_BF16, 1, -1)
    torch.cuda.synchronize()

"""The two SA modules over their one layer body (pn2.pointnet2_utils._SetAbstraction): the
launches a no_grad forward issues, by ops.kernel_timer's record names, against lists read off
the two separate module bodies this one replaced; and what the reference's heads and the tools
read from the modules -- state_dict keys, and a dict (SSG) or a list of dicts (MSG) as
``_pack_cache``."""
import pytest
import torch

import cases

DEV = "cuda"
B, N = 2, 64
FPS, BQ, MLP = "pn2_fps_f32", "pn2_ball_query_f32", "pn2_sa_mlp_max_f32"


def _ssg():
    import pn2
    return pn2.PointNetSetAbstraction(point_number=16, sample_number=8, radius=0.4, in_channel=3,
                                      mlp=[32, 32, 64])


def _group_all():
    import pn2
    return pn2.PointNetSetAbstraction(None, None, None, 64 + 3, [64, 128], group_all=True)


def _msg():
    import pn2
    return pn2.PointNetSetAbstractionMsg(16, [4, 8], [0.2, 0.4], 0, [[32, 32, 64], [32, 32, 64]])


def _ready(module, seed):
    cases.randomize_bn(module, seed)
    return module.to(DEV).eval()


def _second_forward_names(module, points, feature):
    """Record names of the second of two forwards (the first one packs the weights)."""
    from pn2 import ops
    with torch.no_grad():
        torch.manual_seed(7)
        first = module(points, feature)
        torch.manual_seed(7)
        with ops.kernel_timer() as timer:
            out = module(points, feature)
    torch.cuda.synchronize()
    for a, b in zip(first, out):
        assert torch.equal(a, b)
    return [rec[0] for rec in timer.records], out


@pytest.mark.gpu
def test_ssg_and_group_all_launches():
    torch.manual_seed(31)
    sa, sa_all = _ready(_ssg(), 31), _ready(_group_all(), 32)
    x = cases.cloud("uniform3", B, N, 33).permute(0, 2, 1).contiguous().to(DEV)
    names, (new_points, feature) = _second_forward_names(sa, x, None)
    assert names == [FPS, BQ, MLP]
    assert new_points.shape == (B, 3, 16) and feature.shape == (B, 64, 16)
    names, (zeros, pooled) = _second_forward_names(sa_all, new_points, feature)
    assert names == [MLP]
    assert zeros.shape == (B, 3, 1) and pooled.shape == (B, 128, 1)
    assert not zeros.any()


@pytest.mark.gpu
@pytest.mark.parametrize("bq_multi,queries", [(1, 1), (0, 2)])
def test_msg_launches(bq_multi, queries):
    from pn2 import tuning
    torch.manual_seed(34)
    sa = _ready(_msg(), 34)
    x = cases.cloud("uniform3", B, N, 35).permute(0, 2, 1).contiguous().to(DEV)
    with tuning.override(bq_multi=bq_multi):
        names, (new_points, feature) = _second_forward_names(sa, x, None)
    assert names == [FPS] + [BQ] * queries + [MLP, MLP]
    assert new_points.shape == (B, 3, 16) and feature.shape == (B, 128, 16)


_BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def test_state_dict_keys_and_pack_cache_type():
    sa = _ssg()
    assert list(sa.state_dict()) == (
        ["mlp_convs.%d.%s" % (i, p) for i in range(3) for p in ("weight", "bias")] +
        ["mlp_bns.%d.%s" % (i, p) for i in range(3) for p in _BN])
    assert type(sa._pack_cache) is dict
    msg = _msg()
    assert list(msg.state_dict()) == (
        ["conv_blocks.%d.%d.%s" % (s, i, p) for s in range(2) for i in range(3)
         for p in ("weight", "bias")] +
        ["bn_blocks.%d.%d.%s" % (s, i, p) for s in range(2) for i in range(3) for p in _BN])
    assert type(msg._pack_cache) is list and [type(c) for c in msg._pack_cache] == [dict, dict]

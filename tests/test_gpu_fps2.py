"""Two sampling levels in one launch (pn2_fps2_f32, csrc/fps_body.h fps2_block) and the
standalone launch at level-2 sizes (clouds of up to 512 points): bit for bit what two pn2_fps_f32
launches write (indices, gathered centroids, packed records of both levels), the reference's
goldens where a case has the shape, and the CPU oracle (farthest_point_sample,
pointnet2_utils.py:47-68) everywhere else."""
import numpy as np
import pytest
import torch

import cases
import oracle
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _to_dev_view(p):
    if p.stride(2) == 1:
        return p.contiguous().to(DEV)
    return p.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)


def _bits(t):
    return t.cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.cpu().numpy()


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(("idx", "new_points", "packed centroids", "packed points")[-len(got):], got, want):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="%s: %s" % (what, name))


def _check(p, S1, S2, st1, st2, want1=None):
    """fps2_direct(p) against two fps_direct launches and the oracle (or a golden's level 1)."""
    from pn2 import ops
    dp = _to_dev_view(p)
    d1, d2 = st1.to(DEV), st2.to(DEV)
    r1, r2 = ops.fps2_direct(dp, S1, S2, d1, d2)
    assert ops.last_fps2_path == "two_level"
    s1 = ops.fps_direct(dp, S1, d1)
    s2 = ops.fps_direct(s1[1], S2, d2)
    torch.cuda.synchronize()
    _assert_same(r1, s1, "level 1")
    _assert_same(r2, s2, "level 2")
    if want1 is None:
        want1 = oracle.farthest_point_sample(p, S1, st1)
    np.testing.assert_array_equal(r1[0].cpu().numpy(), want1)
    newp1 = torch.from_numpy(np.ascontiguousarray(oracle.index_points(p, want1)))
    np.testing.assert_array_equal(_bits(r1[1]), newp1.numpy().view(np.uint32))
    want2 = oracle.farthest_point_sample(newp1, S2, st2)
    np.testing.assert_array_equal(r2[0].cpu().numpy(), want2)
    np.testing.assert_array_equal(_bits(r2[1]), oracle.index_points(newp1, want2).view(np.uint32))
    # level 2 samples level 1's packed centroids: its packed input IS that array
    np.testing.assert_array_equal(_bits(r2[3]), _bits(r1[2]))


# partial waves, an S1 that is no multiple of 64 (one, two and four level-2 waves; 64 and 128
# points run level 1 on the 256-thread block), the headline's shape, and S2 = 1 (no iteration)
SHAPES = [(64, 16, 4), (128, 64, 64), (130, 65, 33), (1024, 512, 128), (1024, 512, 1)]


@pytest.mark.parametrize("layout", ["strided", "contig"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,S1,S2", SHAPES)
def test_two_level_equals_two_launches_and_oracle(N, S1, S2, B, layout):
    g = torch.Generator().manual_seed(N * 7 + S2 + B)
    p = cases.as_layout(cases.cloud("uniform3", B, N, 100 + N + B), layout)
    _check(p, S1, S2, torch.randint(0, N, (B,), generator=g), torch.randint(0, S1, (B,), generator=g))


@pytest.mark.parametrize("N,S1,S2", [(1024, 512, 128), (600, 300, 129), (130, 65, 33)])
def test_two_level_duplicate_heavy_cloud(N, S1, S2):
    """Many exact duplicates: every maximum is tied, the first index must win in both levels."""
    g = torch.Generator().manual_seed(N)
    p = cases.as_layout(cases.cloud("dup3", 3, N, 41), "strided")
    _check(p, S1, S2, torch.randint(0, N, (3,), generator=g), torch.randint(0, S1, (3,), generator=g))


@pytest.mark.parametrize("name", ["u3_strided", "dup3_strided"])
def test_two_level_level1_matches_reference_golden(name):
    gd = load_golden("index_%s.npz" % name)
    p = cases.as_layout(torch.from_numpy(gd["points"]), str(gd["layout"]))
    S1 = int(gd["S"])
    st1 = torch.from_numpy(gd["start"])
    st2 = torch.randint(0, S1, (p.shape[0],), generator=torch.Generator().manual_seed(3))
    _check(p, S1, 128, st1, st2, want1=gd["fps_idx"])


@pytest.mark.parametrize("kind,layout", [("uniform3", "strided"), ("uniform3", "contig"), ("dup3", "contig"),
                                         ("onehot10", "strided")])
@pytest.mark.parametrize("S", [128, 1])
@pytest.mark.parametrize("N", [512, 300, 65])
def test_standalone_level2_sizes_vs_oracle(N, S, kind, layout):
    """The standalone launch at level-2 sizes: clouds of 257..512 points leave half of the
    512 x 2 block's point slots empty (65: the one-wave block)."""
    from pn2 import ops
    B = 3
    p = cases.as_layout(cases.cloud(kind, B, N, 7 + N), layout)
    st = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(N + S))
    want = oracle.farthest_point_sample(p, S, st)
    idx, newp, cpk, ppk = ops.fps_direct(_to_dev_view(p), S, st.to(DEV))
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    np.testing.assert_array_equal(_bits(newp), oracle.index_points(p, want).view(np.uint32))
    np.testing.assert_array_equal(_bits(cpk[..., :p.shape[2]]), _bits(newp))


def test_ineligible_shapes_take_two_launches():
    """One-hot clouds, an S1 past the cap and a forced block shape run the two launches, and
    the call says so; the results are the oracle's."""
    from pn2 import ops, tuning
    B = 2
    for kind, N, S1, S2, keys in (("onehot10", 1024, 512, 128, {}), ("uniform3", 1024, 520, 128, {}),
                                  ("uniform3", 1024, 512, 128, {"fps_mid": 256})):
        p = cases.as_layout(cases.cloud(kind, B, N, 5), "strided")
        g = torch.Generator().manual_seed(8)
        st1, st2 = torch.randint(0, N, (B,), generator=g), torch.randint(0, S1, (B,), generator=g)
        with tuning.override(**keys):
            assert not ops.fps2_eligible(N, p.shape[2], S1, S2)
            r1, r2 = ops.fps2_direct(_to_dev_view(p), S1, S2, st1.to(DEV), st2.to(DEV))
        assert ops.last_fps2_path == "separate"
        want1 = oracle.farthest_point_sample(p, S1, st1)
        np.testing.assert_array_equal(r1[0].cpu().numpy(), want1)
        newp1 = torch.from_numpy(np.ascontiguousarray(oracle.index_points(p, want1)))
        np.testing.assert_array_equal(r2[0].cpu().numpy(), oracle.farthest_point_sample(newp1, S2, st2))


def test_pipeline_geometry_path_per_head():
    """The pipeline's geometry chain samples an SSG head's two levels in one launch and keeps an
    MSG head's two launches; both give the eager forward's geometry for the same draws."""
    from pn2 import heads, ops
    from pn2.pipeline import PipelinedForward
    x = cases.cloud("uniform3", 2, 1024, 3).permute(0, 2, 1).contiguous().to(DEV)
    for factory, path in ((heads.ClsSSG, "two_level"), (heads.ClsMSG, "separate")):
        model = cases.build_head(factory, 1).to(DEV)
        pf = PipelinedForward(model)
        with torch.no_grad():
            pf._fps_chain(x)  # launches of >= 64 clouds: the 256 x 4 profile keeps two launches
        assert pf.fps_paths == ["separate"]
        pf.launch_batch = 32  # one B=32 batch per launch (the headline): the automatic blocks
        torch.manual_seed(11)
        with torch.no_grad():
            entries = pf._fps_chain(x)
        assert pf.fps_paths == [path]
        torch.manual_seed(11)
        st1, st2 = torch.randint(0, 1024, (2,)), torch.randint(0, 512, (2,))
        s1 = ops.fps_direct(x.permute(0, 2, 1), 512, st1.to(DEV))
        s2 = ops.fps_direct(s1[1], 128, st2.to(DEV))
        (_, n1, c1, p1, _), (_, n2, c2, p2, _) = list(entries.values())[:2]
        _assert_same((n1, c1, p1), s1[1:], "%s sa1" % path)
        _assert_same((n2, c2, p2), s2[1:], "%s sa2" % path)

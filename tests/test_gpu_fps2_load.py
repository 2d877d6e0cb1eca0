"""The two-level FPS launch beside other kernels: launched on a high-priority stream while SA
chain kernels run on another stream (the pipelines' geometry streams), it gives the quiet result
every time -- the same load and pass rule as tests/test_gpu_fps_load.py (0 wrong of 15 launches).
Level 2's exchange runs on the waves its points need while the others only attend the barrier,
so this is the guard for that exchange when the chip is shared.  Reference:
pointnet2_utils.py:47-68."""
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_two_level_fps_deterministic_beside_chain_launches():
    import pn2
    from pn2 import ops
    from pn2.pointnet2_utils import _pack_chain
    torch.manual_seed(4)
    sa = pn2.PointNetSetAbstraction(512, 32, 0.2, 3, [64, 64, 128])
    cases.randomize_bn(sa, 4)
    sa = sa.to(DEV).eval()
    B, N = 32, 1024
    pts = cases.cloud("uniform3", B, N, 7).permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    lo, hi = torch.cuda.Stream.priority_range()
    s_hi = torch.cuda.Stream(DEV, priority=min(lo, hi))
    s_lo = torch.cuda.Stream(DEV)
    with torch.no_grad():
        s0 = torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(1)).to(DEV)
        st = torch.randint(0, 512, (B,), generator=torch.Generator().manual_seed(9)).to(DEV)
        # the quiet result: the two separate launches, alone on the chip
        q1 = ops.fps_direct(pts, 512, s0)
        q2 = ops.fps_direct(q1[1], 128, st)
        _, newp, cpk, ppk = q1
        idx, cnt = ops.ball_query_direct(ppk, cpk, 3, 0.2, 32, True)
        wts, als, bes, cins, splits = _pack_chain(sa.mlp_convs, sa.mlp_bns, sa._pack_cache, 0, 3, True)
        out = torch.empty(B * 512, 128, device=DEV)
        torch.cuda.synchronize()
        bad = 0
        for _ in range(15):
            s_lo.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_lo):
                for _ in range(3):
                    ops.sa_mlp_max_impl(out, 0, pts, None, newp, idx, wts, als, bes, cins, splits, cnt=cnt)
            with torch.cuda.stream(s_hi):
                g1, g2 = ops.fps2_direct(pts, 512, 128, s0, st)
            assert ops.last_fps2_path == "two_level"
            torch.cuda.synchronize()
            ok = all(torch.equal(a, b) for a, b in zip(g1 + g2, q1 + q2))
            bad += 0 if ok else 1
        assert bad == 0, "%d of 15 two-level FPS launches beside the chains differ" % bad

"""pn2_group_backward_f32 / ops.group_backward_direct / the group_backward route of
train._GroupTrain.backward: every point's feature gradient is the float32 sum of the grouped
rows that name it, taken in ascending (s, k) position order from +0.0.

Oracle, on host copies in float32:  out = zeros(B*N, D); np.add.at(out, wrapped flat index,
rows in position order).  Every comparison is np.array_equal on a uint32 view of the bits (signed
zeros and NaN payloads cannot hide behind ==).

Gradient values: a seeded normal, each row scaled by a power of two from 2^-20 to 2^20, so that
another order of the same rows changes bits.  Checked on the CPU for every case below (the real
shapes with the CPU oracle's ball-query lists of the same seeded clouds): the position-order sum
and the reverse-order sum differ in at least one output word of every case -- odd_c3 10,
odd_c3_ff 9, odd_c10 1, odd_c10_ff 2 (of 370; lists of 3 to 5 rows), same / same_vec 6 (of the 8
words of the one point that has rows), padded 27, wrap 1, wrap_vec 2, long 5 (of 6), sa2 73372 of
131072, msg 91206 and msg_vec 89514 of 163840 -- so the reversed order fails every case; and
torch's CPU index_add_ gives the oracle's bits in all of them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cases
from test_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name -> (B, N, S, K, D, C, feature_first, lists)
CASES = {
    # odd everything, D no multiple of 4; offsets 3 / 10 / 0 and row strides 8 / 15
    "odd_c3": (2, 37, 5, 7, 5, 3, False, "random"),
    "odd_c3_ff": (2, 37, 5, 7, 5, 3, True, "random"),
    "odd_c10": (2, 37, 5, 7, 5, 10, False, "random"),
    "odd_c10_ff": (2, 37, 5, 7, 5, 10, True, "random"),
    # every index equal: one point takes S*K rows, the other 63 are exactly +0.0
    "same": (2, 64, 4, 8, 4, 3, False, "same"),
    "same_vec": (2, 64, 4, 8, 4, 4, False, "same"),  # offset 4, stride 8: 16-byte loads
    # lists padded as the ball query pads them, destinations on both sides of point 64 and 128
    "padded": (1, 130, 3, 16, 33, 3, False, "padded"),
    # int64, negative indices, a permuted idx view
    "wrap": (2, 96, 6, 8, 8, 3, False, "wrap"),
    "wrap_vec": (2, 96, 6, 8, 8, 4, True, "wrap"),  # offset 0, stride 12: 16-byte loads
    # one list longer than the 64 positions a wave loads at once (and than the 8 rows in flight)
    "long": (1, 70, 9, 16, 6, 3, False, "same"),
    # the real layers
    "sa2": (2, 512, 128, 64, 128, 3, False, "ball"),
    "msg": (1, 512, 128, 64, 320, 3, True, "ball"),
    "msg_vec": (1, 512, 128, 64, 320, 4, True, "ball"),  # 16-byte loads, two passes over D
}
VEC = ("same_vec", "wrap_vec", "msg_vec")


def rows(B, S, K, W, seed):
    """[B,S,K,W] float32: N(0,1), each row times 2^e, e uniform in -20..20."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, S, K, W), dtype=np.float32)
    e = g.integers(-20, 21, size=(B, S, K, 1))
    return x * np.exp2(e).astype(np.float32)


def ball_lists(B, N, S, K, seed):
    """int64 [B,S,K] device lists of ops.ball_query_direct (radius 0.4) around FPS centroids of a
    seeded unit-sphere cloud."""
    from pn2 import ops
    pts = cases.cloud("uniform3", B, N, seed).to(DEV)
    _, _, cpk, ppk = ops.fps_direct(pts, S, torch.zeros(B, dtype=torch.long, device=DEV))
    return ops.ball_query_direct(ppk, cpk, 3, 0.4, K)


def lists(name):
    """The case's idx as a device tensor [B,S,K] (dtype and strides as the case says)."""
    B, N, S, K, D, C, ff, kind = CASES[name]
    g = np.random.default_rng(len(name) + B * N)
    if kind == "random":
        return torch.from_numpy(g.integers(0, N, size=(B, S, K))).to(DEV)
    if kind == "same":
        return torch.full((B, S, K), 17, dtype=torch.long, device=DEV)
    if kind == "padded":  # ascending distinct hits, then the first repeated; int32
        idx = np.empty((B, S, K), np.int32)
        for s, (lo, m) in enumerate(((58, 12), (120, 10), (0, 16))):
            idx[:, s, :m] = np.arange(lo, lo + m)
            idx[:, s, m:] = lo
        return torch.from_numpy(idx).to(DEV)
    if kind == "wrap":  # [-N, N), stored [B,K,S]: the [B,S,K] view is not contiguous
        t = torch.from_numpy(g.integers(-N, N, size=(B, K, S))).to(DEV).permute(0, 2, 1)
        assert not t.is_contiguous()
        return t
    return ball_lists(B, N, S, K, 7)


def oracle(dg, idx, N, D, off):
    """np.add.at over host copies; indices outside [-N, N) contribute nothing."""
    B, S, K, _ = dg.shape
    idx = idx.astype(np.int64)
    ok = (idx >= -N) & (idx < N)
    flat = (np.where(idx < 0, idx + N, idx) + np.arange(B).reshape(B, 1, 1) * N)[ok]
    out = np.zeros((B * N, D), np.float32)
    np.add.at(out, flat, dg[..., off:off + D][ok])
    return out.reshape(B, N, D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(dgrouped device, idx device, expected host) -- made once, never modified."""
    B, N, S, K, D, C, ff, _ = CASES[name]
    dg = rows(B, S, K, C + D, 100 + len(name))
    idx = lists(name)
    want = oracle(dg, idx.cpu().numpy(), N, D, 0 if ff else C)
    return torch.from_numpy(dg).to(DEV), idx, want


def launch_into(out, dg, idx, N, D, ff):
    """The C entry writing into the caller's `out` ([B,N,D] contiguous view)."""
    from pn2 import _lib
    L = _lib.load()
    B, S, K, W = dg.shape
    ws = torch.empty(L.pn2_group_backward_workspace_bytes(B, N, S, K), dtype=torch.uint8, device=DEV)
    ib, is_, ik = idx.stride()
    _lib.check(L.pn2_group_backward_f32(
        dg.data_ptr(), dg.stride(2), 0 if ff else W - D, idx.data_ptr(),
        _lib.INDEX_I32 if idx.dtype == torch.int32 else _lib.INDEX_I64, ib, is_, ik, B, N, S, K, D,
        out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dg.device)), "pn2_group_backward_f32")


@pytest.mark.parametrize("name", sorted(CASES))
def test_sum_in_position_order(name):
    from pn2 import _lib, ops
    B, N, S, K, D, C, ff, _ = CASES[name]
    dg, idx, want = case(name)
    if name in VEC:  # what the 16-byte path needs
        assert D % 4 == 0 and (0 if ff else C) % 4 == 0 and (C + D) % 4 == 0 and dg.data_ptr() % 16 == 0
    _lib.device_errors()
    got = ops.group_backward_direct(dg, idx, N, D, ff)
    assert got.shape == (B, N, D) and got.is_contiguous()
    assert _lib.device_errors() == 0
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    if CASES[name][7] == "same":  # the untouched points are +0.0, not -0.0
        rest = np.delete(bits(got.cpu().numpy()), 17, axis=1)
        assert not rest.any()


def test_dispatcher_op_and_fake():
    dg, idx, want = case("odd_c3")
    got = torch.ops.pn2.group_backward(dg, idx, 37, 5, False)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.ops.pn2.group_backward(torch.empty(2, 5, 7, 8, device=DEV),
                                         torch.empty(2, 5, 7, dtype=torch.long, device=DEV), 37, 5, False)
    assert tuple(f.shape) == (2, 37, 5) and f.dtype == torch.float32


def test_out_of_range_index():
    """One index equal to N: PN2_DEVERR_INDEX, every other position still summed bit-exactly,
    nothing written outside dfeat."""
    from pn2 import _lib
    B, N, S, K, D, C, ff, _ = CASES["odd_c3"]
    dg, idx, _ = case("odd_c3")
    idx = idx.clone()
    idx[1, 2, 3] = N
    want = oracle(dg.cpu().numpy(), idx.cpu().numpy(), N, D, C)
    G, n = 1024, B * N * D
    sentinel = -12345.0
    buf = torch.full((G + n + G,), sentinel, device=DEV)
    _lib.device_errors()
    launch_into(buf[G:G + n], dg, idx, N, D, ff)
    assert _lib.device_errors() == _lib.DEVERR_INDEX
    host = buf.cpu().numpy()
    assert np.array_equal(bits(host[G:G + n].reshape(B, N, D)), bits(want))
    guard = bits(np.full(G, sentinel, np.float32))
    assert np.array_equal(bits(host[:G]), guard) and np.array_equal(bits(host[G + n:]), guard)


@pytest.mark.parametrize("name", ["odd_c10_ff", "padded", "wrap_vec"])
def test_full_write(name):
    B, N, S, K, D, C, ff, _ = CASES[name]
    dg, idx, want = case(name)
    out = torch.full((B, N, D), float("nan"), device=DEV)
    launch_into(out, dg, idx, N, D, ff)
    host = out.cpu().numpy()
    assert not np.isnan(host).any()
    assert np.array_equal(bits(host), bits(want))


def test_repeatable():
    from pn2 import ops
    B, N, S, K, D, C, ff, _ = CASES["sa2"]
    dg, idx, _ = case("sa2")
    a = ops.group_backward_direct(dg, idx, N, D, ff).cpu().numpy()
    b = ops.group_backward_direct(dg, idx, N, D, ff).cpu().numpy()
    assert np.array_equal(bits(a), bits(b))


def _sa_step(mod, pts, feat0, R, key):
    """One forward + backward of the layer under tuning key group_backward=key ->
    (feature.grad [B,D,N], the grouped tensor's gradient, the neighbour lists)."""
    from pn2 import train, tuning
    cap = {}
    orig = train.group_train

    def spy(points, idx, centers, feature, feature_first):
        g = orig(points, idx, centers, feature, feature_first)
        assert g is not None, "the grouping Function did not apply"
        cap["idx"] = idx
        g.register_hook(lambda gr: cap.__setitem__("dg", gr.detach().clone()))
        return g

    feat = feat0.clone().requires_grad_(True)
    train.group_train = spy
    try:
        with tuning.override(group_backward=key):
            torch.manual_seed(5)  # the FPS start draw
            _, new_feature = mod(pts, feat)
            (new_feature * R).sum().backward()
    finally:
        train.group_train = orig
    return feat.grad, cap["dg"], cap["idx"]


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_through_autograd(mode):
    from pn2 import pointnet2_utils as P
    B, N, D = 2, 512, 128
    torch.manual_seed(3)
    mod = P.PointNetSetAbstraction(128, 64, 0.4, D + 3, [32, 32, 64])
    cases.randomize_bn(mod, 4)
    mod = mod.to(DEV).train(mode == "train")
    pts = cases.cloud("uniform3", B, N, 9).permute(0, 2, 1).contiguous().to(DEV)
    g = torch.Generator().manual_seed(10)
    feat0 = torch.randn(B, D, N, generator=g).to(DEV)
    R = torch.randn(B, 64, 128, generator=g).to(DEV)
    grad1, dg, idx = _sa_step(mod, pts, feat0, R, 1)
    assert tuple(dg.shape) == (B, 128, 64, D + 3)
    flat = (idx.cpu().long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    want = torch.zeros(B * N, D).index_add_(0, flat, dg.cpu()[..., 3:].reshape(-1, D)).view(B, N, D)
    assert np.array_equal(bits(grad1.permute(0, 2, 1).cpu().numpy()), bits(want.numpy()))
    # index_add_ on the device: the same sums in another order (tests/test_train.py's bar for
    # this gradient)
    grad0, _, _ = _sa_step(mod, pts, feat0, R, 0)
    close(grad0.cpu().numpy(), grad1.cpu().numpy(), 1e-3, "feature grad, group_backward 0 vs 1")


def test_deterministic_flag_takes_the_kernel():
    """torch.use_deterministic_algorithms(True) with the key at 0: the Function runs the kernel."""
    from pn2 import ops, train, tuning
    B, N, S, K, D, C, ff, _ = CASES["padded"]
    dg, idx, want = case("padded")
    assert tuning.get("group_backward") == 0
    feature = torch.randn(B, N, D, device=DEV, requires_grad=True)
    points = torch.randn(B, N, C, device=DEV)
    centers = torch.randn(B, S, C, device=DEV)
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        g = train.group_train(points, idx.long(), centers, feature, ff)
        with ops.kernel_timer() as t:
            g.backward(dg)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert np.array_equal(bits(feature.grad.cpu().numpy()), bits(want))
    assert [r[0] for r in t.records] == ["pn2_group_backward_f32"]

"""pn2.ops' functions over the BatchNorm / ReLU / max sweeps of csrc/train.hip
(bn_train_forward_direct, bn_relu_apply_direct, group_max_direct, bn_relu_backward_direct): what
they hand to the C ABI for a strided view, and that ops.kernel_timer records the launches of
pn2.train's route.  The kernels themselves are judged in tests/test_gpu_train_kernels.py."""
import numpy as np
import pytest
import torch

import cases
import train_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 65


def _abi():
    from pn2 import _lib as lib
    from pn2.ops import _stream
    return lib, lib.load(), _stream


def _strided(C, ints):
    """[M, C] rows of stride C + 4: the left columns of a wider tensor (C = 64: 16-byte aligned
    rows, the 4-column kernels; C = 5: the one-column kernels)."""
    g = torch.Generator().manual_seed(100 + C)
    wide = torch.randint(-3, 4, (M, C + 4), generator=g).float() if ints else torch.randn(M, C + 4, generator=g)
    view = wide.to(DEV)[:, :C]
    assert view.stride() == (C + 4, 1) and not view.is_contiguous()
    return view


def bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("K", [5, 13])
@pytest.mark.parametrize("C", [64, 5])
def test_group_max_direct_reads_a_strided_view(C, K):
    from pn2 import ops
    lib, L, stream = _abi()
    a = _strided(C, True)  # small integers: ties
    G = M // K
    out, arg = ops.group_max_direct(a, K)
    assert out.shape == (G, C) and arg.shape == (G, C) and arg.dtype == torch.int32
    want = torch.empty(G, C, device=DEV)
    want_arg = torch.empty(G, C, dtype=torch.int32, device=DEV)
    lib.check(L.pn2_group_max_f32(a.data_ptr(), G, K, C, C + 4, want.data_ptr(), C, want_arg.data_ptr(),
                                  stream(a)), "pn2_group_max_f32")
    np.testing.assert_array_equal(bits(out), bits(want))
    np.testing.assert_array_equal(arg.cpu().numpy(), want_arg.cpu().numpy())
    ref, ref_arg = tr.group_max(a.cpu().numpy(), K)
    np.testing.assert_array_equal(bits(out), ref.view(np.int32))
    np.testing.assert_array_equal(arg.cpu().numpy(), ref_arg)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("C", [64, 5])
def test_bn_relu_apply_direct_reads_a_strided_view(C, relu):
    from pn2 import ops
    lib, L, stream = _abi()
    y = _strided(C, False)
    g = torch.Generator().manual_seed(C)
    mean, invstd, gamma, beta = (torch.randn(C, generator=g).to(DEV) for _ in range(4))
    A = ops.bn_relu_apply_direct(y, mean, invstd, gamma, beta, relu)
    assert A.shape == (M, C) and A.is_contiguous()
    want = torch.empty(M, C, device=DEV)
    lib.check(L.pn2_bn_relu_apply_f32(y.data_ptr(), M, C, C + 4, mean.data_ptr(), invstd.data_ptr(),
                                      gamma.data_ptr(), beta.data_ptr(), want.data_ptr(), C,
                                      0 if relu else lib.LAYER_NO_RELU, stream(y)), "pn2_bn_relu_apply_f32")
    np.testing.assert_array_equal(bits(A), bits(want))
    assert bool((A >= 0).all()) == relu  # the flag arrived


def _mlp(cin, couts, seed):
    torch.manual_seed(seed)
    dims = [cin] + couts
    convs = [torch.nn.Conv2d(dims[i], dims[i + 1], 1).to(DEV) for i in range(len(couts))]
    bns = [torch.nn.BatchNorm2d(c).to(DEV) for c in couts]
    for b in bns:
        cases.randomize_bn(b, seed + 1)
    return convs, bns


def test_timer_records_the_bn_sweeps():
    """The shapes of test_gpu_train_gemm.py::test_route_records_the_kernels."""
    from pn2 import ops, train
    convs, bns = _mlp(19, [32, 64], 40)
    x = torch.randn(8, 16, 8, 19, device=DEV, requires_grad=True)
    with ops.kernel_timer() as t:
        train.mlp_max_train(x, convs, bns).sum().backward()
    names = [r[0] for r in t.records]
    assert names.count("pn2_bn_train_forward_f32") == 2
    assert names.count("pn2_group_max_f32") == 1
    assert names.count("pn2_bn_relu_backward_f32") == 2
    assert all(r[4] > 0 for r in t.records if r[0] in (
        "pn2_bn_train_forward_f32", "pn2_group_max_f32", "pn2_bn_relu_backward_f32"))  # bytes
    for b in bns:
        b.eval()
    with ops.kernel_timer() as t:
        train.mlp_max_frozen(x, convs, bns).sum().backward()
    names = [r[0] for r in t.records]
    assert names.count("pn2_bn_relu_apply_f32") == 1
    assert names.count("pn2_bn_relu_group_max_f32") == 1
    assert names.count("pn2_bn_relu_backward_f32") == 2
    assert not names.count("pn2_bn_train_forward_f32") and not names.count("pn2_group_max_f32")

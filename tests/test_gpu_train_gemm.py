"""pn2_gemm_nt_f32 / pn2_gemm_nn_f32 / pn2_gemm_tn_f32, their ops and the train_gemm route of
train._MlpMaxTrain (csrc/train_gemm.hip; the contracts are in include/pn2.h).

Accuracy is checked against float64 numpy on host copies, element by element:
    |got - want| <= 2 * (n + 3) * 2^-24 * sum_i |a_i| |b_i|     (n the reduction length; for nt
                                                                 |bias| is added to the sum)
-- the standard bound gamma_n * sum |a_i b_i| of a float32 sum in any order, plus 2^-23 per
product for the split's dropped terms, times 2.  Bit comparisons are np.array_equal on a uint32
view.  Operands are laid out three ways: contiguous, as slices of rows 5 floats wider, and with
every base pointer one float past a 16-byte boundary."""
import copy
import functools

import numpy as np
import pytest
import torch

import cases
from conftest import load_golden
from test_train import _build, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -12345.0
G = 256  # guard band, floats (1 KiB: keeps the matrix base 16-byte aligned)

SHAPES = [(1, 1, 1), (33, 13, 3), (70, 129, 131), (64, 64, 64), (40, 256, 259)]
MODES = ["contig", "ld", "offset"]
KINDS = ["nt", "nn", "tn"]


def _lib():
    from pn2 import _lib as lib
    return lib, lib.load()


def slab_rows():
    return int(_lib()[1].pn2_gemm_tn_slab_rows())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Mat:
    """A [r, c] float32 matrix inside a sentinel-filled device buffer: guard bands before and
    after, leading dimension c (+5 in mode 'ld'), base one float further in mode 'offset'.
    host=None: an output, pre-filled with NaN."""

    def __init__(self, r, c, mode, host=None):
        self.r, self.c = r, c
        self.ld = c + 5 if mode == "ld" else c
        self.off = G + (1 if mode == "offset" else 0)
        self.buf = torch.full((self.off + r * self.ld + G,), SENT, device=DEV)
        view = self.view()
        if host is None:
            view.fill_(float("nan"))
        else:
            view.copy_(torch.from_numpy(np.ascontiguousarray(host, np.float32)))
        self.ptr = self.buf.data_ptr() + 4 * self.off
        if mode == "offset":
            assert self.ptr % 16 == 4
        else:
            assert self.ptr % 16 == 0

    def view(self):
        return self.buf[self.off:self.off + self.r * self.ld].view(self.r, self.ld)[:, :self.c]

    def result(self):
        """The matrix on the host, after checking that nothing outside it changed."""
        host = self.buf.cpu().numpy()
        inside = np.zeros(host.shape, bool)
        rows = self.off + np.arange(self.r)[:, None] * self.ld + np.arange(self.c)[None, :]
        inside[rows.reshape(-1)] = True
        sent = bits(np.float32(SENT))
        assert (bits(host)[~inside] == sent).all(), "a write outside the output matrix"
        return host[rows]


def operands(kind, M, N, K, seed, spread=False):
    """(A, B, bias) host float32 in the entry's shapes.  spread: each column of A and of B times
    its own power of two from 2^-20 to 2^20."""
    g = np.random.default_rng(seed)
    sa, sb = {"nt": ((M, K), (N, K)), "nn": ((M, K), (K, N)), "tn": ((M, N), (M, K))}[kind]
    A = g.standard_normal(sa, dtype=np.float32)
    B = g.standard_normal(sb, dtype=np.float32)
    if spread:
        A = A * np.exp2(g.integers(-20, 21, size=(1, sa[1]))).astype(np.float32)
        B = B * np.exp2(g.integers(-20, 21, size=(1, sb[1]))).astype(np.float32)
    bias = g.standard_normal(N, dtype=np.float32) if kind == "nt" else None
    return A, B, bias


def want_and_bound(kind, A, B, bias):
    """(float64 result, the element-wise error bound)."""
    a, b = A.astype(np.float64), B.astype(np.float64)
    if kind == "nt":
        want, mag, n = a @ b.T, np.abs(a) @ np.abs(b).T, A.shape[1]
        if bias is not None:
            want, mag = want + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    elif kind == "nn":
        want, mag, n = a @ b, np.abs(a) @ np.abs(b), A.shape[1]
    else:
        want, mag, n = a.T @ b, np.abs(a).T @ np.abs(b), A.shape[0]
    return want, 2.0 * (n + 3) * 2.0 ** -24 * mag


def launch(kind, a, b, bias, c, M, N, K):
    """The C entry on Mat operands."""
    lib, L = _lib()
    st = lib.stream_ptr(a.buf.device)
    if kind == "nt":
        lib.check(L.pn2_gemm_nt_f32(a.ptr, a.ld, b.ptr, b.ld, 0 if bias is None else bias.data_ptr(),
                                    c.ptr, c.ld, M, N, K, st), "pn2_gemm_nt_f32")
    elif kind == "nn":
        lib.check(L.pn2_gemm_nn_f32(a.ptr, a.ld, b.ptr, b.ld, c.ptr, c.ld, M, N, K, st), "pn2_gemm_nn_f32")
    else:
        ws = torch.empty(max(int(L.pn2_gemm_tn_workspace_bytes(M, N, K)), 4), dtype=torch.uint8, device=DEV)
        lib.check(L.pn2_gemm_tn_f32(a.ptr, a.ld, b.ptr, b.ld, c.ptr, c.ld, M, N, K, ws.data_ptr(),
                                    int(L.pn2_gemm_tn_workspace_bytes(M, N, K)), st), "pn2_gemm_tn_f32")


def run_case(kind, M, N, K, mode, seed, spread=False, with_bias=True):
    """Launch through the C entry; checks the full write, the guards and gaps and the float64
    bound; prints the worst error / bound ratio."""
    A, B, bias = operands(kind, M, N, K, seed, spread)
    if not with_bias:
        bias = None
    want, bound = want_and_bound(kind, A, B, bias)
    a, b = Mat(*A.shape, mode, A), Mat(*B.shape, mode, B)
    c = Mat(*want.shape, mode)
    bias_d = None if bias is None else torch.from_numpy(bias).to(DEV)
    launch(kind, a, b, bias_d, c, M, N, K)
    got = c.result()
    assert not np.isnan(got).any(), "an output element was not written"
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s M=%d N=%d K=%d %s%s: worst error / bound = %.3f" % (
        kind, M, N, K, mode, " spread" if spread else "", worst))
    assert (err <= bound).all(), "worst error / bound = %.3f" % worst
    # the inputs keep their bits
    assert np.array_equal(bits(a.result()), bits(A)) and np.array_equal(bits(b.result()), bits(B))
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_full_write_guards(kind, M, N, K, mode):
    run_case(kind, M, N, K, mode, seed=M * 7 + N * 3 + K)


@pytest.mark.parametrize("M,N,K", [(33, 13, 3), (70, 129, 131)])
@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_scale_spread(kind, M, N, K):
    """Columns scaled over 2^-20 .. 2^20: the bound is relative to each element's own products,
    so a dropped low plane (2^-16 of a product) misses it at every scale."""
    run_case(kind, M, N, K, "ld", seed=11, spread=True)


def test_nt_without_bias():
    run_case("nt", 33, 13, 3, "offset", seed=5, with_bias=False)


@pytest.mark.parametrize("N,K", [(13, 3), (64, 131)])
@pytest.mark.parametrize("dM", [-1, 0, 1, None])
def test_tn_around_the_slab(dM, N, K):
    R = slab_rows()
    M = 2 * R + 37 if dM is None else R + dM
    run_case("tn", M, N, K, "ld", seed=M + N)


# ------------------------------------------------------------------------------ row independence
@functools.lru_cache(maxsize=None)
def rows_case(kind):
    """300 rows of A, B, bias on the device, and the ops result -- made once, never modified."""
    from pn2 import ops
    A, B, bias = operands(kind, 300, 70, 131, seed=21)
    A, B = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    bias = None if bias is None else torch.from_numpy(bias).to(DEV)
    full = ops.gemm_nt_direct(A, B, bias) if kind == "nt" else ops.gemm_nn_direct(A, B)
    return A, B, bias, full


def _rows(kind, A, B, bias):
    from pn2 import ops
    return ops.gemm_nt_direct(A, B, bias) if kind == "nt" else ops.gemm_nn_direct(A, B)


@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_row_independence(kind):
    A, B, bias, full = rows_case(kind)
    sel = torch.from_numpy(np.random.default_rng(3).permutation(300)[:37]).to(DEV)
    part = _rows(kind, A[sel].contiguous(), B, bias)
    assert np.array_equal(bits(part.cpu().numpy()), bits(full[sel].cpu().numpy()))
    one = _rows(kind, A[211:212], B, bias)
    assert one.shape == (1, 70)
    assert np.array_equal(bits(one.cpu().numpy()), bits(full[211:212].cpu().numpy()))


@pytest.mark.parametrize("kind", ["nt", "nn"])
def test_nan_stays_in_its_row(kind):
    A, B, bias, full = rows_case(kind)
    A2 = A.clone()
    A2[140, 77] = float("nan")
    got = _rows(kind, A2, B, bias).cpu().numpy()
    assert not np.isfinite(got[140]).any()
    keep = np.arange(300) != 140
    assert np.array_equal(bits(got[keep]), bits(full.cpu().numpy()[keep]))


# ------------------------------------------------------------------------------ slab rule
def test_tn_slab_rule():
    from pn2 import ops
    R = slab_rows()
    M, N, K = 2 * R + 37, 64, 131
    A, B, _ = operands("tn", M, N, K, seed=31)
    A, B = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    whole = ops.gemm_tn_direct(A, B).cpu().numpy()
    P = [ops.gemm_tn_direct(A[j * R:(j + 1) * R], B[j * R:(j + 1) * R]).cpu().numpy() for j in range(3)]
    want = np.float32(P[0].astype(np.float64) + P[1] + P[2])
    assert np.array_equal(bits(whole), bits(want))
    # another order of the same partials changes bits somewhere: the rule is observable
    other = np.float32(P[0].astype(np.float32) + P[1] + P[2])
    assert not np.array_equal(bits(other), bits(want))
    # R all-zero rows more: one more partial of +0.0
    A0 = torch.cat([A, torch.zeros(R, N, device=DEV)])
    B0 = torch.cat([B, torch.zeros(R, K, device=DEV)])
    assert np.array_equal(bits(ops.gemm_tn_direct(A0, B0).cpu().numpy()), bits(whole))
    assert np.array_equal(bits(ops.gemm_tn_direct(A, B).cpu().numpy()), bits(whole))


# ------------------------------------------------------------------------------ ops
def test_ops_and_fakes():
    from pn2 import ops
    A, B, bias, full = rows_case("nt")
    assert np.array_equal(bits(torch.ops.pn2.gemm_nt(A, B, bias).cpu().numpy()), bits(full.cpu().numpy()))
    nobias = torch.ops.pn2.gemm_nt(A, B, None)
    assert np.array_equal(bits(nobias.cpu().numpy()), bits(ops.gemm_nt_direct(A, B, None).cpu().numpy()))
    A, B, _, full = rows_case("nn")
    assert np.array_equal(bits(torch.ops.pn2.gemm_nn(A, B).cpu().numpy()), bits(full.cpu().numpy()))
    X = rows_case("nt")[0]  # [300, 131] beside A [300, 131]: A^T X
    assert np.array_equal(bits(torch.ops.pn2.gemm_tn(A, X).cpu().numpy()),
                          bits(ops.gemm_tn_direct(A, X).cpu().numpy()))
    assert ops.gemm_tn_direct(A[:0], X[:0]).abs().sum().item() == 0.0
    # strided views are read in place, other views copied: the same bits
    wide = torch.randn(300, 140, device=DEV)
    a = ops.gemm_nn_direct(wide[:, 3:134], B)
    b = ops.gemm_nn_direct(wide[:, 3:134].contiguous(), B)
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s: torch.empty(*s, device="meta")
        assert tuple(torch.ops.pn2.gemm_nt(e(9, 5), e(7, 5), e(7)).shape) == (9, 7)
        assert tuple(torch.ops.pn2.gemm_nt(e(9, 5), e(7, 5), None).shape) == (9, 7)
        assert tuple(torch.ops.pn2.gemm_nn(e(9, 5), e(5, 7)).shape) == (9, 7)
        assert tuple(torch.ops.pn2.gemm_tn(e(9, 5), e(9, 7)).shape) == (5, 7)


def _mlp(cin, couts, seed, conv=torch.nn.Conv2d, bn=torch.nn.BatchNorm2d):
    torch.manual_seed(seed)
    dims = [cin] + couts
    convs = [conv(dims[i], dims[i + 1], 1).to(DEV) for i in range(len(couts))]
    bns = [bn(c).to(DEV) for c in couts]
    for b in bns:
        cases.randomize_bn(b, seed + 1)
    return convs, bns


@pytest.mark.parametrize("input_grad", [True, False])
def test_route_records_the_kernels(input_grad):
    from pn2 import ops, train, tuning
    convs, bns = _mlp(19, [32, 64], 40)
    x = torch.randn(8, 16, 8, 19, device=DEV, requires_grad=input_grad)
    assert tuning.get("train_gemm") == 0
    with ops.kernel_timer() as t:
        train.mlp_max_train(x, convs, bns).sum().backward()
    assert not [r[0] for r in t.records if r[0].startswith("pn2_gemm")]
    with tuning.override(train_gemm=1), ops.kernel_timer() as t:
        train.mlp_max_train(x, convs, bns).sum().backward()
    names = [r[0] for r in t.records if r[0].startswith("pn2_gemm")]
    assert names.count("pn2_gemm_nt_f32") == 2 and names.count("pn2_gemm_tn_f32") == 2
    assert names.count("pn2_gemm_nn_f32") == (2 if input_grad else 1)
    assert len(names) == (6 if input_grad else 5)


# ------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("name", sorted(cases.TRAIN_CASES))
def test_train_step_matches_reference_with_kernels(name):
    """tests/test_train.py::test_train_step_matches_reference's checks and tolerances with the
    three products on the kernels (train_gemm=1)."""
    from pn2 import ops, tuning
    g = load_golden("train_%s.npz" % name)
    mod, (B, N, D, wseed, fseed) = _build(name)
    mod = mod.cuda()
    pts = torch.from_numpy(g["points"]).cuda()
    feat = None
    if "feature" in g:
        feat = torch.from_numpy(g["feature"]).cuda().requires_grad_(True)
    with tuning.override(train_gemm=1), ops.kernel_timer() as t:
        torch.manual_seed(fseed)
        new_points, new_feature = mod(pts, feat)
        (new_feature * torch.from_numpy(g["R"]).cuda()).sum().backward()
    ran = {r[0] for r in t.records}
    assert {"pn2_gemm_nt_f32", "pn2_gemm_tn_f32"} <= ran, "the GEMM kernels did not run"
    np.testing.assert_array_equal(new_points.detach().cpu().numpy(), g["new_points"])
    close(new_feature.detach().cpu().numpy(), g["new_feature"], 1e-4, "new_feature")
    if feat is not None:
        close(feat.grad.cpu().numpy(), g["feature_grad"], 1e-3, "feature grad")
    for k, p in mod.named_parameters():
        if k.endswith(".bias") and ("conv" in k):  # analytically zero: float noise on both sides
            scale = float(np.abs(g["grad." + k[:-5] + ".weight"]).max())
            assert float(p.grad.abs().max()) <= 1e-4 * scale, k
            continue
        close(p.grad.cpu().numpy(), g["grad." + k], 1e-3, "grad " + k)
    for k, b in mod.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(g["buf." + k]), k
        else:
            close(b.cpu().numpy(), g["buf." + k], 1e-4, k)


def _clear_pairs(h, dim):
    """1 where a group's two largest values are more than 1e-4 relative apart (the rule of
    test_train_mlp_matches_torch_on_device): the two routes' forwards may pick different argmax
    rows at a near-tie and route that pair's gradient to another row -- not an error.  The
    upstream gradient is zeroed there; no tolerance is loosened."""
    top2 = torch.topk(h, 2, dim=dim)[0]
    a, b = top2.select(dim, 0), top2.select(dim, 1)
    return ((a - b) > 1e-4 * (a.abs() + 1e-2)).float()


def _compare_routes(run, mods, R):
    """run(mods) -> (output, leaves) at train_gemm 0 and 1 on copies of the modules; out at 1e-4,
    gradients at 1e-3, statistics at 1e-4, train-mode conv bias within 1e-4 of its weight's."""
    from pn2 import tuning
    res = []
    for key in (0, 1):
        ms = copy.deepcopy(mods)
        with tuning.override(train_gemm=key):
            out, leaves = run(ms)
            (out * R).sum().backward()
        res.append((out.detach(), [l.grad for l in leaves], ms))
    (o0, l0, m0), (o1, l1, m1) = res
    close(o1.cpu(), o0.cpu(), 1e-4, "out")
    for a, b in zip(l1, l0):
        close(a.cpu(), b.cpu(), 1e-3, "input grad")
    for a, b in zip(m1[0] + m1[1], m0[0] + m0[1]):
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            if k == "bias" and not isinstance(a, torch.nn.modules.batchnorm._BatchNorm) and m1[1][0].training:
                assert float(p.grad.abs().max()) <= 1e-4 * float(a.weight.grad.abs().max())
                continue
            close(p.grad.cpu(), q.grad.cpu(), 1e-3, k)
        for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
            close(p.float().cpu(), q.float().cpu(), 1e-4, k)


@pytest.mark.parametrize("pool", [True, False])
def test_v1_shared_mlp_routes_agree(pool):
    from pn2 import train
    B, N = 2, 50
    convs, bns = _mlp(3, [16, 32], 50, torch.nn.Conv1d, torch.nn.BatchNorm1d)
    x0 = torch.randn(B, 3, N, device=DEV)
    with torch.no_grad():
        h = x0
        for c, b in zip(copy.deepcopy(convs), copy.deepcopy(bns)):
            h = torch.relu(b(c(h)))  # [B, 32, N]
    g = torch.Generator().manual_seed(51)
    if pool:
        R = torch.randn(B, 32, generator=g).to(DEV) * _clear_pairs(h, 2)
    else:
        R = torch.randn(B, N, 32, generator=g).to(DEV)

    def run(ms):
        x = x0.clone().requires_grad_(True)
        return train.point_mlp_train(x, ms[0], ms[1], False, pool=pool), [x]

    _compare_routes(run, (convs, bns), R)


def test_frozen_recompute_routes_agree():
    """mlp_max_frozen (the eval-grad backward's recompute) at train_gemm 1 against 0."""
    from pn2 import train
    B, S, K, C = 2, 24, 16, 19
    convs, bns = _mlp(C, [32, 64], 60)
    for b in bns:
        b.eval()
    x0 = torch.randn(B, S, K, C, device=DEV)
    with torch.no_grad():
        h = x0.permute(0, 3, 2, 1)  # [B, C, K, S]
        for c, b in zip(convs, bns):
            h = torch.relu(b(c(h)))
    R = torch.randn(B, 64, S, generator=torch.Generator().manual_seed(61)).to(DEV) * _clear_pairs(h, 2)

    def run(ms):
        x = x0.clone().requires_grad_(True)
        return train.mlp_max_frozen(x, ms[0], ms[1]), [x]

    _compare_routes(run, (convs, bns), R)


# ------------------------------------------------------------------------------ reproducible step
def _two_steps(mod, pts, feat0, R, seed):
    from pn2 import tuning
    state = copy.deepcopy(mod.state_dict())
    out = []
    for _ in range(2):
        mod.load_state_dict(state)
        mod.zero_grad(set_to_none=True)
        feat = feat0.clone().requires_grad_(True)
        with tuning.override(train_gemm=1, group_backward=1):
            torch.manual_seed(seed)  # the FPS start draw
            _, new_feature = mod(pts, feat)
            (new_feature * R).sum().backward()
        step = {"new_feature": new_feature.detach(), "feature grad": feat.grad}
        step.update({"grad " + k: p.grad for k, p in mod.named_parameters()})
        step.update({"buf " + k: b.detach().clone() for k, b in mod.named_buffers()})
        out.append({k: v.cpu().numpy() for k, v in step.items()})
    return out


@pytest.mark.parametrize("which", ["ssg", "msg"])
def test_reproducible_step(which):
    """Two train steps from one state under train_gemm=1, group_backward=1: every output,
    gradient and running statistic bit-identical."""
    from pn2 import pointnet2_utils as P
    if which == "ssg":
        B, N, D = 2, 256, 16
        torch.manual_seed(70)
        mod = P.PointNetSetAbstraction(32, 16, 0.5, 3 + D, [32, 64], False)
        cases.randomize_bn(mod, 71)
        mod = mod.to(DEV).train()
        pts = cases.cloud("uniform3", B, N, 72).permute(0, 2, 1).contiguous().to(DEV)
        g = torch.Generator().manual_seed(73)
        feat0 = torch.randn(B, D, N, generator=g).to(DEV)
        R = torch.randn(B, 64, 32, generator=g).to(DEV)
        seed = 5
    else:
        gold = load_golden("train_msg.npz")
        mod, (B, N, D, wseed, seed) = _build("msg")
        mod = mod.to(DEV)
        pts = torch.from_numpy(gold["points"]).to(DEV)
        feat0 = torch.from_numpy(gold["feature"]).to(DEV)
        R = torch.from_numpy(gold["R"]).to(DEV)
    a, b = _two_steps(mod, pts, feat0, R, seed)
    assert a.keys() == b.keys() and len(a) > 4
    for k in a:
        if a[k].dtype == np.float32:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k
    assert np.abs(a["feature grad"]).max() > 0

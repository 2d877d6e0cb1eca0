"""pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32 (csrc/fc_train.hip, the slab
instantiation of its kernel pair; contract in include/pn2.h), ops.fc_rows_*_direct and the
train_head_rows route of train.linear_bn_train.  The entries are driven by test_gpu_fc_train's
run_entries.

Below the 64-row limit the any-B entries must give the bits of the 64-row entries; above it the
order rules are checked directly: rows of Y against the 64-row forward on chunks of X, every
float64 column sum against an explicit ascending host loop over the GPU's own Y / dY, sampled
dW elements against a host fma chain.  Values are also held against test_gpu_fc_train's float64
formulation at its tolerances (Y: the float32-sum bound; 1e-4 forward, 1e-3 gradients).  The
bits of every output of both pairs are pinned by tests/golden/fc_train_bits.json
(tools/record_fc_train_bits.py)."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from test_gpu_fc_train import (BNS, MOM, OUT, SHAPES, _cls_tail, _routes_agree, _two_model_steps, dvec, make_inputs,
                               max_rows, reference, run_entries)
from test_gpu_train_gemm import bits, want_and_bound
from test_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for k in OUT:
        assert np.array_equal(bits(a[k]), bits(b[k])), "%s %s" % (what, k)


# ------------------------------------------------------------------------------ below the cap
# batch statistics of one row are PN2_EINVAL in both pairs (test_abi_fc_rows)
BELOW = [(B, N, K, bn) for B in (1, 2, 33, 64) for N, K in ((5, 3), (7, 256), (512, 1024)) for bn in BNS
         if not (B == 1 and bn == "batch")]
BELOW += [(33, 5, 1029, bn) for bn in BNS]  # K > 1024: the backward's second pass over dW's columns


@pytest.mark.parametrize("B,N,K,bn", BELOW)
def test_same_bits_as_the_64_row_entries(B, N, K, bn):
    d = make_inputs(B, N, K, seed=B * 11 + N + K)
    for relu in (1, 0):
        same_bits(run_entries(d, bn, relu, "contig", rows=True), run_entries(d, bn, relu, "contig", rows=False),
                  "relu=%d" % relu)


# ------------------------------------------------------------------------------ row independence
@pytest.mark.parametrize("B", [65, 129, 200])
def test_rows_of_y_equal_the_64_row_forward_on_chunks(B):
    from pn2 import ops
    for N, K in ((7, 259), (70, 64)):
        d = make_inputs(B, N, K, seed=B + K)
        X, W, b = dvec(d["X"]), dvec(d["W"]), dvec(d["bias"])
        g, be, rm, rv = (dvec(d[k]) for k in ("gamma", "beta", "rm", "rv"))
        full = ops.fc_rows_forward_direct(X, W, b, None, None, None, None, 0.0, 0.0, False, False)[0].cpu().numpy()
        for r0 in range(0, B, 64):
            part = ops.fc_bn_forward_direct(X[r0:r0 + 64], W, b, None, None, None, None, 0.0, 0.0, False, False)[0]
            assert np.array_equal(bits(part.cpu().numpy()), bits(full[r0:r0 + 64])), (N, K, r0)
        # batch statistics change A, never Y
        Yb = ops.fc_rows_forward_direct(X, W, b, g, be, rm, rv, 1e-5, 0.1, True, False)[0].cpu().numpy()
        assert np.array_equal(bits(Yb), bits(full))


# ------------------------------------------------------------------------------ the order rules
def fma32(a, b, c):
    """float32(a*b + c) with one rounding.  The product of two float32 is exact in float64; the
    float64 sum is made round-to-odd (TwoSum's error term says whether it was inexact), after
    which the rounding to float32 is the single rounding of the exact value."""
    p = float(a) * float(b)
    c = float(c)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    if err != 0.0:
        (i,) = struct.unpack("<q", struct.pack("<d", t))
        if not i & 1:
            i += 1 if (err > 0) == (t > 0) else -1
            (t,) = struct.unpack("<d", struct.pack("<q", i))
    return np.float32(t)


RULE_CASES = [(65, 1, 1), (65, 5, 3), (65, 7, 259), (129, 1, 6), (129, 5, 259), (129, 7, 3), (65, 5, 1029)]


@pytest.mark.parametrize("bn", ["batch", "frozen"])
@pytest.mark.parametrize("B,N,K", RULE_CASES)
def test_column_sums_and_dw_follow_the_rule(B, N, K, bn):
    d = make_inputs(B, N, K, seed=B * 5 + N * 3 + K)
    want = reference(d, bn, 1)
    d["dA"] = want["dA"]  # nothing rides on the side of the ReLU's kink against float64 below
    got = run_entries(d, bn, 1, "contig", rows=True)
    f64 = np.float64
    Y, dY, eps = got["Y"], got["dY"], d["eps"]
    if bn == "batch":
        s, q = np.zeros(N, f64), np.zeros(N, f64)
        for r in range(B):  # ascending rows from +0.0
            v = Y[r].astype(f64)
            s = s + v
            q = q + v * v
        mean = s / f64(B)
        var = np.maximum(q / f64(B) - mean * mean, 0.0)
        invstd = 1.0 / np.sqrt(var + eps)
        unb = var * f64(B) / f64(B - 1)
        rm = ((1.0 - MOM) * d["rm"].astype(f64) + MOM * mean).astype(np.float32)
        rv = ((1.0 - MOM) * d["rv"].astype(f64) + MOM * unb).astype(np.float32)
        mu, is_ = mean.astype(np.float32), invstd.astype(np.float32)
    else:
        rm, rv = d["rm"], d["rv"]
        mu, is_ = d["rm"], (1.0 / np.sqrt(d["rv"].astype(f64) + eps)).astype(np.float32)
    assert np.array_equal(bits(got["stats"][:N]), bits(mu)), "mean"
    assert np.array_equal(bits(got["stats"][N:]), bits(is_)), "invstd"
    assert np.array_equal(bits(got["rm"]), bits(rm)), "running_mean"
    assert np.array_equal(bits(got["rv"]), bits(rv)), "running_var"

    pre = ((Y - mu) * is_) * d["gamma"] + d["beta"]  # float32, each operation rounded
    assert pre.dtype == np.float32
    assert np.array_equal(bits(got["A"]), bits(np.where(pre > 0, pre, np.float32(0)))), "A"
    dXn = np.where(pre > 0, d["dA"], np.float32(0))
    s1, s2, sb, s32 = np.zeros(N, f64), np.zeros(N, f64), np.zeros(N, f64), np.zeros(N, np.float32)
    for r in range(B):
        dr = dXn[r].astype(f64)
        s1 = s1 + dr
        s2 = s2 + dr * ((Y[r].astype(f64) - mu.astype(f64)) * is_.astype(f64))
        sb = sb + dY[r].astype(f64)
        s32 = (s32 + dXn[r]).astype(np.float32)
    assert np.array_equal(bits(got["dbeta"]), bits(s1.astype(np.float32))), "dbeta"
    assert np.array_equal(bits(got["dgamma"]), bits(s2.astype(np.float32))), "dgamma"
    assert np.array_equal(bits(got["dbias"]), bits(sb.astype(np.float32))), "dbias"
    if N >= 5:
        assert not np.array_equal(bits(s32), bits(s1.astype(np.float32))), "the order is not observable"

    # dW: sampled elements, one fma per ascending row from +0.0f
    g = np.random.default_rng(B + N + K)
    picks = {(0, 0), (N - 1, K - 1)} | {(int(g.integers(N)), int(g.integers(K))) for _ in range(6)}
    for n, k in sorted(picks):
        acc = np.float32(0)
        for r in range(B):
            acc = fma32(dY[r, n], d["X"][r, k], acc)
        assert bits(got["dW"][n, k]) == bits(acc), "dW[%d][%d]" % (n, k)

    # and the values against the float64 formulation
    _, bound = want_and_bound("nt", d["X"], d["W"], d["bias"])
    assert (np.abs(Y.astype(f64) - want["Y"]) <= bound).all(), "Y"
    close(got["A"], want["A"], 1e-4, "A")
    close(got["stats"][:N], want["mean"], 1e-4, "mean")
    close(got["stats"][N:], want["invstd"], 1e-4, "invstd")
    close(got["dgamma"], want["dgamma"], 1e-3, "dgamma")
    close(got["dbeta"], want["dbeta"], 1e-3, "dbeta")
    close(dY, want["dY"], 1e-3, "dY")
    close(got["dW"], want["dW"], 1e-3, "dW")
    if bn == "batch":  # analytically zero: float noise on both sides
        assert float(np.abs(got["dbias"]).max()) <= 1e-4 * float(np.abs(got["dW"]).max()), "dbias"
    else:
        close(got["dbias"], want["dbias"], 1e-3, "dbias")


def test_fma32_rounds_once():
    """The host chain's step against exact rational arithmetic, on ties that a float64 sum
    rounded twice gets wrong."""
    from fractions import Fraction
    g = np.random.default_rng(7)
    # exact = 2^24 + 3 - 2^-46: float64 rounds it onto the float32 tie 2^24 + 3, which then goes up
    cases_ = [(np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23), np.float32(2.0 ** 24 + 2))]
    assert np.float32(float(cases_[0][0]) * float(cases_[0][1]) + float(cases_[0][2])) == np.float32(2.0 ** 24 + 4)
    assert fma32(*cases_[0]) == np.float32(2.0 ** 24 + 2)
    cases_ += [tuple(np.float32(v) for v in g.standard_normal(3)) for _ in range(200)]
    for a, b, c in cases_:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo = np.float32(float(exact))  # a neighbour of the exact value
        cand = sorted({lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))},
                      key=lambda v: (abs(Fraction(float(v)) - exact), int(bits(v)[0]) & 1))
        assert bits(fma32(a, b, c)) == bits(cand[0]), (a, b, c)


# ------------------------------------------------------------------------------ recorded bits
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fc_train_bits.json")


def golden_shapes():
    shapes = [(max_rows() if B == "max" else B, N, K) for B, N, K in SHAPES]
    shapes += [c[:3] for c in BELOW] + RULE_CASES + [(33, 5, 1029), (65, 5, 1029), (128, 6, 64), (129, 5, 1028)]
    return sorted(set(shapes))


def golden_bits():
    """{"B,N,K,bn,relu,entry": {output: CRC32 of its raw bytes}} for every recorded case: each
    shape with every BN mode (one row: not batch) and with and without ReLU, on the 64-row entries
    (up to 64 rows) and on the any-B entries, contiguous operands, make_inputs(seed B*11 + N + K)."""
    out = {}
    for B, N, K in golden_shapes():
        d = make_inputs(B, N, K, seed=B * 11 + N + K)
        for bn in BNS:
            if B == 1 and bn == "batch":
                continue
            for relu in (1, 0):
                for rows in ([False, True] if B <= max_rows() else [True]):
                    got = run_entries(d, bn, relu, "contig", rows=rows)
                    key = "%d,%d,%d,%s,%d,%s" % (B, N, K, bn, relu, "rows" if rows else "64")
                    out[key] = {k: "%08x" % zlib.crc32(np.ascontiguousarray(got[k], np.float32).tobytes())
                                for k in OUT}
    return out


def test_bits_are_the_recorded_ones():
    """Every output of both entry pairs has the bits recorded before the kernels became one
    template pair (above 64 rows there is no second kernel to compare against)."""
    with open(GOLDEN) as f:
        want = json.load(f)["crc32"]
    got = golden_bits()
    assert got.keys() == want.keys()
    bad = ["%s %s" % (k, o) for k in want for o in OUT if got[k][o] != want[k][o]]
    assert not bad, "%d outputs differ, the first: %s" % (len(bad), ", ".join(bad[:8]))


# ------------------------------------------------------------------------------ loads and edges
@pytest.mark.parametrize("bn", BNS)
@pytest.mark.parametrize("K", [259, 260])
def test_leading_dimensions_and_unaligned_bases(K, bn):
    """ld > width (and not a multiple of 4) and a base one float off a 16-byte boundary switch
    the 16-byte loads off: the same bits as the contiguous case (K = 260: that one runs the
    16-byte path; K = 259: dword loads everywhere), nothing written outside any output."""
    d = make_inputs(65, 5, K, seed=K)
    base = run_entries(d, bn, 1, "contig", rows=True)
    for mode in ("ld", "offset"):
        same_bits(run_entries(d, bn, 1, mode, rows=True), base, mode)


def test_momentum_zero_keeps_running_statistics():
    d = make_inputs(65, 5, 6, seed=3)
    got = run_entries(d, "batch", 1, "contig", rows=True, momentum=0.0)
    assert np.array_equal(bits(got["rm"]), bits(d["rm"])) and np.array_equal(bits(got["rv"]), bits(d["rv"]))


# ------------------------------------------------------------------------------ routes
def _names(t, prefix):
    return [r[0] for r in t.records if r[0].startswith(prefix)]


def test_cls_tail_route_agrees_with_the_modules():
    from pn2 import heads, ops, tuning
    mod = cases.build_head(heads.ClsSSG, 60).to(DEV)
    g = torch.Generator().manual_seed(61)
    x0 = torch.randn(72, 1024, generator=g).to(DEV)
    R = torch.randn(72, 7, generator=g).to(DEV)
    with tuning.override(train_head_rows=1), ops.kernel_timer() as t:
        _routes_agree(mod, lambda m, x: m._fc(x), x0, R, True, ("fc1.bias", "fc2.bias"))
    assert _names(t, "pn2_fc_rows") == ["pn2_fc_rows_forward_f32"] * 3 + ["pn2_fc_rows_backward_f32"] * 3
    assert not _names(t, "pn2_fc_bn")
    assert [r[0] for r in t.records].count("pn2_gemm_nn_f32") == 3


def test_mean_mlp_route_agrees_with_the_modules():
    from pn2 import heads, ops, tuning
    mod = cases.build_head(heads.TranslationSSG, 92).to(DEV)
    g = torch.Generator().manual_seed(93)
    x0 = torch.randn(72, 3, generator=g).to(DEV)
    R = torch.randn(72, 3, generator=g).to(DEV)
    with tuning.override(train_head_rows=1), ops.kernel_timer() as t:
        _routes_agree(mod, lambda m, x: m._mean_mlp(x), x0, R, True, ("mean_fc1.bias",))
    assert _names(t, "pn2_fc_rows") == ["pn2_fc_rows_forward_f32"] * 2 + ["pn2_fc_rows_backward_f32"] * 2
    assert not _names(t, "pn2_fc_bn")


def test_route_needs_both_keys():
    from pn2 import ops, tuning
    assert tuning.get("train_head_rows") == 0
    for keys, rows in ((dict(train_head=1), 0), (dict(train_head_rows=1), 0),
                       (dict(train_head=1, train_head_rows=1), 3)):
        mod, x = _cls_tail(72)
        with tuning.override(**keys), ops.kernel_timer() as t:
            mod._fc(x).sum().backward()
        assert not _names(t, "pn2_fc_bn"), keys
        names = _names(t, "pn2_fc_rows")
        assert names.count("pn2_fc_rows_forward_f32") == rows == names.count("pn2_fc_rows_backward_f32"), keys
    # 64 rows or fewer keep the 64-row kernels either way
    mod, x = _cls_tail(64)
    with tuning.override(train_head=1, train_head_rows=1), ops.kernel_timer() as t:
        mod._fc(x).sum().backward()
    assert len(_names(t, "pn2_fc_bn")) == 6 and not _names(t, "pn2_fc_rows")


# ------------------------------------------------------------------------------ reproducible step
@pytest.mark.parametrize("which", ["cls_ssg", "translation_ssg"])
def test_reproducible_whole_model_step_above_64_rows(which):
    """test_gpu_fc_train.test_reproducible_whole_model_step at B = 72, N = 1024 with
    train_head_rows=1 beside the three reproducibility keys: the loss, every gradient, every
    buffer and every parameter after Adam's step bit-identical between two runs."""
    from pn2 import heads, ops, tuning
    B, N = 72, 1024
    g = torch.Generator().manual_seed(80)
    if which == "cls_ssg":
        mod = cases.build_head(heads.ClsSSG, 81).to(DEV).train()
        pts = cases.cloud("uniform3", B, N, 82).permute(0, 2, 1).contiguous().to(DEV)
        target = torch.randint(0, 7, (B,), generator=g).to(DEV)
        fl = lambda m: F.nll_loss(m(pts)[0], target)
    else:
        mod = cases.build_head(heads.TranslationSSG, 83).to(DEV).train()
        pts = cases.cloud("onehot10", B, N, 84).permute(0, 2, 1).contiguous().to(DEV)
        mean = torch.randn(B, 3, generator=g).to(DEV)
        target = torch.randn(B, 3, generator=g).to(DEV)
        fl = lambda m: F.mse_loss(m(pts, mean), target)
    with tuning.override(train_head_rows=1), ops.kernel_timer() as t:
        a, b = _two_model_steps(mod, fl)
    per_step = 5 if which == "translation_ssg" else 3
    names = _names(t, "pn2_fc_rows")
    assert names.count("pn2_fc_rows_forward_f32") == 2 * per_step == names.count("pn2_fc_rows_backward_f32")
    assert not _names(t, "pn2_fc_bn")
    assert a.keys() == b.keys() and len(a) > 20
    for k in a:
        if a[k].dtype == np.float32:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k
    for layer in ("fc1.weight", "fc3.weight", "sa1.mlp_convs.0.weight"):
        assert float(np.abs(a["grad " + layer]).max()) > 0, layer

"""Training-batch preparation: pn2.provider.draw_augmentation / prepare_train_batch against the
reference's own training-loop sequence (tests/golden/augment_*.npz, made by
make_goldens_augment.py from provider.py's functions) and its numpy restatement
(tests/augment_ref.py).

Bar: bit-exact float32 bits of the model input and of the mean, prepare_batch's own bar -- the
kernel applies the augmentations in float64 with the reference's roundings (one multiply, one
add, no FMA) and everything after them in numpy's operation order."""
import numpy as np
import pytest
import torch

import augment_ref
import cases
from conftest import golden_names, load_golden

NAMES = golden_names("augment_")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same_draws(got, want):
    for key in ("drop", "scale", "shift"):
        g, w = getattr(got, key), getattr(want, key)
        assert (g is None) == (w is None), key
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, key
            np.testing.assert_array_equal(g, w)


def _labels(g):
    return g["labels"] if "labels" in g else None


# ---------------------------------------------------------------------------------- CPU
def test_golden_set():
    assert NAMES == ["batch", "c6", "chunk", "five", "tiny"]
    shapes = sorted(load_golden("augment_%s.npz" % n)["raw"].shape for n in NAMES)
    assert shapes == [(2, 5, 3), (2, 257, 6), (2, 1030, 3), (3, 2, 3), (4, 1024, 3)]
    with_labels = [("labels" in load_golden("augment_%s.npz" % n)) for n in NAMES]
    assert any(with_labels) and not all(with_labels)


def test_goldens_hold_the_drop_patterns():
    """The set as a whole: point 0 in a drop set, point 1 or 2 dropped, > 80 % dropped, < 5 %
    dropped, none dropped (the generator asserts the same when it picks the seeds)."""
    seen = set()
    for name in NAMES:
        g = load_golden("augment_%s.npz" % name)
        B, N, _ = g["raw"].shape
        np.random.seed(int(g["seed"]))
        for d in augment_ref.literal_draws(B, N).drop:
            seen |= {k for k, hit in (("first", d[0]), ("head", d[1:3].any()), ("most", d.mean() > 0.80),
                                      ("few", 0 < d.mean() < 0.05), ("none", not d.any())) if hit}
    assert seen == {"first", "head", "most", "few", "none"}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load_golden("augment_%s.npz" % name)
    B, N, _ = g["raw"].shape
    np.random.seed(int(g["seed"]))
    draws = augment_ref.literal_draws(B, N)
    assert np.random.random() == float(g["next_draw"])
    raw = g["raw"].copy()
    prepared, mean = augment_ref.prepare_train(raw, _labels(g), draws)
    np.testing.assert_array_equal(raw, g["raw"])
    np.testing.assert_array_equal(_bits(prepared), _bits(g["prepared"]))
    np.testing.assert_array_equal(_bits(mean), _bits(g["mean"]))


@pytest.mark.parametrize("name", NAMES)
def test_draws_match_reference_generator_use(name):
    from pn2.provider import draw_augmentation
    g = load_golden("augment_%s.npz" % name)
    B, N, _ = g["raw"].shape
    seed = int(g["seed"])
    np.random.seed(seed)
    want = augment_ref.literal_draws(B, N)
    np.random.seed(seed)
    got = draw_augmentation(B, N)
    _assert_same_draws(got, want)
    assert got.drop.dtype == np.bool_ and got.scale.dtype == np.float64 and got.shift.dtype == np.float64
    assert np.random.random() == float(g["next_draw"])
    # an explicit RandomState: the same values, the same state afterwards, the global untouched
    np.random.seed(seed + 1)
    before = np.random.get_state()[1].copy()
    rs = np.random.RandomState(seed)
    _assert_same_draws(draw_augmentation(B, N, rng=rs), want)
    assert rs.random_sample() == float(g["next_draw"])
    np.testing.assert_array_equal(np.random.get_state()[1], before)


def test_draw_options_reach_the_generator_calls():
    from pn2.provider import draw_augmentation
    kw = dict(max_dropout_ratio=0.5, scale_low=0.5, scale_high=2.0, shift_range=0.3)
    want = augment_ref.literal_draws(3, 40, np.random.RandomState(5), **kw)
    _assert_same_draws(draw_augmentation(3, 40, rng=np.random.RandomState(5), **kw), want)
    assert want.drop.mean() < 0.5 and np.abs(want.shift).max() > 0.1


@pytest.mark.parametrize("off", ["dropout", "scale", "shift", "all"])
def test_disabled_stage_draws_nothing(off):
    from pn2.provider import draw_augmentation
    B, N = 3, 17
    flags = {k: (k != off and off != "all") for k in ("dropout", "scale", "shift")}
    rs, rs_ref = np.random.RandomState(77), np.random.RandomState(77)
    got = draw_augmentation(B, N, rng=rs, **flags)
    want = augment_ref.literal_draws(B, N, rs_ref, **flags)
    _assert_same_draws(got, want)
    for key, field in (("dropout", "drop"), ("scale", "scale"), ("shift", "shift")):
        assert (getattr(got, field) is None) == (not flags[key])
    nxt = rs.random_sample()
    assert nxt == rs_ref.random_sample()
    if off == "all":  # nothing consumed at all
        assert nxt == np.random.RandomState(77).random_sample()


def test_prepare_train_batch_rejects_cpu_and_bad_input():
    from pn2.provider import Augmentation, draw_augmentation, prepare_train_batch
    x = torch.rand(2, 16, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        prepare_train_batch(x.float())
    with pytest.raises(IndexError):
        prepare_train_batch(x, label=[0, 7])
    with pytest.raises(RuntimeError, match="ROCm"):
        prepare_train_batch(x, device="cpu")
    ok = draw_augmentation(2, 16, rng=np.random.RandomState(0))
    for bad in (draw_augmentation(2, 15, rng=np.random.RandomState(0)),
                draw_augmentation(3, 16, rng=np.random.RandomState(0)),
                ok._replace(scale=np.ones(3)), ok._replace(shift=np.zeros((2, 2))),
                Augmentation(np.zeros((16, 2), dtype=bool), None, None)):
        with pytest.raises(ValueError, match="aug"):
            prepare_train_batch(x, aug=bad)


def test_names_exported():
    from pn2 import provider
    assert {"prepare_train_batch", "draw_augmentation", "prepare_batch"} <= set(provider.__all__)


# ---------------------------------------------------------------------------------- GPU
def _run(src, labels, **kw):
    from pn2.provider import prepare_train_batch
    x, mean = prepare_train_batch(src, labels, **kw)
    assert x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1
    return x.transpose(2, 1).cpu().numpy(), None if mean is None else mean.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_prepare_train_batch_matches_reference(name):
    g = load_golden("augment_%s.npz" % name)
    labels = torch.from_numpy(g["labels"]) if "labels" in g else None
    B, N, C = g["raw"].shape
    for src in (torch.from_numpy(g["raw"].copy()), torch.from_numpy(g["raw"]).cuda()):
        np.random.seed(int(g["seed"]))
        x, mean = _run(src, labels, with_mean=True)
        assert np.random.random() == float(g["next_draw"])
        assert x.shape == g["prepared"].shape and mean.shape == (B, C)
        np.testing.assert_array_equal(_bits(x), _bits(g["prepared"]))
        np.testing.assert_array_equal(_bits(mean), _bits(g["mean"]))
        np.testing.assert_array_equal(src.cpu().numpy(), g["raw"])  # never augmented in place


def _sweep_case(B, N, C, seed):
    raw = cases.raw_batch("raw", B, N, seed, C)
    draws = augment_ref.literal_draws(B, N, np.random.RandomState(seed + 1))
    return raw, np.arange(B) % 7, draws


def _aug(draws):
    from pn2.provider import Augmentation
    return Augmentation(*draws)


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,C,strided,normalize,with_labels", [
    (1, 2, 3, False, True, True),
    (2, 255, 3, False, True, False),
    (2, 256, 3, False, False, True),
    (3, 1025, 9, True, True, True),
    (2, 2049, 3, False, True, True),
])
def test_prepare_train_batch_matches_restatement(B, N, C, strided, normalize, with_labels):
    raw, labels, draws = _sweep_case(B, N, C, 7000 + N)
    if N == 2:  # keep the two points apart: a collapsed cloud (NaN) has its own test
        draws = draws._replace(drop=np.array([[True, False]]))
    if not with_labels:
        labels = None
    want, want_mean = augment_ref.prepare_train(raw, labels, draws, normalize=normalize)
    assert not np.isnan(want).any()
    t = torch.from_numpy(raw).cuda()
    if strided:  # a [B,N,C] view of [B,C,N] storage
        t = t.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        assert t.stride(2) == N
    x, mean = _run(t, None if labels is None else torch.from_numpy(labels), with_mean=True,
                   normalize=normalize, aug=_aug(draws))
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(_bits(mean), _bits(want_mean))
    np.testing.assert_array_equal(t.cpu().numpy(), raw)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", ["drop", "scale", "shift", "no_drop", "no_scale", "no_shift", "none"])
def test_each_stage_alone_and_each_stage_off(keep):
    from pn2.provider import prepare_batch
    B, N, C = 2, 300, 6
    raw, labels, draws = _sweep_case(B, N, C, 7100)
    fields = ("drop", "scale", "shift")
    if keep == "none":
        on = []
    elif keep.startswith("no_"):
        on = [f for f in fields if "no_" + f != keep]
    else:
        on = [keep]
    assert len(on) == {"none": 0}.get(keep, 2 if keep.startswith("no_") else 1)
    draws = draws._replace(**{f: None for f in fields if f not in on})
    want, want_mean = augment_ref.prepare_train(raw, labels, draws)
    t = torch.from_numpy(raw).cuda()
    x, mean = _run(t, torch.from_numpy(labels), with_mean=True, aug=_aug(draws))
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(_bits(mean), _bits(want_mean))
    if keep == "none":
        px, pmean = prepare_batch(t, torch.from_numpy(labels), with_mean=True)
        np.testing.assert_array_equal(_bits(x), _bits(px.transpose(2, 1).cpu().numpy()))
        np.testing.assert_array_equal(_bits(mean), _bits(pmean.cpu().numpy()))


def _all_dropped_case(N, C):
    raw, labels, draws = _sweep_case(2, N, C, 7200 + N)
    drop = draws.drop.copy()
    drop[0] = True
    drop[1] = False
    drop[1, 0] = True
    draws = draws._replace(drop=drop)
    return raw, labels, draws, augment_ref.prepare_train(raw, labels, draws)


def test_all_dropped_expectation():
    """What the restatement gives for a cloud that is N copies of point 0.  N = 2: the row sum
    x + x and its half are exact, the centroid is the point, the max norm 0 and xyz 0 / 0 = NaN.
    N = 130: the sequential sum of 130 equal values rounds, so the centroid misses the point by
    ulps and the result is a finite direction -- which the kernel has to reproduce as well."""
    for N, nan in ((2, True), (130, False)):
        want = _all_dropped_case(N, 6)[3][0]
        assert np.isnan(want[0, :, :3]).all() == nan and np.isnan(want[0, :, :3]).any() == nan
        assert not np.isnan(want[1]).any() and not np.isnan(want[0, :, 3:]).any()
        np.testing.assert_array_equal(want[0], np.broadcast_to(want[0, :1], want[0].shape))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 130])
def test_all_points_dropped(N):
    """Cloud 0 wholly dropped: every point is point 0.  NaN against NaN on values (the sign of a
    0 / 0 NaN is the FPU's, not the algorithm's); everything that is a number, bit for bit."""
    raw, labels, draws, (want, want_mean) = _all_dropped_case(N, 6)
    x, mean = _run(torch.from_numpy(raw), torch.from_numpy(labels), with_mean=True, aug=_aug(draws))
    np.testing.assert_array_equal(np.isnan(x), np.isnan(want))
    num = ~np.isnan(want)
    np.testing.assert_array_equal(_bits(x)[num], _bits(want)[num])
    np.testing.assert_array_equal(_bits(mean), _bits(want_mean))

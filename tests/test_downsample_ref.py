"""tests/downsample_ref.py (the reference's numpy farthest_point_sample restated) against the
goldens tests/golden/make_goldens_downsample.py wrote by running the reference's own function:
indices, gathered rows and generator consumption, bit for bit; and each golden still has the
property it was searched for (downsample_ref.PROPERTIES).  CPU only."""
import numpy as np
import pytest

import downsample_ref
from conftest import golden_names, load_golden

NAMES = golden_names("downsample_")


def test_golden_set():
    assert len(NAMES) >= 13
    props = {str(load_golden("downsample_%s.npz" % n)["prop"]) for n in NAMES}
    assert props == set(downsample_ref.PROPERTIES)
    dtypes = {load_golden("downsample_%s.npz" % n)["cloud"].dtype for n in NAMES}
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    g = load_golden("downsample_%s.npz" % name)
    cloud, number = g["cloud"], int(g["number"])
    np.random.seed(int(g["seed"]))
    rows = downsample_ref.farthest_point_sample(cloud, number)
    assert np.random.random() == float(g["next_draw"])
    assert rows.dtype == cloud.dtype == g["rows"].dtype
    np.testing.assert_array_equal(rows, g["rows"])
    idx = downsample_ref.sample_indices(cloud, number, g["idx"][0])
    np.testing.assert_array_equal(idx, g["idx"])
    np.testing.assert_array_equal(cloud[g["idx"]], g["rows"])


@pytest.mark.parametrize("name", NAMES)
def test_golden_has_its_property(name):
    g = load_golden("downsample_%s.npz" % name)
    assert downsample_ref.PROPERTIES[str(g["prop"])](g["cloud"], int(g["number"]), g["idx"]), str(g["prop"])


def test_fma64_emulation_is_exact():
    """The float64 half of the fma property is covered on every interpreter: without math.fma
    the restatement's fma is rational arithmetic rounded once."""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0
    assert a * b + c == 0.0                       # separately rounded: the product rounds to 1
    assert downsample_ref._fma64(a, b, c) == -2.0 ** -60


def test_issue_example_repeats_past_n():
    """number > N: N iterations take every point, the rest repeat the first index of an
    all-zero distance array."""
    cloud = np.array([[0, 0, 0], [9, 0, 0], [1, 0, 0], [3, 0, 0], [6, 0, 0]], dtype=np.float64)
    idx = downsample_ref.sample_indices(cloud, 9, 2)
    assert sorted(idx[:5].tolist()) == [0, 1, 2, 3, 4] and idx[5:].tolist() == [0, 0, 0, 0]

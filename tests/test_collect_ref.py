"""tests/collect_ref.py (the numpy restatement of the camera-cloud front end) against
hand-computed cases, and its visit-order DBSCAN against rule 4's closed form on every fixture the
GPU test uses."""
import numpy as np
import pytest

import collect_ref as ref


def test_three_collinear_points():
    # 0 -- 1 at distance 1, 1 -- 2 at distance 1, 0 -- 2 at distance 2; r = 1.5
    pc = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    nbr = ref.neighbour_matrix(pc, 1.5)
    assert nbr.tolist() == [[True, True, False], [True, True, True], [False, True, True]]
    assert ref.radius_counts(pc, 1.5).tolist() == [2, 3, 2]
    # the boundary is strict: at r = 1 exactly nobody but the point itself is a neighbour
    assert ref.radius_counts(pc, 1.0).tolist() == [1, 1, 1]
    # count > nb_points: 1 keeps all three, 2 keeps the middle one only
    assert ref.delet_outlier_radius(pc, 1, 1.5).tolist() == pc.tolist()
    assert ref.delet_outlier_radius(pc, 2, 1.5).tolist() == [[1, 0, 0]]
    # min_points = 3: only the middle point is core, the ends are its border
    assert ref.dbscan_labels(pc, 1.5, 3).tolist() == [0, 0, 0]
    # min_points = 2: all core, one chain
    assert ref.dbscan_labels(pc, 1.5, 2).tolist() == [0, 0, 0]
    assert ref.dbscan_labels(pc, 1.5, 4).tolist() == [-1, -1, -1]


def test_border_point_between_two_clusters():
    # two dense ends on the x axis (each point twice) and one point between them:
    #   index  0,3: 0.0   1,4: 0.1   2,5: -0.1   6,9: 2.0   7,10: 2.1   8,11: 1.9   12: 1.0
    x = [0.0, 0.1, -0.1] * 2 + [2.0, 2.1, 1.9] * 2 + [1.0]
    pc = np.array([[v, 0, 0] for v in x])
    # r = 1.05: each end point sees its 6; 0.0, 0.1, 2.0 and 1.9 also see point 12 (1.0, 0.9);
    # point 12 sees those 8 and itself
    assert ref.radius_counts(pc, 1.05).tolist() == [7, 7, 6, 7, 7, 6, 7, 6, 7, 7, 6, 7, 9]
    assert ref.dbscan_labels(pc, 1.05, 10).tolist() == [-1] * 13  # nobody is core
    # min_points = 7: point 12 is core and joins the two ends; -0.1 and 2.1 are its border
    assert ref.dbscan_labels(pc, 1.05, 7).tolist() == [0] * 13
    # r = 0.95 cuts point 12 from 0.0 and 2.0 (distance 1.0), not from 0.1 and 1.9 (0.9)
    assert ref.radius_counts(pc, 0.95).tolist() == [6, 7, 6, 6, 7, 6, 6, 6, 7, 6, 6, 7, 5]
    # min_points = 6: every end point is core, point 12 (5) is not and has core neighbours in
    # both clusters: it takes the smaller label
    assert ref.dbscan_labels(pc, 0.95, 6).tolist() == [0] * 6 + [1] * 6 + [0]
    # the ends swapped: the cluster at x = 2 now holds the smallest index, and the border point
    # still takes label 0 -- which now is the other cluster
    swapped = np.vstack([pc[6:12], pc[:6], pc[12:]])
    assert ref.dbscan_labels(swapped, 0.95, 6).tolist() == [0] * 6 + [1] * 6 + [0]


def test_duplicates():
    pc = np.array([[1.0, 2, 3]] * 4 + [[9.0, 9, 9]])
    assert ref.radius_counts(pc, 1e-3).tolist() == [4, 4, 4, 4, 1]
    assert ref.dbscan_labels(pc, 1e-3, 4).tolist() == [0, 0, 0, 0, -1]
    assert ref.dbscan_labels(pc, 1e-3, 1).tolist() == [0, 0, 0, 0, 1]
    assert ref.delet_outlier_radius(pc, 3, 1e-3).shape == (4, 3)
    assert ref.delet_outlier_radius(pc, 4, 1e-3).shape == (0, 3)


def test_all_noise(capsys):
    pc = ref.noise_cloud()
    assert ref.dbscan_labels(pc, ref.EPS, 3).tolist() == [-1] * len(pc)
    assert ref.cluster_point(pc, ref.EPS, 3) is None
    assert capsys.readouterr().out == "Null point\n"


def test_clip_and_nan():
    pc = np.array([[0.0, 0, 0.5], [0, 0, 2.0], [0, 0, np.nan], [0, 0, 2.5], [0, 0, 0.0], [0, 0, -0.1]])
    assert ref.clip_distance(pc)[:, 2].tolist() == [0.5, 2.0, 0.0]
    assert ref.clip_distance(pc, [0.5, 0.5])[:, 2].tolist() == [0.5]


def test_cluster_point_shapes_and_errors():
    pc = ref.five_cloud(C=6)
    np.random.seed(7)
    out = ref.cluster_point(pc, ref.EPS, 10)
    assert out.shape == (5, 20, 6) and out.dtype == np.float64
    with pytest.raises(ValueError):
        ref.cluster_point(np.array([[0.0, 0, 0], [5, 5, 5], [5, 5, 5.01]]), 0.1, 1)


@pytest.mark.parametrize("name", sorted(ref.LABEL_FIXTURES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_visit_order_equals_closed_form(name, dtype):
    build, eps, mp = ref.LABEL_FIXTURES[name]
    pc = build(3, dtype)
    labels = ref.dbscan_labels(pc, eps, mp)
    assert np.array_equal(labels, ref.labels_closed_form(pc, eps, mp))
    # each fixture is what its name says
    if name.startswith("border"):
        nbr = ref.neighbour_matrix(pc, eps)
        core = nbr.sum(1) >= mp
        mid = int(np.flatnonzero(~core)[0])
        assert (~core).sum() == 1 and labels.max() == 1
        assert sorted(set(labels[np.flatnonzero(nbr[mid] & core)].tolist())) == [0, 1] and labels[mid] == 0
    if name == "line":
        assert len(pc) == 600 and (labels == 0).all()
    if name == "five":
        assert labels.max() == 4
        centre_x = [pc[labels == l, 0].mean() for l in range(5)]
        assert centre_x != sorted(centre_x)  # label order is index order, not spatial order
        assert len(set(np.bincount(labels[labels >= 0]).tolist())) == 5  # unequal sizes
    if name == "noise":
        assert (labels == -1).all()


def test_swapped_border_fixture_is_the_other_order():
    a, b = ref.border_cloud(False), ref.border_cloud(True)
    la, lb = ref.dbscan_labels(a, ref.EPS, 10), ref.dbscan_labels(b, ref.EPS, 10)
    # cluster 0 is the left blob in one fixture and the right blob in the other
    assert (a[la == 0, 0].mean() < 0.085) != (b[lb == 0, 0].mean() < 0.085)


def test_lattice_sits_on_the_boundary():
    pc = ref.lattice_cloud()
    xyz = pc[:, :3]
    d2 = ((xyz[:, None] - xyz[None]) ** 2).sum(-1)
    assert (d2 == 0.125 * 0.125).sum() > 1000  # pairs exactly at r
    assert (ref.radius_counts(pc, 0.125) == 1).all()  # strict: none of them counts
    assert ref.radius_counts(pc, 0.126).max() == 7

"""The numpy restatement tests/plane_ref.py (include/pn2.h P1-P7) on clouds whose answer is known:
what tests/test_gpu_plane.py compares the kernels with must itself find the table."""
import numpy as np
import pytest

import collect_ref
import plane_ref as ref


def test_table_is_found_with_three_point_samples():
    pc = ref.table_cloud()
    table = ref.is_table(pc)
    assert pc.shape == (3900, 3) and table.sum() == 3000
    np.random.seed(1)
    samples = ref.draw_samples(len(pc), 3, 64)
    st = ref.segment(pc, samples, 0.006)
    assert st["result"][4] == 39 and st["result"][5] == 3000
    assert np.array_equal(st["flags"] != 0, table)  # exactly the table's rows
    assert st["result"][6] == st["err"][39] and st["count"].max() == 3000
    np.random.seed(1)
    kept = ref.delete_plane(pc, 0.006, 3, 64)  # the same draw again
    assert kept.shape == (900, 3) and np.array_equal(kept, pc[~table])  # the others, in input order
    np.random.seed(1)
    model, inliers = ref.segment_plane(pc, 0.006, 3, 64)
    assert inliers.dtype == np.int64 and np.array_equal(inliers, np.flatnonzero(table))
    # the refit over 3000 rows: the table is z = 0.8 +- 0.002
    assert abs(model[2]) > 0.99999 and abs(abs(model[3]) - 0.8) < 1e-3 and abs(np.linalg.norm(model[:3]) - 1) < 1e-12


def test_table_with_twenty_point_samples():
    """A 20-point fit over the whole cloud mixes table and boxes: fewer rows fit, none off the table."""
    pc = ref.table_cloud()
    np.random.seed(1)
    st = ref.segment(pc, ref.draw_samples(len(pc), 20, 64), 0.006)
    assert 0 < st["result"][5] <= 3000
    assert not (st["flags"] != 0)[~ref.is_table(pc)].any()


def test_lattice_ties_go_to_the_lowest_index():
    pc = collect_ref.lattice_cloud()  # 343 points, every coordinate a multiple of 1/8
    np.random.seed(2)
    st = ref.segment(pc, ref.draw_samples(len(pc), 3, 200), 1e-3)
    count, err, result = st["count"], st["err"], st["result"]
    ties = np.flatnonzero((count == 49) & (err == 0.0))  # a lattice plane holds 7 x 7 points exactly
    assert count.max() == 49 and len(ties) == 13 and ties[0] == 5
    assert result[4] == 5 and result[5] == 49 and result[6] == 0.0
    assert st["flags"].sum() == 49


def test_degenerate_sample_rows():
    pc = ref.degenerate_cloud()
    st = ref.segment(pc, ref.DEGENERATE_N3, 0.01)
    assert not st["planes"][[0, 1, 3]].any() and not st["count"][[0, 1, 3]].any() and not st["err"].any()
    assert np.array_equal(st["planes"][2], [0, 0, 1, -1]) and st["result"][4] == 2 and st["result"][5] == 13
    st = ref.segment(pc, ref.DEGENERATE_N4, 0.01)
    assert not st["planes"][[0, 2]].any() and st["count"].tolist() == [0, 13, 0]
    assert np.array_equal(st["planes"][1], [0, 0, 1, -1]) and st["result"][4] == 1  # the duplicate counts twice
    assert np.array_equal(np.flatnonzero(st["flags"]), [2] + list(range(4, 16)))


def test_nothing_but_zero_planes():
    pc = ref.degenerate_cloud()
    st = ref.segment(pc, ref.ALL_ZERO_N3, 0.01)
    assert not st["planes"].any() and not st["count"].any()
    assert st["result"].tolist() == [0, 0, 0, 0, -1, 0, 0, 0] and not st["flags"].any()
    assert np.array_equal(ref.delete_plane(pc, 0.01, 3, 4, samples=ref.ALL_ZERO_N3), pc)  # unchanged
    model, inliers = ref.segment_plane(pc, 0.01, 3, 4, samples=ref.ALL_ZERO_N3)
    assert not model.any() and len(inliers) == 0


def test_out_of_range_row_is_skipped_and_nan_rows_never_fit():
    pc = ref.degenerate_cloud()
    table = np.array([[4, 5, 16], [4, -1, 8], [4, 5, 8]])
    st = ref.segment(pc, table, 0.01)
    assert not st["planes"][:2].any() and st["result"][4] == 2
    pc[6] = [np.nan, 0, 1]
    pc[7] = [0.75, np.inf, 1]
    st = ref.segment(pc, np.array([[4, 5, 8], [4, 6, 8], [7, 5, 8]]), 0.01)
    assert st["count"].tolist() == [11, 0, 0] and st["result"][4] == 0  # a NaN plane never wins
    assert st["flags"][[6, 7]].tolist() == [0, 0]


def test_chains_start_from_plus_zero():
    assert np.signbit(ref.chain_sum([-0.0, -0.0])) == False and ref.chain_sum([]) == 0.0  # noqa: E712
    assert ref.chain_sum([1e16, 1.0, 1.0]) == 1e16 and ref.chain_sum([1.0, 1.0, 1e16]) == 1e16 + 2  # left to right


def test_arguments():
    pc = ref.degenerate_cloud()
    for kw in (dict(ransac_n=2), dict(ransac_n=17), dict(num_iterations=0), dict(distance_threshold=0.0),
               dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")),
               dict(distance_threshold=float("inf"))):
        with pytest.raises(ValueError):
            ref.delete_plane(pc, **{**dict(distance_threshold=0.01, ransac_n=3, num_iterations=4), **kw})

"""The hand-built neighbour lists of tests/sa_lists.py, checked without a GPU: every list obeys
the contract of ops.sa_mlp_max_impl, the table reaches the edges of the chain's compact
bookkeeping it was built for (csrc/sa_chain.hip compact_scan_kernel), and every group's planted
neighbour dominates its float64 max.  These are conditions on the cases, not measurements."""
import numpy as np
import pytest

import sa_lists as sl

ALL = [(n, p) for n in sl.CASES for p in sl.patterns_of(n)]


def _layout(cnt):
    """Per cloud: each group's first unit and unit count (the scan's exclusive prefix sum)."""
    u = sl.units_of(cnt)
    start = np.cumsum(u, axis=1) - u
    return start, u


@pytest.mark.parametrize("order", sl.ORDERS)
@pytest.mark.parametrize("name,pattern", ALL)
def test_lists_obey_the_contract(name, pattern, order):
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    idx, cnt, want = sl.reference(name, pattern, order)
    assert np.isfinite(want).all() and want.min() >= 0.0 and want.max() > 0.0
    idx, cnt = idx.numpy(), cnt.numpy()
    assert idx.shape == (B, S, K) and idx.dtype == np.int64
    assert cnt.shape == (B, S) and cnt.dtype == np.int32
    hot = sl.hot_points(N)
    if pattern == "nohit":
        assert (cnt == 0).any() and (cnt > 0).any()
    else:
        assert cnt.min() >= 1
    assert cnt.max() <= K
    for b in range(B):
        for s in range(S):
            c, row = cnt[b, s], idx[b, s]
            if c == 0:  # the ball query's row for a centroid without a neighbour
                assert (row == N).all()
                continue
            assert row[:c].min() >= 0 and row[:c].max() < N
            assert (row[c:] == row[0]).all()
            p = sl.planted_row(c, b * S + s)
            assert row[p] in hot and np.isin(row[:c], hot).sum() == 1
            if order == "asc":
                assert (np.diff(row[:c]) > 0).all()
            elif order == "perm":
                assert len(set(row[:c])) == c
    if order == "dup" and pattern in ("full", "ramp") and K >= 32 and name in sl.MAIN:
        assert any(len(set(idx[b, s, :cnt[b, s]])) < cnt[b, s] for b in range(B) for s in range(S))


def test_patterns_are_what_they_say():
    for name, pattern in ALL:
        C, D, mode, mlp, K, S, N, B = sl.CASES[name]
        cnt = sl.counts(B, S, K, pattern)
        total = sl.units_of(cnt).sum(axis=1)
        if pattern == "ones":
            assert (cnt == 1).all()
        if pattern == "full":
            assert (cnt == K).all()
        if pattern == "exact":
            assert (total % sl.UNITS_PER_WG == 0).all()
        if pattern == "plus1":
            assert (total % sl.UNITS_PER_WG == 1).all()
        if pattern == "ramp" and S >= K:
            assert set(cnt[0]) == set(range(1, K + 1))
    # every unit count of the large K occurs in some ramp
    for name in ("k72", "k128wide"):
        C, D, mode, mlp, K, S, N, B = sl.CASES[name]
        seen = set()
        for pattern in ("ramp", "exact", "plus1", "full"):
            seen |= set(sl.units_of(sl.counts(B, S, K, pattern)).ravel())
        assert len(seen) >= 8 and int(sl.units_of(K)) in seen


def test_fill16_placements():
    """The first 16-unit group exactly fills workgroup 1; the second starts one unit into
    workgroup 2 and ends in workgroup 3."""
    C, D, mode, mlp, K, S, N, B = sl.CASES["k128wide"]
    start, u = _layout(sl.counts(B, S, K, "fill16"))
    for b in range(B):
        assert list(u[b, :16]) == [1] * 16 and (start[b, :16] // 16 == 0).all()
        assert (start[b, 16], u[b, 16]) == (16, 16)
        assert (start[b, 17], u[b, 17]) == (32, 1)
        assert (start[b, 18], u[b, 18]) == (33, 16)
        assert start[b, 18] // 16 == 2 and (start[b, 18] + 15) // 16 == 3


def test_table_reaches_the_bookkeeping_edges():
    offsets, straddle_starts, straddle_offsets = set(), set(), set()
    spans = crowded = unused = tail_partial = 0
    for name, pattern in ALL:
        C, D, mode, mlp, K, S, N, B = sl.CASES[name]
        if K <= sl.UNIT_ROWS:
            continue
        cnt = sl.counts(B, S, K, pattern)
        start, u = _layout(cnt)
        wpc = sl.compact_wpc(S, K)
        for b in range(B):
            total = int(u[b].sum())
            assert total <= wpc * sl.UNITS_PER_WG
            offsets |= set(start[b] % sl.UNITS_PER_WG)
            first_wg, last_wg = start[b] // 16, (start[b] + u[b] - 1) // 16
            two = first_wg != last_wg
            spans += int(two.sum())
            # where a straddling group starts in its first workgroup and ends in its second
            straddle_starts |= set((start[b] % 16)[two])
            straddle_offsets |= set(((start[b] + u[b]) % 16)[two])
            crowded += int((np.bincount(first_wg) > 8).any())
            unused += int(-(-total // 16) < wpc)
            tail_partial += int(total % 16 != 0)
    assert offsets == set(range(16))             # groups start at every offset of a workgroup
    # straddlers split 15 + 1 (one unit left in the first workgroup) and 1 + 15, and many ways
    # between; they end at many offsets of the second
    assert {1, 15} <= straddle_starts and len(straddle_starts) >= 8 and len(straddle_offsets) >= 8
    assert spans > 0       # a group spans two workgroups
    assert crowded > 0     # more groups in a workgroup than the automatic pool's 8 rows
    assert unused > 0      # trailing workgroups without a unit (desc.y < 0)
    assert tail_partial > 0  # a last workgroup with unused units (cunits = -1)


def test_scan_loop_cases():
    """S above kScanThreads: every scan thread walks more than one group."""
    pers = {(sl.CASES[n][5] + sl.SCAN_THREADS - 1) // sl.SCAN_THREADS for n in ("bigS", "midS")}
    assert pers == {2, 3}
    assert sl.CASES["bigS"][4:8] == (16, 1040, 128, 2) and sl.CASES["bigS"][3] == [32, 32, 64]
    assert sl.CASES["one"][5] == 1 and sl.CASES["one"][7] == 1


def test_prepass_cases_have_the_rows():
    """The wide first layers take the per-point pre-pass only when 4*B*N <= B*S*K (plan_chain)."""
    for name in ("k128wide", "k32wide"):
        C, D, mode, mlp, K, S, N, B = sl.CASES[name]
        assert D == 128 and 4 * B * N <= B * S * K


@pytest.mark.parametrize("name,pattern", ALL)
def test_planted_row_dominates(name, pattern):
    """In every group the planted row alone gives the float64 max of at least one channel, by
    more than 100x the comparison's absolute tolerance (1e-5 of the output's max magnitude)."""
    C, D, mode, mlp, K, S, N, B = sl.CASES[name]
    for order in sl.ORDERS if name in sl.MAIN else ("asc",):
        idx, cnt, want = sl.reference(name, pattern, order)
        y = sl.rows_out(name, idx)
        np.testing.assert_array_equal(y.max(axis=2), want)
        margin = 100 * 1e-5 * np.abs(want).max()
        idx, cnt = idx.numpy(), cnt.numpy()
        for b in range(B):
            for s in range(S):
                c = cnt[b, s]
                if c <= 1:
                    continue  # (a single row is the max)
                p = sl.planted_row(c, b * S + s)
                others = y[b, s, :c][idx[b, s, :c] != idx[b, s, p]]
                assert (y[b, s, p] > others.max(axis=0) + margin).any(), (name, pattern, order, b, s)

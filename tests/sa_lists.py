"""Neighbour lists built by hand for the fused gather -> MLP -> max call (pn2_sa_mlp_max_f32 /
_bf16 through ops.sa_mlp_max_impl), the inputs that go with them and the float64 reference.
Plain numpy / torch, no GPU: tests/test_sa_lists.py checks the table, tests/test_gpu_sa_lists.py
runs it.

The lists obey the contract of ops.sa_mlp_max_impl (csrc/sa_chain.hip ChainArgs): idx[b,s,:cnt]
are indices in [0,N), idx[b,s,cnt:] all equal idx[b,s,0], 1 <= cnt <= K -- except the rows the
ball query writes for a centroid without a neighbour (pattern "nohit"): cnt = 0, every index N.

The chain's compact launch (pool_mode 3) lays each group's ceil(cnt / 8) units of 8 rows out in
group order, 16 units per workgroup (kUnitRows, kUnitsPerWG); the patterns below choose the
counts so that the group boundaries fall where that bookkeeping can go wrong.

Every group holds one planted neighbour that dominates its max: a "hot" point whose features
are ~50x the others' (D > 0) or that lies ~10x as far from the centroids (D = 0).  A kernel that
drops the planted row (a unit, a seam row, the last distinct row) is then wrong by far more
than the tolerance.  Its row cycles over: row 0, the last distinct row, the first row of the
last unit, row 7 / 8 (the unit seam)."""
import functools

import numpy as np
import torch

import cases
import oracle

UNIT_ROWS = 8       # csrc/sa_chain.hip kUnitRows
UNITS_PER_WG = 16   # kUnitsPerWG
SCAN_THREADS = 512  # kScanThreads: compact_scan_kernel scans ceil(S / 512) groups per thread

PATTERNS = ("ones", "full", "ramp", "fill16", "exact", "plus1", "nohit")
ORDERS = ("asc", "perm", "dup")
FEAT_SCALE = 50.0   # a hot point's features against the others'
DIST_SCALE = 10.0   # D = 0: a hot point's distance from the origin against the unit sphere's


def units_of(cnt):
    """8-row units of a group with cnt distinct neighbours (compact_scan_kernel: at least one)."""
    return np.maximum(1, (np.asarray(cnt) + UNIT_ROWS - 1) // UNIT_ROWS)


def compact_wpc(S, K):
    """Chain workgroups per cloud of a compact launch (csrc/sa_chain.hip compact_wpc)."""
    return (S * ((K + UNIT_ROWS - 1) // UNIT_ROWS) + UNITS_PER_WG - 1) // UNITS_PER_WG


def hot_points(N):
    """The cloud's hot point indices: both ends, and points with at least 8 ordinary points on
    either side, so that an ascending list can hold one at any planted row."""
    return sorted({0, 9, N // 4, N // 2, (3 * N) // 4, N - 10, N - 1})


def planted_row(cnt, g):
    """Row of group g's planted neighbour among its cnt distinct rows."""
    m = g % 4
    if m == 0:
        p = 0
    elif m == 1:
        p = cnt - 1
    elif m == 2:
        p = UNIT_ROWS * ((cnt - 1) // UNIT_ROWS)
    else:
        p = 7 if (g // 4) % 2 == 0 else 8
    return min(p, cnt - 1)


def _retarget(cnt, K, residue):
    """Move each cloud's total units to `residue` (mod 16): add one-row units to the last
    groups that have room, else take whole units from them."""
    maxu = int(units_of(K))
    for c in cnt:
        d = int((residue - units_of(c).sum()) % UNITS_PER_WG)
        for s in range(len(c) - 1, -1, -1):
            while d and units_of(c[s]) < maxu:
                c[s] = min(K, UNIT_ROWS * int(units_of(c[s])) + 1)
                d -= 1
        d = int((units_of(c).sum() - residue) % UNITS_PER_WG)
        for s in range(len(c) - 1, -1, -1):
            while d and units_of(c[s]) > 1:
                c[s] = UNIT_ROWS * (int(units_of(c[s])) - 1)
                d -= 1
        if (units_of(c).sum() - residue) % UNITS_PER_WG:
            raise ValueError("sa_lists: %d groups of K = %d cannot total %d units (mod 16)"
                             % (len(c), K, residue))
    return cnt


def counts(B, S, K, units_pattern):
    """cnt [B, S] int32 of a named pattern."""
    s = np.arange(S)[None, :]
    b = np.arange(B)[:, None]
    step = 1 if K <= 32 else 5  # coprime to 72 and 128: a few dozen groups reach every unit count
    ramp = (1 + (s * step + 3 * b) % K).astype(np.int32)
    if units_pattern == "ones":
        cnt = np.ones((B, S), np.int32)
    elif units_pattern == "full":
        cnt = np.full((B, S), K, np.int32)
    elif units_pattern == "ramp":
        cnt = ramp
    elif units_pattern == "fill16":
        if K != 128 or S != 19:
            raise ValueError("sa_lists: fill16 is 19 groups of K = 128")
        cnt = np.ones((B, S), np.int32)
        cnt[:, 16] = cnt[:, 18] = K  # units 16..31 (one workgroup) and 33..48 (two)
    elif units_pattern == "exact":
        cnt = _retarget(ramp, K, 0)
    elif units_pattern == "plus1":
        cnt = _retarget(ramp, K, 1)
    elif units_pattern == "nohit":
        cnt = ramp
        cnt[:, 2::5] = 0
        if S > 1:
            cnt[0, S - 1] = 0
            cnt[B - 1, 0] = 0
    else:
        raise ValueError(units_pattern)
    return np.ascontiguousarray(cnt, np.int32)


def build(B, S, K, N, units_pattern, order, seed):
    """idx [B, S, K] int64 and cnt [B, S] int32 (torch, CPU).  Group g = b*S + s holds one of
    hot_points(N) at planted_row(cnt, g) and ordinary points elsewhere.  order: "asc" distinct
    ascending (the ball query's), "perm" distinct shuffled, "dup" drawn with replacement."""
    if order not in ORDERS:
        raise ValueError(order)
    rng = np.random.default_rng(seed)
    cnt = counts(B, S, K, units_pattern)
    hot = hot_points(N)
    ordinary = np.setdiff1d(np.arange(N), hot)
    idx = np.full((B, S, K), N, np.int64)
    for b in range(B):
        for s in range(S):
            c = int(cnt[b, s])
            if c == 0:
                continue
            g = b * S + s
            p = planted_row(c, g)
            for t in range(len(hot)):  # the first hot point with room on both sides
                h = hot[(g + t) % len(hot)]
                lo, hi = ordinary[ordinary < h], ordinary[ordinary > h]
                if len(lo) >= p and len(hi) >= c - 1 - p:
                    break
            else:
                raise ValueError("sa_lists: no hot point of N = %d fits row %d of %d" % (N, p, c))
            if order == "asc":
                row = np.concatenate([np.sort(rng.choice(lo, p, replace=False)), [h],
                                      np.sort(rng.choice(hi, c - 1 - p, replace=False))])
            else:
                rest = rng.choice(ordinary, c - 1, replace=order == "dup")
                row = np.concatenate([rest[:p], [h], rest[p:]])
            idx[b, s, :c] = row
            idx[b, s, c:] = row[0]
    return torch.from_numpy(idx), torch.from_numpy(cnt)


# ---------------------------------------------------------------------------- case table
# name -> (C, D, mode, mlp, K, S, N, B); mode 0: SSG rows [xyz | features], 1: MSG rows
# [features | xyz].  One layer set per compiled chain signature (T0, T1, KB0M of
# PN2_CHAIN_SIGS), C = 3 and the 10-channel one-hot layout, D in {0, 13, 128}, every K of
# {12, 16, 24, 32, 72, 128}.  S*K is a multiple of 32 wherever the full launch is the chain
# kernel too (K = 16, 32, 128), so both launches use the same arithmetic (chain_fit f16_ok).
CASES = {
    "k12":      (3, 0, 0, [64, 64, 128], 12, 40, 64, 2),        # (2,2,1); K % 8 != 0
    "k16msg":   (3, 13, 1, [32, 32, 64], 16, 48, 96, 3),        # (1,1,0)
    "k24":      (3, 0, 0, [64, 96, 128], 24, 37, 100, 2),       # (2,3,1)
    "k32oh":    (10, 0, 0, [32, 32, 64], 32, 33, 128, 2),       # (1,1,1)
    "k72":      (3, 13, 0, [64, 64, 128], 72, 23, 160, 2),      # (2,2,0); 9 units per full group
    "k128wide": (3, 128, 0, [128, 128, 256], 128, 19, 256, 2),  # (4,4,-1) / (4,4,9); fill16
    "k32wide":  (3, 128, 1, [64, 64, 128], 32, 40, 128, 2),     # (2,2,-1) / (2,2,0)
    "k16oh":    (10, 13, 1, [64, 96, 128], 16, 24, 64, 2),      # (2,3,0)
    "bigS":     (3, 0, 0, [32, 32, 64], 16, 1040, 128, 2),      # the scan's per-thread loop
    "midS":     (3, 0, 0, [32, 32, 64], 16, 600, 128, 2),       # ... at 2 groups per thread
    "one":      (3, 0, 0, [32, 32, 64], 32, 1, 64, 1),          # S = 1, B = 1
}
# the cases every pattern x order runs on (the last three run "ramp" only)
MAIN = ("k12", "k16msg", "k24", "k32oh", "k72", "k128wide", "k32wide", "k16oh")


def patterns_of(name):
    if name not in MAIN:
        return ("ramp",)
    return tuple(p for p in PATTERNS if p != "fill16" or name == "k128wide")


def chainable(K):
    """The full (non-compact) launch of this K is the chain kernel (plan_chain)."""
    return K in (8, 16) or K % 32 == 0


def oracle_layers(convs, bns):
    out = []
    for conv, bn in zip(convs, bns):
        out.append(dict(W=conv.weight.detach().reshape(conv.weight.shape[0], -1).cpu().numpy(),
                        b=conv.bias.detach().cpu().numpy(), gamma=bn.weight.detach().cpu().numpy(),
                        beta=bn.bias.detach().cpu().numpy(), mean=bn.running_mean.cpu().numpy(),
                        var=bn.running_var.cpu().numpy(), eps=bn.eps))
    return out


@functools.lru_cache(maxsize=None)
def module(name, last_beta=None):
    """The case's SA module on the CPU (seeded weights, cases.randomize_bn statistics) ->
    (module, convs, bns).  last_beta: the last BatchNorm's bias on every channel."""
    import pn2
    C, D, mode, mlp, K, S, N, B = CASES[name]
    seed = sorted(CASES).index(name)
    torch.manual_seed(3100 + seed)
    if mode == 1:
        sa = pn2.PointNetSetAbstractionMsg(S, [K], [0.3], D, [mlp], num_category=C - 3)
        convs, bns = sa.conv_blocks[0], sa.bn_blocks[0]
    else:
        sa = pn2.PointNetSetAbstraction(S, K, 0.3, C + D, mlp)
        convs, bns = sa.mlp_convs, sa.mlp_bns
    cases.randomize_bn(sa, 3200 + seed)
    if last_beta is not None:
        with torch.no_grad():
            bns[-1].bias.fill_(last_beta)
    return sa.eval(), convs, bns


@functools.lru_cache(maxsize=None)
def inputs(name, plant=True):
    """points [B,N,C], features [B,N,D] or None, centres [B,S,C] (float32, CPU).  The centres
    are random points of the unit sphere, not FPS picks.  plant=False: no hot points."""
    C, D, mode, mlp, K, S, N, B = CASES[name]
    seed = sorted(CASES).index(name)
    kind = "onehot10" if C == 10 else "uniform3"
    pts = cases.cloud(kind, B, N, 3300 + seed)
    ctr = cases.cloud(kind, B, max(S, 8), 3400 + seed)[:, :S].contiguous()  # (one point alone normalises to 0/0)
    feat = torch.randn(B, N, D, generator=torch.Generator().manual_seed(3500 + seed)) if D else None
    if plant:
        for i, h in enumerate(hot_points(N)):
            if D:
                feat[:, h] *= FEAT_SCALE * (1.0 + 0.1 * i)
            else:
                xyz = pts[:, h, :3]
                pts[:, h, :3] = xyz / xyz.norm(dim=1, keepdim=True) * (DIST_SCALE * (1.0 + 0.1 * i))
    return pts, feat, ctr


def clamp_index(idx, N):
    """The SA kernels' rule for an index outside [0, N) (the ball query's no-neighbour pad N):
    the row reads point 0 of its cloud."""
    return torch.where((idx < 0) | (idx >= N), torch.zeros_like(idx), idx)


def rows_out(name, idx, last_beta=None, plant=True):
    """Every row's last-layer output in float64, [B, S, K, cout]."""
    C, D, mode, mlp, K, S, N, B = CASES[name]
    pts, feat, ctr = inputs(name, plant)
    _, convs, bns = module(name, last_beta)
    grouped = oracle.group(pts, feat, clamp_index(idx, N), ctr, feature_first=mode == 1)
    y = oracle.mlp_max(grouped.reshape(B, S * K, 1, -1), oracle_layers(convs, bns))
    return y.reshape(B, S, K, -1)


@functools.lru_cache(maxsize=None)
def reference(name, units_pattern, order, last_beta=None, plant=True):
    """(idx, cnt, want): the lists and oracle.mlp_max(oracle.group(...)) in float64
    [B, S, cout], over all K rows of every group (the padding repeats the first neighbour)."""
    C, D, mode, mlp, K, S, N, B = CASES[name]
    seed = 3600 + 100 * sorted(CASES).index(name) + 10 * PATTERNS.index(units_pattern) + ORDERS.index(order)
    idx, cnt = build(B, S, K, N, units_pattern, order, seed)
    want = rows_out(name, idx, last_beta, plant).max(axis=2)
    want.setflags(write=False)
    return idx, cnt, want

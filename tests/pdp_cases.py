"""Forests, rows, grids and the reference shared by test_pdp_paths.py (CPU) and test_pdp_gpu.py.

The forests are those of shap_cases.py (seed 0) plus a depth-33 spine; rows are ``random_rows(1, kinds, N)``. A
numeric feature's grid is the forests' threshold grid (so ``x == thr`` ties are common) plus NaN, +-inf and three
off-grid values; a categorical's is every level plus NaN, -1, n and n + 1 (never +-inf: ``(int)inf`` is undefined in
``k_predict`` too). The reference is what partial dependence did before the grid kernel: overwrite the rows of X
and re-score with ``Forest.predict_raw``.
"""
import numpy as np
import torch

import shap_cases as sc

CASES = dict(sc.CASES)
CASES["spine33"] = ([0] * 30 + [3, 33, 70], dict(depth=33, ntrees=4, spine=True))

NAN, INF = float("nan"), float("inf")

# (case, S) whose tuples must fork: fork_share >= 0.5 at N = 257 (measured values in test_pdp_paths.py)
FORKING = [
    ("f2_depth8", [1]), ("f2_depth8", [0, 1]), ("f3_unused", [2]), ("f3_unused", [0, 2]), ("cats", [4]),
    ("cats", [2]), ("cats", [0, 3]), ("k3", [0, 2]), ("k3", [1]), ("spine33", [0]), ("stump", [0]),
]
# kept for what they exercise, exempt from the floor: a feature nobody splits on, 74 tuples = two chunks with
# 70-level bitsets, wide F, depth-33 walks, a single leaf
EXEMPT = [
    ("f3_unused", [1]), ("cats", [3]), ("f33", [0]), ("f33", [32]), ("f33", [0, 31, 32]), ("spine33", [32]),
    ("single_leaf", [0]), ("single_leaf", [0, 2]),
]
SETS = FORKING + EXEMPT


def set_id(cs):
    return f"{cs[0]}-{'_'.join(map(str, cs[1]))}"


def make_case(name, seed=0):
    kinds, kw = CASES[name]
    return kinds, sc.random_forest(seed, kinds, **kw)


def feature_grid(kind):
    if kind:
        return [float(i) for i in range(kind)] + [NAN, -1.0, float(kind), float(kind + 1)]
    return [float(v) for v in sc.GRID] + [NAN, INF, -INF, 0.25, -0.75, 3.0]


def tuples(kinds, S, G=None):
    """V [|S|, G] float32: ``V[s][k] = grid_s[(k * (1 + 2 s)) % len(grid_s)]``, G = the longest grid unless given
    (the tuple list then repeats)."""
    grids = [feature_grid(kinds[f]) for f in S]
    G = max(len(g) for g in grids) if G is None else G
    V = [[g[(k * (1 + 2 * s)) % len(g)] for k in range(G)] for s, g in enumerate(grids)]
    return torch.tensor(V, dtype=torch.float32).view(len(S), G)


def overwritten(X, S, V, g):
    Xg = X.clone()
    for s, f in enumerate(S):
        Xg[f] = V[s, g]
    return Xg


def reference(forest, X, S, V, t0=0, t1=None):
    """[G, N, K]: overwrite and re-score, on X's device."""
    G = V.shape[1]
    if G == 0:
        return torch.zeros(0, X.shape[1], forest.K, dtype=torch.float32, device=X.device)
    return torch.stack([forest.predict_raw(overwritten(X, S, V.to(X.device), g), t0, t1) for g in range(G)])


def fork_share(forest, X, S, V):
    """Share of (row, tree) pairs whose tuples reach at least 2 distinct leaves."""
    leaves = torch.stack([forest.predict_raw(overwritten(X, S, V, g), return_leaves=True)[1]
                          for g in range(V.shape[1])])                       # [G, N, T]
    return float((leaves != leaves[0]).any(0).double().mean())

"""Two oracles for baseline (interventional) SHAP that never touch the path table of ops/shap.py, shared by
test_shap_baseline_paths.py (CPU) and test_shap_baseline_gpu.py.

Baseline SHAP of a row x against a background row b: the Shapley values of the game ``v(S) = f(x_S, b_~S)``.
Both oracles return float64 ``[N, B, K, F+1]`` (last cell: the bias ``f(b)``), in the margin space, per-tree sums.

1. :func:`brute_force`: the Shapley sum over every subset of F <= 6 features; hybrid rows are scored by
   :func:`walk`, a plain fp64 walk of the ``forest.trees`` node tables.
2. :func:`node_recursion`: for any F. x and b walk a tree together; where they part, x's child is followed with
   the feature marked "x" and b's child with it marked "b" (a marked feature follows only its mark). A leaf
   reached with ``a`` x-marks and ``c`` b-marks gives ``+value (a-1)! c! / (a+c)!`` to every x-marked feature,
   ``-value a! (c-1)! / (a+c)!`` to every b-marked one, and ``value`` to the bias when ``a == 0``.
"""
from fractions import Fraction
from functools import lru_cache
from itertools import combinations
from math import factorial

import numpy as np


def go_left(tree, n, v):
    """The scoring rule of one split for the value ``v`` of its feature."""
    if v != v:
        return bool(tree.na_left[n])
    if tree.is_cat[n]:
        code = int(v)
        if code < 0 or code >= int(tree.cat_nbits[n]):
            return bool(tree.na_left[n])
        return bool((int(tree.cat_bits[n][code >> 5]) >> (code & 31)) & 1)
    return v < float(tree.thr[n])


def walk(forest, row):
    """Raw margin [K] of one row (a sequence of F values), fp64."""
    out = np.zeros(forest.K, np.float64)
    for tree, cls in zip(forest.trees, forest.tree_class):
        n = 0
        while tree.feat[n] >= 0:
            n = int(tree.left[n]) if go_left(tree, n, float(row[tree.feat[n]])) else int(tree.right[n])
        out[cls] += float(tree.value[n])
    return out


def brute_force(forest, X, Bg):
    """X [F, N], Bg [F, B] float32 arrays -> [N, B, K, F+1]."""
    F, N = X.shape
    B = Bg.shape[1]
    assert F <= 6
    wt = [Fraction(factorial(s) * factorial(F - s - 1), factorial(F)) for s in range(F)]
    out = np.zeros((N, B, forest.K, F + 1), np.float64)
    for i in range(N):
        for j in range(B):
            v = {}
            for mask in range(1 << F):
                v[mask] = walk(forest, [X[f, i] if (mask >> f) & 1 else Bg[f, j] for f in range(F)])
            out[i, j, :, F] = v[0]
            for f in range(F):
                rest = [g for g in range(F) if g != f]
                for s in range(F):
                    for S in combinations(rest, s):
                        mask = sum(1 << g for g in S)
                        out[i, j, :, f] += float(wt[s]) * (v[mask | (1 << f)] - v[mask])
    return out


@lru_cache(maxsize=None)
def _weight(p, q):
    return float(Fraction(factorial(p - 1) * factorial(q), factorial(p + q)))


def node_recursion(forest, X, Bg):
    """X [F, N], Bg [F, B] float32 arrays -> [N, B, K, F+1]."""
    F, N = X.shape
    B = Bg.shape[1]
    out = np.zeros((N, B, forest.K, F + 1), np.float64)

    def rec(tree, n, x, b, marks, phi):
        f = int(tree.feat[n])
        if f < 0:
            val = float(tree.value[n])
            xs = [g for g, m in marks.items() if m == "x"]
            bs = [g for g, m in marks.items() if m == "b"]
            a, c = len(xs), len(bs)
            for g in xs:
                phi[g] += val * _weight(a, c)
            for g in bs:
                phi[g] -= val * _weight(c, a)
            if a == 0:
                phi[F] += val
            return
        lx, lb = go_left(tree, n, float(x[f])), go_left(tree, n, float(b[f]))
        child = lambda left: int(tree.left[n]) if left else int(tree.right[n])
        if f in marks:
            rec(tree, child(lx if marks[f] == "x" else lb), x, b, marks, phi)
        elif lx == lb:
            rec(tree, child(lx), x, b, marks, phi)
        else:
            rec(tree, child(lx), x, b, {**marks, f: "x"}, phi)
            rec(tree, child(lb), x, b, {**marks, f: "b"}, phi)

    for i in range(N):
        for j in range(B):
            for tree, cls in zip(forest.trees, forest.tree_class):
                rec(tree, 0, X[:, i], Bg[:, j], {}, out[i, j, cls])
    return out

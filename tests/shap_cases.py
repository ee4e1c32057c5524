"""Hand-built forests and rows shared by test_shap_paths.py (CPU) and test_shap_gpu.py.

Every cover is > 0 (the fp64 oracle ``explain.tree_shap`` divides by zero fractions). Thresholds and row
values come from one small grid, so ``x == thr`` ties are common; a tenth of the numeric splits have
``thr = +inf``; rows carry NaN, +-inf (numeric columns only: ``(int)inf`` is undefined in the oracle) and the
categorical codes -1, nbits, nbits + 1.
"""
import numpy as np
import torch

from llama_github_io_amd.ops.forest import Forest, Tree

GRID = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], dtype=np.float32)


def random_tree(rng, kinds, depth, p_leaf=0.15, spine=False, skip=None):
    """kinds[f]: 0 = numeric, n > 0 = categorical with n levels. ``spine``: one child of every split is a leaf
    and level d splits on feature d (mod F), so the deepest path has min(depth, F) distinct features.
    ``skip``: a feature no split uses."""
    F = len(kinds)
    usable = [f for f in range(F) if f != skip]
    feat, thr, nal, iscat, bits, nbits, left, right, value, cover = ([] for _ in range(10))

    def new(c):
        feat.append(-1); thr.append(0.0); nal.append(0); iscat.append(0); bits.append(None); nbits.append(0)
        left.append(-1); right.append(-1); value.append(0.0); cover.append(c)
        return len(feat) - 1

    def grow(n, d, may_split):
        if d == depth or not may_split or (d > 0 and not spine and rng.random() < p_leaf):
            value[n] = float(rng.normal()) * 0.1
            return
        f = usable[d % len(usable)] if spine else usable[int(rng.integers(len(usable)))]
        feat[n], nal[n] = f, int(rng.integers(2))
        if kinds[f]:
            nl = kinds[f]
            w = rng.integers(0, 1 << 32, size=(nl + 31) // 32, dtype=np.uint64).astype(np.uint32)
            if nl % 32:
                w[-1] &= np.uint32((1 << (nl % 32)) - 1)
            iscat[n], bits[n], nbits[n] = 1, w, nl
        else:
            thr[n] = float("inf") if rng.random() < 0.1 else float(GRID[int(rng.integers(len(GRID)))])
        u = float(rng.uniform(0.1, 0.9))
        l, r = new(cover[n] * u), new(cover[n] * (1.0 - u))
        left[n], right[n] = l, r
        side = int(rng.integers(2))
        grow(l, d + 1, not spine or side == 0)
        grow(r, d + 1, not spine or side == 1)

    grow(new(float(rng.uniform(50, 100))), 0, True)
    n = len(feat)
    return Tree(feat=np.asarray(feat, np.int32), thr=np.asarray(thr, np.float32), bin=np.zeros(n, np.int32),
                na_left=np.asarray(nal, np.int8), is_cat=np.asarray(iscat, np.int8), cat_bits=bits,
                cat_nbits=np.asarray(nbits, np.int32), left=np.asarray(left, np.int32),
                right=np.asarray(right, np.int32), value=np.asarray(value, np.float32),
                cover=np.asarray(cover, np.float64), gain=np.zeros(n, np.float64))


def random_forest(seed, kinds, depth, ntrees, K=1, **kw):
    rng = np.random.default_rng(seed)
    trees = [random_tree(rng, kinds, depth, **kw) for _ in range(ntrees)]
    return Forest(trees, [i % K for i in range(ntrees)], K)


def random_rows(seed, kinds, N):
    """[F, N] float32; the first rows are the special ones, whatever N is."""
    rng = np.random.default_rng(seed + 1000)
    F = len(kinds)
    X = np.empty((F, N), np.float32)
    for f, k in enumerate(kinds):
        if k:
            col = rng.integers(0, k, size=N).astype(np.float32)
            special = [np.nan, -1.0, float(k), float(k + 1)]
        else:
            col = np.where(rng.random(N) < 0.5, rng.choice(GRID, N), rng.normal(size=N)).astype(np.float32)
            special = [np.nan, np.inf, -np.inf, 0.5]
        for i, v in enumerate(special[:N]):
            col[(i + f) % N if N >= 4 else i] = v
        if N > 8:
            col[rng.integers(4, N, size=max(1, N // 10))] = np.nan
        X[f] = col
    return torch.from_numpy(X)


# name -> (kinds, forest kwargs); ``skip`` names a feature whose column must stay exactly 0
CASES = {
    "stump": ([0], dict(depth=1, ntrees=1)),
    "single_leaf": ([0, 0, 0], dict(depth=0, ntrees=1)),
    "f2_depth8": ([0, 0], dict(depth=8, ntrees=4)),
    "f3_unused": ([0, 0, 0], dict(depth=5, ntrees=4, skip=1)),
    "cats": ([0, 3, 33, 70, 0], dict(depth=6, ntrees=4, p_leaf=0.1)),
    "k3": ([0, 5, 0], dict(depth=4, ntrees=6, K=3)),
    "f33": ([0] * 30 + [3, 33, 70], dict(depth=6, ntrees=4, skip=7)),
}


def make_case(name, seed=0):
    kinds, kw = CASES[name]
    return kinds, random_forest(seed, kinds, **kw)

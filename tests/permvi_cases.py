"""Variants, index rows and the reference shared by test_permvi_paths.py (CPU) and test_permvi_gpu.py.

The forests and rows are those of pdp_cases.py (shap_cases.py plus the depth-33 spine). A variant shuffles one
feature: ``variants(F, 2)`` shuffles every feature twice, ``src_rows`` draws the permutations from one seeded
generator as ``rapids._permutation_varimp`` does, and the special index rows (identity, reversed, all zeros) pin
"never diverges" and "every row takes row 0's value" (NaN or a special code in ``random_rows``). The reference is
what permutation importance did before the kernel: clone X, overwrite the feature's row with the shuffled one and
re-score with ``Forest.predict_raw``.
"""
import torch

import pdp_cases as pc

sc = pc.sc
CASES = pc.CASES
make_case = pc.make_case


def variants(F, repeats=2):
    return list(range(F)) * repeats


def cyclic(F, J):
    """J variants, the features repeating cyclically."""
    return [j % F for j in range(J)]


def src_rows(J, N, seed=7):
    g = torch.Generator().manual_seed(seed)
    if J == 0:
        return torch.zeros(0, N, dtype=torch.long)
    return torch.stack([torch.randperm(N, generator=g) for _ in range(J)])


def identity(J, N):
    return torch.arange(N).repeat(J, 1)


def reversed_rows(J, N):
    return torch.arange(N - 1, -1, -1).repeat(J, 1)


def zeros(J, N):
    return torch.zeros(J, N, dtype=torch.long)


def overwritten(X, f, idx):
    Xp = X.clone()
    Xp[f] = X[f][idx.to(X.device).long()]
    return Xp


def reference(forest, X, feats, src, t0=0, t1=None):
    """[J, N, K]: clone, overwrite and re-score, on X's device."""
    if len(feats) == 0:
        return torch.zeros(0, X.shape[1], forest.K, dtype=torch.float32, device=X.device)
    return torch.stack([forest.predict_raw(overwritten(X, f, src[j]), t0, t1) for j, f in enumerate(feats)])


def diverge_share(forest, X, feats, src):
    """Share of (row, tree) pairs where at least one variant reaches a leaf other than the row's own."""
    own = forest.predict_raw(X, return_leaves=True)[1]                                      # [N, T]
    leaves = torch.stack([forest.predict_raw(overwritten(X, f, src[j]), return_leaves=True)[1]
                          for j, f in enumerate(feats)])                                    # [J, N, T]
    return float((leaves != own[None]).any(0).double().mean())

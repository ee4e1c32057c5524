"""Shared cases of the Extended Isolation Forest scoring tests (test_eif_paths.py, test_eif_gpu.py): the ordered fp64
walk that ``k_eif_path`` (csrc/eif_kernels.hip) must reproduce bit for bit, trained forests, a hand-built forest whose
arithmetic is exact in any order, and the scoring code from before ``ops/eif.py`` kept verbatim as an oracle."""
import numpy as np
import torch

from llama_github_io_amd.models.base import DataInfo
from llama_github_io_amd.models.isoforest import (ExtendedIsolationForestModel, ExtendedIsolationForestTrainer,
                                                  c_factor)

TRAINED = [(3, 0, 64, 7), (5, 4, 256, 9), (33, 16, 256, 5), (28, 27, 300, 4)]     # (F, extension_level, sample_size, T)
ROWS = (1, 63, 64, 65, 257)         # the wave and block edges of k_eif_path (64 lanes, 256 rows per block)
MARGIN = 2.0 ** -40                 # relative distance from a hyperplane below which two summation orders may disagree


def case_id(c):
    return c if isinstance(c, str) else "F{}_ext{}_S{}_T{}".format(*c)


ALL_CASES = TRAINED + ["dyadic"]


def _info(F):
    return DataInfo([f"x{i}" for i in range(F)], np.zeros(F, np.int32), [None] * F, None, None)


_models = {}


def trained(F, ext, sample_size, ntrees):
    """An ExtendedIsolationForestModel grown on the host from ``torch.randn(F, 1500)`` (generator seed F, model seed 3)."""
    key = (F, ext, sample_size, ntrees)
    if key not in _models:
        X = torch.randn(F, 1500, generator=torch.Generator().manual_seed(F))
        tr = ExtendedIsolationForestTrainer(dict(ntrees=ntrees, sample_size=sample_size, extension_level=ext, seed=3))
        _models[key] = tr.fit(X, None, None, None, _info(F))
    return _models[key]


DYADIC_F = 4


def dyadic_trees():
    """Three complete depth-3 trees over 4 features in the trainer's format. Normals and offsets are multiples of 1/8
    in [-4, 4]; every root normal has integer components in [-1, 1], one of them 1 and one of them 0 (feature 3)."""
    rng = np.random.default_rng(11)
    trees = []
    for t in range(3):
        M = 15                                              # heap order: children of i are 2i + 1, 2i + 2
        normal = rng.integers(-32, 33, size=(M, DYADIC_F)) / 8.0
        normal[rng.random((M, DYADIC_F)) < 0.3] = 0.0
        normal[~normal.any(1), 0] = 0.125                   # no split without a hyperplane
        normal[0] = [[1, -1, 1, 0], [-1, 1, 1, 0], [1, 1, -1, 0]][t]
        offset = rng.integers(-32, 33, size=M) / 8.0
        left = np.array([2 * i + 1 if i < 7 else -1 for i in range(M)], dtype=np.int64)
        right = np.array([2 * i + 2 if i < 7 else -1 for i in range(M)], dtype=np.int64)
        nrows = np.array([0] * 7 + [int(v) for v in rng.integers(1, 9, size=8)], dtype=np.int64)
        value = np.array([0.0] * 7 + [3 + float(c_factor(n)) for n in nrows[7:]])
        normal[7:] = 0.0
        offset[7:] = 0.0
        trees.append(dict(normal=normal, offset=offset, left=left, right=right, value=value, nrows=nrows, depth=3))
    return trees


def dyadic_rows(n=257):
    """float32 [4, n], multiples of 1/8 in [-8, 8]; row r < 48 lies exactly on the root hyperplane of tree r % 3."""
    rng = np.random.default_rng(12)
    X = rng.integers(-64, 65, size=(DYADIC_F, n)) / 8.0
    trees = dyadic_trees()
    for r in range(min(48, n)):
        nv, off = trees[r % 3]["normal"][0], trees[r % 3]["offset"][0]
        X[:, r] = rng.integers(-8, 9, size=DYADIC_F) / 8.0          # in [-1, 1]
        j = int(np.nonzero(nv == 1)[0][0])
        X[j, r] = off - sum(nv[k] * X[k, r] for k in range(DYADIC_F) if k != j)     # |.| <= 4 + 2
    assert np.abs(X).max() <= 8 and np.array_equal(X * 8, np.round(X * 8))
    return torch.from_numpy(X.astype(np.float32))


def as_model(trees, F, sample_size):
    m = ExtendedIsolationForestModel("eif_case", dict(ntrees=len(trees), sample_size=sample_size), _info(F))
    m.trees = trees
    m.output["sample_size"] = sample_size
    m.output["ntrees"] = len(trees)
    return m


def model_of(case):
    if case == "dyadic":
        if case not in _models:
            _models[case] = as_model(dyadic_trees(), DYADIC_F, 64)
        return _models[case]
    return trained(*case)


def rows_of(case, n=257):
    """Finite float32 rows [F, n] of a case."""
    if case == "dyadic":
        return dyadic_rows(n)
    F = case[0]
    return torch.randn(F, n, generator=torch.Generator().manual_seed(100 + F))


def with_non_finite(X, poison_feat=None, seed=5):
    """A copy of X with NaN, +inf and -inf in about 5 % of the cells. With ``poison_feat``, row 0 keeps its finite
    values but for a NaN in that feature."""
    g = torch.Generator().manual_seed(seed)
    out = X.clone()
    u = torch.rand(X.shape, generator=g)
    out[u < 0.02] = float("nan")
    out[(u >= 0.02) & (u < 0.035)] = float("inf")
    out[(u >= 0.035) & (u < 0.05)] = float("-inf")
    if poison_feat is not None:
        out[:, 0] = X[:, 0]
        out[poison_feat, 0] = float("nan")
    return out


def root_zero_feature(model):
    """The first feature whose normal component is zero at the root of tree 0, or None (a fully extended root)."""
    z = np.nonzero(np.asarray(model.trees[0]["normal"])[0] == 0)[0]
    return int(z[0]) if len(z) else None


def mojo_trees(model):
    """``load_eif``'s dicts of the model after a MOJO write / read of its tree blobs."""
    from llama_github_io_amd.mojo import algos as A
    kv, blobs = {}, {}
    A.write_eif(model, kv, blobs)
    return A.load_eif(kv, blobs)["trees"]


def _host_tree(tr):
    """(normal, off, left, right, leaf value) of a tree in either format, as ``ops.eif.pack`` defines them."""
    left, right = np.asarray(tr["left"]), np.asarray(tr["right"])
    if "offset" in tr:
        return np.asarray(tr["normal"], np.float64), np.asarray(tr["offset"], np.float64), left, right, np.asarray(tr["value"])
    nrm, pt = torch.as_tensor(tr["normal"]), torch.as_tensor(tr["point"])
    off = (nrm * pt).sum(1).numpy()
    value = np.zeros(len(left))
    todo = [(0, 0)]
    while todo:
        i, d = todo.pop()
        if left[i] < 0:
            value[i] = float(d) + float(c_factor(int(tr["rows"][i])))
        else:
            todo += [(int(left[i]), d + 1), (int(right[i]), d + 1)]
    return nrm.numpy(), off, left, right, value


def walk_reference(X, trees, nan_to_zero, keep_zeros, details=False):
    """The ordered fp64 walk: at a split ``s = 0; for f in the listed features, ascending: s = s + x[f] * n[f]``, every
    product and sum rounded on its own; left iff ``(s - off) <= 0``; the leaf values added in forest order from 0.
    X: float32 [F, N]. Returns the float64 sums [N]; with ``details`` also the smallest relative margin
    ``|s - off| / (|off| + sum |x n|)`` over the nodes each row visits [N] and the leaf each row reaches [T, N]."""
    x = np.asarray(X, dtype=np.float32).astype(np.float64)
    if nan_to_zero:
        x = np.nan_to_num(x, nan=0.0, posinf=np.finfo(np.float64).max, neginf=-np.finfo(np.float64).max)
    N = x.shape[1]
    tot = np.zeros(N)
    margin = np.full(N, np.inf)
    leaves = np.zeros((len(trees), N), dtype=np.int64)
    with np.errstate(all="ignore"):
        for t, tr in enumerate(trees):
            nrm, off, left, right, value = _host_tree(tr)
            todo = [(0, np.arange(N))]
            while todo:
                i, idx = todo.pop()
                if len(idx) == 0:
                    continue
                if left[i] < 0:
                    leaves[t, idx] = i
                    continue
                s = np.zeros(len(idx))
                mass = np.full(len(idx), abs(off[i]))
                for f in range(nrm.shape[1]):
                    if keep_zeros or nrm[i, f] != 0:
                        p = x[f, idx] * nrm[i, f]
                        s = s + p
                        mass = mass + np.abs(p)
                d = s - off[i]
                margin[idx] = np.fmin(margin[idx], np.abs(d) / mass)
                go_left = d <= 0
                todo += [(int(left[i]), idx[go_left]), (int(right[i]), idx[~go_left])]
            tot = tot + value[leaves[t]]
    return (tot, margin, leaves) if details else tot


_refs = {}


def reference(case, mode, finite=True):
    """(rows [F, 257], sums, margins, leaves, trees) of a case, computed once. ``mode``: 'native' (the trainer's trees,
    nan_to_zero, zeros dropped) or 'mojo' (the trees after a MOJO round trip, values pass through, zeros kept)."""
    key = (case_id(case), mode, finite)
    if key not in _refs:
        model = model_of(case)
        X = rows_of(case)
        if not finite:
            X = with_non_finite(X, root_zero_feature(model))
        trees = model.trees if mode == "native" else mojo_trees(model)
        native = mode == "native"
        sums, margin, leaves = walk_reference(X, trees, native, not native, details=True)
        _refs[key] = (X, sums, margin, leaves, trees)
    return _refs[key]


# ---- the scoring code from before ops/eif.py, verbatim ----
def old_path_lengths(trees, X):
    """``ExtendedIsolationForestModel._path_lengths`` as it was: one fp64 GEMM per tree, gathers per level."""
    Xr = torch.nan_to_num(X.T.double(), nan=0.0)
    N = Xr.shape[0]
    tot = torch.zeros(N, dtype=torch.float64, device=Xr.device)
    for tr in trees:
        nrm = torch.as_tensor(tr["normal"], device=Xr.device)          # [nodes, F]
        off = torch.as_tensor(tr["offset"], device=Xr.device)          # [nodes]
        left = torch.as_tensor(tr["left"], device=Xr.device).long()
        right = torch.as_tensor(tr["right"], device=Xr.device).long()
        leafv = torch.as_tensor(tr["value"], device=Xr.device)
        proj = Xr @ nrm.T - off                                         # one GEMM per tree
        node = torch.zeros(N, dtype=torch.long, device=Xr.device)
        for _ in range(int(tr["depth"]) + 1):
            isleaf = left[node] < 0
            go_left = proj.gather(1, node[:, None]).squeeze(1) <= 0
            nxt = torch.where(go_left, left[node], right[node])
            node = torch.where(isleaf, node, nxt)
        tot += leafv[node]
    return tot / max(1, len(trees))


def old_score_eif_mean(trees, X):
    """The mean path length of ``mojo.algos.score_eif`` as it was, over ``load_eif``'s trees."""
    Xr = X.T.double()
    N = Xr.shape[0]
    dev = Xr.device
    tot = torch.zeros(N, dtype=torch.float64, device=dev)
    for tr in trees:
        nrm, pt = tr["normal"].to(dev), tr["point"].to(dev)
        left, right, rows = tr["left"].to(dev), tr["right"].to(dev), tr["rows"].to(dev)
        proj = Xr @ nrm.T - (nrm * pt).sum(1)            # (row - p) . n per node
        node = torch.zeros(N, dtype=torch.long, device=dev)
        height = torch.zeros(N, dtype=torch.float64, device=dev)
        for _ in range(64):
            isleaf = left[node] < 0
            if bool(isleaf.all()):
                break
            go_left = proj.gather(1, node[:, None]).squeeze(1) <= 0     # NaN -> right, as in scoreTree0
            node = torch.where(isleaf, node, torch.where(go_left, left[node], right[node]))
            height = height + (~isleaf).double()
        cf = torch.tensor([float(c_factor(int(r))) for r in tr["rows"].tolist()], dtype=torch.float64, device=dev)
        tot += height + cf[node]
    return tot / max(1, len(trees))

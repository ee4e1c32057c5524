"""References and data shared by test_forest_stages_paths.py (CPU), test_forest_stages_gpu.py and
test_forest_stages_rest.py.

The forests and rows are those of pdp_cases.py / shap_cases.py. ``Forest.predict_raw`` (``k_predict`` on the device)
is the reference for the staged margins and the leaves; the feature frequencies are counted here without deciding a
split again: from the leaf a row reached, climb a parent table built from the ``Tree`` objects and count the
features met on the way up."""
import numpy as np
import pandas as pd
import torch

import h2o
from h2o.tree import H2OTree

import pdp_cases as pc

ROWS = [1, 63, 64, 65, 257]
ALL_CASES = list(pc.CASES)


def climb_counts(forest, leaves, F, t0=0, t1=None):
    """(freq int64 [F, N], depth int64 [T, N]) from ``leaves`` int [T, N] (flat node indices of the trees
    [t0, t1)): per (row, tree) walk up from the leaf through ``parent`` and count ``feat[parent]``."""
    trees = forest.trees[t0:t1]
    leaves = np.asarray(leaves.cpu(), dtype=np.int64)
    T, N = leaves.shape
    freq = np.zeros((F, N), dtype=np.int64)
    depth = np.zeros((T, N), dtype=np.int64)
    base = 0
    for t, tree in enumerate(trees):
        parent = np.full(tree.n_nodes, -1, dtype=np.int64)
        for n in range(tree.n_nodes):
            if tree.feat[n] >= 0:
                parent[tree.left[n]] = n
                parent[tree.right[n]] = n
        per_tree = np.zeros((F, N), dtype=np.int64)
        for i in range(N):
            n = leaves[t, i] - base
            assert 0 <= n < tree.n_nodes and tree.feat[n] < 0, "not a leaf of this tree"
            while parent[n] >= 0:
                n = parent[n]
                per_tree[tree.feat[n], i] += 1
                depth[t, i] += 1
        assert np.array_equal(per_tree.sum(0), depth[t])
        freq += per_tree
        base += tree.n_nodes
    return freq, depth


def check_stages(forest, X, t0=0, t1=None):
    """stage and leaves of ``predict_stages`` against ``predict_raw`` over [t0, t0 + t + 1), bit for bit."""
    t1 = len(forest.trees) if t1 is None else t1
    st, lv = forest.predict_stages(X, t0, t1, leaves=True)
    T, N = t1 - t0, X.shape[1]
    assert st.shape == (T, N) and st.dtype == torch.float32 and st.device == X.device
    assert lv.shape == (T, N) and lv.dtype == torch.int32 and lv.device == X.device
    for t in range(T):
        ref = forest.predict_raw(X, t0, t0 + t + 1)[:, forest.tree_class[t0 + t]]
        assert torch.equal(st[t], ref), f"tree {t0 + t}"
    assert torch.equal(lv, forest.predict_raw(X, t0, t1, return_leaves=True)[1].T.contiguous())
    return st, lv


def check_freq(forest, X, skip=None):
    F, N = X.shape
    lv, fq = forest.predict_stages(X, stage=False, leaves=True, freq=True)
    assert fq.shape == (F, N) and fq.dtype == torch.int32 and fq.device == X.device
    ref, depth = climb_counts(forest, lv, F)
    assert np.array_equal(fq.cpu().numpy().astype(np.int64), ref)
    assert np.array_equal(ref.sum(0), depth.sum(0))
    if skip is not None:
        assert not bool(fq[skip].any())
    return fq


def check_subsets(forest, X):
    """Every combination of requested outputs gives the tensors of the full request; ``out=`` keeps its guard."""
    T, N = len(forest.trees), X.shape[1]
    full = dict(zip(("stage", "leaves", "freq"), forest.predict_stages(X, leaves=True, freq=True)))
    for mask in range(1, 8):
        want = {k: bool(mask >> i & 1) for i, k in enumerate(("stage", "leaves", "freq"))}
        got = forest.predict_stages(X, **want)
        got = (got,) if isinstance(got, torch.Tensor) else got
        names = [k for k in ("stage", "leaves", "freq") if want[k]]
        assert len(got) == len(names)
        for k, g in zip(names, got):
            assert torch.equal(g, full[k]), (mask, k)
    buf = torch.full((T * N + 64,), -7.0, dtype=torch.float32, device=X.device)
    got = forest.predict_stages(X, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got, full["stage"])
    assert bool((buf[T * N:] == -7.0).all()), "cells after the result were written"


# ---- end to end ----
def training_frame(n=300, seed=0):
    h2o.init(verbose=False)
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"a": rng.normal(size=n), "b": rng.normal(size=n), "c": rng.choice(list("xyz"), n)})
    df.loc[::13, "b"] = np.nan
    df["r"] = df.a * 2 + np.nan_to_num(df.b) * df.a + (df.c == "x")
    df["y"] = np.where(df.a + (df.c == "x") + rng.normal(size=n) * 0.3 > 0, "1", "0")
    df["y3"] = np.where(df.a > 0.5, "hi", np.where(df.a + np.nan_to_num(df.b) < -0.5, "lo", "mid"))
    return h2o.H2OFrame(df, column_types={"y": "enum", "y3": "enum"})


X_COLS = ["a", "b", "c"]
PARAMS = dict(ntrees=6, max_depth=3, seed=1)


def estimator(algo, y, fr, **kw):
    from h2o.estimators import H2OGradientBoostingEstimator, H2ORandomForestEstimator
    cls = {"gbm": H2OGradientBoostingEstimator, "drf": H2ORandomForestEstimator}[algo]
    est = cls(**dict(PARAMS, **kw))
    est.train(x=X_COLS, y=y, training_frame=fr)
    return est


def stage_names(n_iter, K=1):
    return [f"T{n + 1}.C{c + 1}" for n in range(n_iter) for c in range(K)]


def model_matrix(est, fr):
    m = est._model
    with_rows = m._adapt(fr)
    return with_rows.model_matrix(m.info, device=m.device)


def check_staged_equals_raw(est, fr):
    """Every column of staged_predict_proba(fr) is the response from ``_raw(X, ntrees=n)``, bit for bit, and the
    last stage is ``predict``."""
    m = est._model
    X, offset = model_matrix(est, fr)
    K = m._trees_per_iter()
    sp = est.staged_predict_proba(fr)
    nb = m.ntrees_built()
    assert sp.names == stage_names(nb, K)
    stages = m.staged_predict_proba(X)
    assert len(stages) == nb
    for n in range(1, nb + 1):
        raw = m._raw(X, ntrees=n)
        assert torch.equal(stages[n - 1], raw), f"margins of stage {n}"
        P = m.score_from_raw(raw, offset)
        P = P.reshape(X.shape[1], -1)
        for c in range(K):
            col = sp._col(f"T{n}.C{c + 1}").data
            assert torch.equal(col, P[:, c].double()), f"stage {n} class {c}"
    return sp


def follow(tree, path):
    node = tree.root_node
    for ch in path:
        node = node.left_child if ch == "L" else node.right_child
    return node


def check_leaf_assignment(est, fr, init_f=0.0):
    """Node_ID names leaves of H2OTree whose predictions sum to the margin; Path leads to the same node."""
    m = est._model
    ids = est.predict_leaf_node_assignment(fr, "Node_ID")
    paths = est.predict_leaf_node_assignment(fr, "Path")
    T = len(m.forest.trees)
    assert ids.names == paths.names == stage_names(T)
    N = fr.nrows
    total = np.full(N, float(init_f), dtype=np.float64)
    abs_total = np.zeros(N, dtype=np.float64)
    for t in range(T):
        tree = H2OTree(est, t)
        c = ids._col(t)
        assert c.type == "int"
        j = c.data.cpu().numpy().astype(np.int64)
        pred = np.asarray(tree.predictions, dtype=np.float64)[j]
        assert not np.isnan(pred).any(), "a Node_ID names a split node"
        total += pred
        abs_total += np.abs(pred)
        pc_ = paths._col(t)
        assert pc_.type == "enum" and list(pc_.domain) == sorted(set(pc_.domain))
        codes = pc_.data.cpu().numpy()
        assert set(np.unique(codes).tolist()) == set(range(len(pc_.domain))), "a path of the domain never occurs"
        reached = {p: follow(tree, p) for p in pc_.domain}
        for p, node in reached.items():
            assert not hasattr(node, "left_child"), "a path ends at a split"
        assert np.array_equal(np.asarray([reached[pc_.domain[k]].id for k in codes]), j)
    X, _ = model_matrix(est, fr)
    # the forest adds T fp32 leaf values in fp32: each add rounds by at most 2^-24 of a partial sum, and no partial
    # sum exceeds the sum of the |leaf values|; the leaf values themselves are exact in fp64
    margin = (m.forest.predict_raw(X)[:, 0].double() + float(init_f)).cpu().numpy()
    assert np.all(np.abs(total - margin) <= T * 2.0 ** -24 * abs_total)
    return ids, paths, total, abs_total


def frames_equal(a, b):
    assert a.names == b.names
    for n in a.names:
        ca, cb = a._col(n), b._col(n)
        assert ca.type == cb.type and (ca.domain is None) == (cb.domain is None)
        if ca.domain is not None:
            assert list(ca.domain) == list(cb.domain)
        assert torch.equal(ca.data.cpu(), cb.data.cpu()), n

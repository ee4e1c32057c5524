"""Partial dependence through ``Forest.predict_raw_grid`` on CPU tensors: the grid API against overwrite-and-rescore,
``Model.score_from_raw`` against ``score_tensor``, the chunked statistics of ``explain._grid_stats`` and the
fork-share floor that keeps the GPU cases of test_pdp_gpu.py from being one leaf per tree."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from llama_github_io_amd import explain
from llama_github_io_amd.models import builder
from llama_github_io_amd.ops.forest import Forest

import pdp_cases as pc

N = 257


@pytest.mark.parametrize("cs", pc.SETS, ids=pc.set_id)
def test_grid_api_equals_overwrite_and_rescore(cs):
    name, S = cs
    kinds, forest = pc.make_case(name)
    X = pc.sc.random_rows(1, kinds, 65)
    V = pc.tuples(kinds, S)
    got = forest.predict_raw_grid(X, S, V)
    assert got.shape == (V.shape[1], 65, forest.K) and got.dtype == torch.float32
    assert torch.equal(got, pc.reference(forest, X, S, V))


def test_grid_api_tree_range_and_out():
    kinds, forest = pc.make_case("k3")
    X = pc.sc.random_rows(1, kinds, 9)
    V = pc.tuples(kinds, [0, 2])
    assert torch.equal(forest.predict_raw_grid(X, [0, 2], V, 1, 5), pc.reference(forest, X, [0, 2], V, 1, 5))
    G = V.shape[1]
    buf = torch.full((G * 9 * 3 + 64,), -7.0)
    got = forest.predict_raw_grid(X, [0, 2], V, out=buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got, pc.reference(forest, X, [0, 2], V))
    assert bool((buf[G * 9 * 3:] == -7.0).all())
    with pytest.raises(ValueError):
        forest.predict_raw_grid(X, [0, 0], pc.tuples(kinds, [0, 0]))
    with pytest.raises(ValueError):
        forest.predict_raw_grid(X, [3], V[:1])


def test_grid_api_empty_shapes():
    kinds, forest = pc.make_case("k3")
    X = pc.sc.random_rows(1, kinds, 5)
    V = pc.tuples(kinds, [1])
    G = V.shape[1]
    assert forest.predict_raw_grid(X, [1], V[:, :0]).shape == (0, 5, 3)
    assert forest.predict_raw_grid(X[:, :0], [1], V).shape == (G, 0, 3)
    empty = Forest([], [], 3).predict_raw_grid(X, [1], V)
    assert empty.shape == (G, 5, 3) and not bool(empty.any())
    none = forest.predict_raw_grid(X, [1], V, 2, 2)
    assert none.shape == (G, 5, 3) and not bool(none.any())


# ---- the floor: at N = 257 at least half of the (row, tree) pairs of these cases reach two or more leaves ----
MEASURED = {"f2_depth8-1": 0.957, "f2_depth8-0_1": 1.0, "f3_unused-2": 0.980, "f3_unused-0_2": 1.0, "cats-4": 0.797,
            "cats-2": 0.696, "cats-0_3": 0.716, "k3-0_2": 0.869, "k3-1": 0.665, "spine33-0": 1.0, "stump-0": 1.0}


@pytest.mark.parametrize("cs", pc.FORKING, ids=pc.set_id)
def test_fork_share_floor(cs):
    name, S = cs
    kinds, forest = pc.make_case(name)
    share = pc.fork_share(forest, pc.sc.random_rows(1, kinds, N), S, pc.tuples(kinds, S))
    print(f"fork_share {pc.set_id(cs)}: {share:.3f} (measured when written: {MEASURED[pc.set_id(cs)]})")
    assert share >= 0.5


def test_unused_feature_never_forks():
    kinds, forest = pc.make_case("f3_unused")
    X = pc.sc.random_rows(1, kinds, N)
    V = pc.tuples(kinds, [1])
    assert pc.fork_share(forest, X, [1], V) == 0.0
    got = forest.predict_raw_grid(X, [1], V)
    assert torch.equal(got, forest.predict_raw(X)[None].expand_as(got))


# ---- score_from_raw is score_tensor without the forest walk ----
@pytest.fixture(scope="module")
def fr():
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n = 1500
    df = pd.DataFrame({"a": rng.normal(size=n), "b": rng.normal(size=n), "c": rng.choice(list("xyz"), n)})
    df.loc[::13, "b"] = np.nan
    df["y"] = np.where(df.a + (df.c == "x") + rng.normal(size=n) * 0.3 > 0.8, "1", "0")     # imbalanced
    df["y3"] = np.where(df.a > 0.5, "hi", np.where(df.a + np.nan_to_num(df.b) < -0.5, "lo", "mid"))
    df["r"] = df.a * 2 + np.nan_to_num(df.b) * df.a
    df["o"] = rng.normal(size=n) * 0.2
    df["w"] = rng.uniform(0.5, 2.0, size=n)
    return h2o.H2OFrame(df, column_types={"y": "enum", "y3": "enum"})


MODELS = {
    "gbm_bernoulli": ("gbm", "y", dict(offset_column="o")),
    "gbm_bernoulli_balanced": ("gbm", "y", dict(balance_classes=True)),
    "gbm_multinomial": ("gbm", "y3", dict()),
    "gbm_multinomial_balanced": ("gbm", "y3", dict(balance_classes=True)),
    "gbm_gaussian": ("gbm", "r", dict(offset_column="o")),
    "drf_regression": ("drf", "r", dict()),
    "drf_binomial": ("drf", "y", dict()),
    "drf_binomial_balanced": ("drf", "y", dict(balance_classes=True)),
    "xgboost": ("xgboost", "y", dict()),
    "isolationforest": ("isolationforest", None, dict()),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_score_from_raw_equals_score_tensor(fr, name):
    algo, y, extra = MODELS[name]
    kw = dict(x=["a", "b", "c"], training_frame=fr)
    if y is not None:
        kw["y"] = y
    m = builder.train(algo, dict(ntrees=6, max_depth=4, seed=1, **extra), **kw)
    assert m.scores_from_raw()
    if "balanced" in name:
        assert m.output.get("model_class_distrib")
    X, off = fr.model_matrix(m.info, device=m.device)
    assert (off is not None) == ("offset_column" in extra)
    raw = m.forest.predict_raw(X)
    assert torch.equal(m.score_from_raw(raw, off), m.score_tensor(X, off))
    off2 = torch.linspace(-1, 1, X.shape[1], device=X.device)      # every model takes an offset argument
    assert torch.equal(m.score_from_raw(raw, off2), m.score_tensor(X, off2))


def test_models_without_margins_keep_the_old_path(fr):
    m = builder.train("glm", dict(), x=["a", "b", "c"], y="r", training_frame=fr)
    assert not m.scores_from_raw()


# ---- chunked statistics ----
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_chunked_statistics_agree_with_one_chunk(fr, monkeypatch, weighted):
    """Two and three row chunks merged with Chan's update against the one-chunk expressions: rtol 1e-10. With
    N = 1500 <= 2000 rows the fp64 summation bound N * 2^-53 is 2.2e-13; 1e-10 leaves room for the other formula.
    A gaussian GBM: its response is the fp32 margin plus constants, so a row's response does not depend on which
    chunk scores it (a vectorised fp32 sigmoid on the CPU rounds a row differently in the loop's tail)."""
    m = builder.train("gbm", dict(ntrees=6, max_depth=4, seed=1), x=["a", "b", "c"], y="r", training_frame=fr)
    X, off = fr.model_matrix(m.info, device=torch.device("cpu"))
    X = X[:, :1500]
    w = fr._col("w").as_float().double().cpu() if weighted else None
    V = torch.tensor([[-1.5, -0.5, -1.0, 0.3, 0.8, 1.0, float("nan")]], dtype=torch.float32)
    pick = lambda P: P
    m.forest.invalidate()
    m.device = torch.device("cpu")
    one = np.array(explain._grid_stats(m, X, off, w, [0], V, pick))
    assert (one[:, 1] > 1e-3).all()                # no degenerate spread in this check
    per_row = V.shape[1] * m.forest.K * 4
    calls, inner = [], explain._grid_response
    monkeypatch.setattr(explain, "_grid_response", lambda *a: calls.append(a[1].shape[1]) or inner(*a))
    for chunks in (2, 3):
        calls.clear()
        monkeypatch.setattr(explain, "PDP_CHUNK_BYTES", per_row * -(-1500 // chunks))
        got = np.array(explain._grid_stats(m, X, off, w, [0], V, pick))
        np.testing.assert_allclose(got, one, rtol=1e-10, atol=0)
        assert len(calls) == chunks and sum(calls) == 1500

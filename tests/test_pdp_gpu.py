"""k_pd_node_masks / k_predict_grid (csrc/pdp_kernels.hip) against overwrite-and-rescore through ``k_predict``, and
the device path of ``partial_plot`` / ``h`` against the ``H2O_PDP_HIP=0`` loop.

The kernel checks are bitwise (``torch.equal``): the grid kernel adds the same fp32 leaf values in the same (forest)
order as ``k_predict``. The end-to-end checks allow rtol 1e-10 on fp64 statistics of identical fp32 responses."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from llama_github_io_amd import explain
from llama_github_io_amd.models import builder

import pdp_cases as pc

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257]
TUPLES = [1, 2, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_cache = {}


def case(name, dev):
    """(kinds, forest, rows [F, 257] on the device), built once per module."""
    if name not in _cache:
        kinds, forest = pc.make_case(name)
        _cache[name] = (kinds, forest, pc.sc.random_rows(1, kinds, max(ROWS)).to(dev))
    return _cache[name]


def check(forest, X, S, V, t0=0, t1=None):
    V = V.to(X.device)
    ref = pc.reference(forest, X, S, V, t0, t1)
    n = ref.numel()
    buf = torch.full((n + 64,), -7.0, dtype=torch.float32, device=X.device)
    got = forest.predict_raw_grid(X, S, V, t0, t1, out=buf)
    assert got.shape == ref.shape and got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, ref)
    assert bool((buf[n:] == -7.0).all()), "cells after the result were written"


@pytest.mark.parametrize("cs", pc.SETS, ids=pc.set_id)
def test_kernel_equals_k_predict(cs, dev):
    name, S = cs
    kinds, forest, X = case(name, dev)
    V = pc.tuples(kinds, S)
    for n in ROWS:
        check(forest, X[:, :n].contiguous(), S, V)


@pytest.mark.parametrize("name,S", [("cats", [2]), ("cats", [0, 3]), ("f2_depth8", [1])])
def test_tuple_counts(name, S, dev):
    kinds, forest, X = case(name, dev)
    for G in TUPLES:
        check(forest, X[:, :65].contiguous(), S, pc.tuples(kinds, S, G))


def test_every_feature_and_three_features(dev):
    kinds, forest, X = case("f2_depth8", dev)
    check(forest, X, [0, 1], pc.tuples(kinds, [0, 1]))
    check(forest, X, [1, 0], pc.tuples(kinds, [1, 0]))
    kinds, forest, X = case("cats", dev)
    check(forest, X, [3, 0, 2], pc.tuples(kinds, [3, 0, 2]))
    check(forest, X, [0, 1, 2, 3, 4], pc.tuples(kinds, [0, 1, 2, 3, 4]))


def test_tree_ranges_and_classes(dev):
    kinds, forest, X = case("k3", dev)
    V = pc.tuples(kinds, [0, 2])
    for t0, t1 in [(0, None), (1, 5), (2, 3), (0, 1), (4, 6)]:
        check(forest, X, [0, 2], V, t0, t1)
    assert forest.predict_raw_grid(X, [0, 2], V.to(dev), 3, 3).shape == (V.shape[1], X.shape[1], 3)


def test_mask_workspace_batches(dev, monkeypatch):
    """Tuples beyond the mask workspace go in further launches of the launcher's loop."""
    from llama_github_io_amd.ops import forest as fo
    kinds, forest, X = case("cats", dev)
    n_nodes = sum(t.n_nodes for t in forest.trees)
    monkeypatch.setattr(fo, "PD_MASK_BYTES", 8 * n_nodes)          # one chunk per launch
    check(forest, X[:, :65].contiguous(), [3], pc.tuples(kinds, [3], 130))


# ---- end to end ----
@pytest.fixture(scope="module")
def fr():
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n = 1500
    df = pd.DataFrame({"a": rng.normal(size=n), "b": rng.normal(size=n), "c": rng.choice(list("xyz"), n)})
    df.loc[::13, "b"] = np.nan
    df["y"] = np.where(df.a + (df.c == "x") + rng.normal(size=n) * 0.3 > 0, "1", "0")
    df["y3"] = np.where(df.a > 0.5, "hi", np.where(df.a + np.nan_to_num(df.b) < -0.5, "lo", "mid"))
    df["r"] = df.a * 2 + np.nan_to_num(df.b) * df.a
    df["o"] = rng.normal(size=n) * 0.2
    df["w"] = rng.uniform(0.5, 2.0, size=n)
    return h2o.H2OFrame(df, column_types={"y": "enum", "y3": "enum"})


MODELS = {
    "gbm_bernoulli": ("gbm", "y", dict(), None),
    "gbm_multinomial": ("gbm", "y3", dict(), ["hi", "lo"]),
    "drf_regression": ("drf", "r", dict(), None),
    "xgboost_binomial": ("xgboost", "y", dict(), None),
    "gbm_weights_offset": ("gbm", "y", dict(weights_column="w", offset_column="o"), None),
}


def both(monkeypatch, fn):
    monkeypatch.setenv("H2O_PDP_HIP", "0")
    old = fn()
    monkeypatch.delenv("H2O_PDP_HIP")
    return fn(), old


def same_tables(new, old):
    assert list(new) == list(old)
    for key in old:
        assert len(new[key]) == len(old[key])
        for a, b in zip(new[key], old[key]):
            assert list(a) == list(b)
            for lab in ("value", "value2"):
                if lab in b:
                    assert a[lab] == b[lab] or (a[lab] != a[lab] and b[lab] != b[lab])
            for q in ("mean_response", "stddev_response", "std_error_mean_response"):
                np.testing.assert_allclose(a[q], b[q], rtol=1e-10, atol=0, err_msg=f"{key} {a['value']} {q}")


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, fr):
    algo, y, extra, targets = MODELS[request.param]
    m = builder.train(algo, dict(ntrees=8, max_depth=5, seed=1, **extra), x=["a", "b", "c"], y=y, training_frame=fr)
    assert str(m.device).startswith("cuda") and m.scores_from_raw()
    return m, targets


CALLS = {
    "numeric": dict(cols=["a"], nbins=20),
    "enum_na": dict(cols=["c"], include_na=True),
    "user_splits": dict(cols=["b"], user_splits={"b": [-1.0, 0.0, 0.25, 2.0]}, include_na=True),
    "pair": dict(cols=[], nbins=6, col_pairs_2dpdp=[["a", "c"], ["a", "b"]]),
    "ice": dict(cols=["a", "c"], nbins=7, row_index=3),
    "weights": dict(cols=["c", "b"], nbins=9, weight_column="w"),
}


@pytest.mark.parametrize("call", list(CALLS))
def test_partial_plot_equals_rescoring_loop(model, fr, call, monkeypatch):
    m, targets = model
    seen = []
    inner = m.forest.predict_raw_grid
    monkeypatch.setattr(m.forest, "predict_raw_grid", lambda *a, **k: seen.append(1) or inner(*a, **k))
    new, old = both(monkeypatch, lambda: explain.partial_plot(m, fr, targets=targets, **CALLS[call]))
    assert seen, "the device path did not run"
    n_before = len(seen)
    same_tables(new, old)
    assert len(seen) == n_before


def test_partial_plot_row_chunks(model, fr, monkeypatch):
    """Three row chunks through Chan's merge against the loop. The other columns vary under every tuple here, so
    no standard deviation is rounding noise around zero."""
    m, targets = model
    monkeypatch.setattr(explain, "PDP_CHUNK_BYTES", 9 * m.forest.K * 4 * 500)       # 9 tuples: 500 rows per chunk
    calls, inner = [], explain._grid_response
    monkeypatch.setattr(explain, "_grid_response", lambda *a: calls.append(a[1].shape[1]) or inner(*a))
    new, old = both(monkeypatch, lambda: explain.partial_plot(m, fr, ["b"], nbins=9, targets=targets,
                                                              weight_column="w"))
    assert calls == [500, 500, 500] * len(targets or [None])
    same_tables(new, old)


def test_h_equals_rescoring_loop(model, fr, monkeypatch):
    m, _ = model
    new, old = both(monkeypatch, lambda: explain.h(m, fr, ["a", "b"]))
    np.testing.assert_allclose(new, old, rtol=1e-10, atol=0)


@pytest.mark.parametrize("algo", ["dt", "glm"])
def test_unsupported_model_is_unchanged(fr, algo, monkeypatch):
    m = builder.train(algo, dict(seed=1) if algo == "dt" else dict(), x=["a"], y="y", training_frame=fr)
    assert not m.scores_from_raw()
    new, old = both(monkeypatch, lambda: explain.partial_plot(m, fr, ["a"], nbins=5))
    assert new == old

"""k_predict_permuted (csrc/permute_kernels.hip) against clone-overwrite-and-rescore through ``k_predict``, and the
device path of ``rapids._permutation_varimp`` / ``permutation_importance`` / ``(PermutationVarImp ...)`` against the
``H2O_PERMVI_HIP=0`` loop.

The kernel checks are bitwise (``torch.equal``): the kernel adds the same fp32 leaf values in the same (forest)
order as ``k_predict``, one add per tree and cell. End to end the margins are therefore bit-equal too and the two
paths may differ only by the run-to-run spread of the metric kernels, which ``loop_spread`` measures on the
``H2O_PERMVI_HIP=0`` loop alone (two runs, same seed): the three numeric columns must be equal when that spread
is 0 and within 4x the largest relative spread otherwise. Spread observed on an MI355X when this was written: 0
(bit-identical) for every model and call below."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from h2o.model_api import ModelBaseAPI
from llama_github_io_amd import rapids
from llama_github_io_amd.core import dkv
from llama_github_io_amd.models import builder
from llama_github_io_amd.ops import forest as fo

import permvi_cases as pv

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257]
COUNTS = [1, 2, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_cache = {}


def case(name, dev):
    """(kinds, forest, rows [F, 257] on the device), built once per module."""
    if name not in _cache:
        kinds, forest = pv.make_case(name)
        _cache[name] = (kinds, forest, pv.sc.random_rows(1, kinds, max(ROWS)).to(dev))
    return _cache[name]


def check(forest, X, feats, src, t0=0, t1=None, chunks=(None, 64)):
    """One reference, the kernel at the module's chunk size and at 64 variants per chunk (the full 64-bit mask;
    66 variants are then two chunks, the second of 2)."""
    ref = pv.reference(forest, X, feats, src, t0, t1)
    n = ref.numel()
    default = fo.PV_CHUNK
    try:
        for c in chunks:
            fo.PV_CHUNK = default if c is None else c
            buf = torch.full((n + 64,), -7.0, dtype=torch.float32, device=X.device)
            got = forest.predict_raw_permuted(X, feats, src, t0, t1, out=buf)
            assert got.shape == ref.shape and got.data_ptr() == buf.data_ptr()
            assert torch.equal(got, ref), f"chunk size {fo.PV_CHUNK}"
            assert bool((buf[n:] == -7.0).all()), "cells after the result were written"
    finally:
        fo.PV_CHUNK = default


@pytest.mark.parametrize("name", list(pv.CASES))
def test_kernel_equals_k_predict(name, dev):
    kinds, forest, X = case(name, dev)
    feats = pv.variants(len(kinds), 2)
    for n in ROWS:
        check(forest, X[:, :n].contiguous(), feats, pv.src_rows(len(feats), n))


@pytest.mark.parametrize("name", ["cats", "f2_depth8"])
def test_variant_counts(name, dev):
    kinds, forest, X = case(name, dev)
    X = X[:, :65].contiguous()
    for J in COUNTS:
        check(forest, X, pv.cyclic(len(kinds), J), pv.src_rows(J, 65).to(dev))


@pytest.mark.parametrize("name", ["cats", "k3"])
def test_special_index_rows(name, dev):
    kinds, forest, X = case(name, dev)
    feats = pv.variants(len(kinds), 2)
    N = X.shape[1]
    for rows in (pv.identity, pv.reversed_rows, pv.zeros):
        check(forest, X, feats, rows(len(feats), N))
    got = forest.predict_raw_permuted(X, feats, pv.identity(len(feats), N))
    assert torch.equal(got, forest.predict_raw(X)[None].expand_as(got))


def test_tree_ranges_and_classes(dev):
    kinds, forest, X = case("k3", dev)
    feats = pv.variants(3, 2)
    src = pv.src_rows(6, X.shape[1])
    for t0, t1 in [(0, None), (1, 5), (2, 3), (0, 1), (4, 6)]:
        check(forest, X, feats, src, t0, t1)
    none = forest.predict_raw_permuted(X, feats, src, 3, 3)
    assert none.shape == (6, X.shape[1], 3) and not bool(none.any())


def test_chunk_loop_of_the_launcher(dev, monkeypatch):
    """Chunks beyond one launch's share go in further launches of the launcher's loop."""
    kinds, forest, X = case("cats", dev)
    X = X[:, :65].contiguous()
    feats, src = pv.cyclic(5, 130), pv.src_rows(130, 65)
    monkeypatch.setattr(fo, "PV_LAUNCH_CHUNKS", 1)              # one chunk per launch: 3 launches at 64, 9 at 16
    check(forest, X, feats, src, chunks=(64, 16, 7))
    monkeypatch.setattr(fo, "PV_LAUNCH_CHUNKS", 2)              # the last launch has one chunk, of 2 or 4 variants
    check(forest, X, feats, src, chunks=(64, 16, 7))


def test_value_errors_on_device(dev):
    kinds, forest, X = case("k3", dev)
    feats, src = pv.variants(3, 2), pv.src_rows(6, X.shape[1])
    with pytest.raises(ValueError):
        forest.predict_raw_permuted(X[:2].contiguous(), [0, 1], src[:2])        # the forest splits on feature 2
    bad = src.clone()
    bad[5, 0] = X.shape[1]
    for s in (bad, bad.to(dev), -1 - src):
        with pytest.raises(ValueError):
            forest.predict_raw_permuted(X, feats, s)
    with pytest.raises(ValueError):
        forest.predict_raw_permuted(X, feats, src, out=torch.empty(6 * X.shape[1] * 3))        # host buffer


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
    return h2o.H2OFrame(df, column_types={"y": "enum", "y3": "enum"})


MODELS = {
    "gbm_bernoulli": ("gbm", "y", "logloss"),
    "gbm_multinomial": ("gbm", "y3", "logloss"),
    "drf_regression": ("drf", "r", "RMSE"),
    "xgboost_binomial": ("xgboost", "y", "logloss"),
}
NUMERIC = ["Relative Importance", "Scaled Importance", "Percentage"]


class Api(ModelBaseAPI):
    """The client-side model methods around a trained model."""

    def __init__(self, m):
        self._model = m

    def _m(self):
        return self._model


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, fr):
    algo, y, metric = MODELS[request.param]
    m = builder.train(algo, dict(ntrees=8, max_depth=5, seed=1), x=["a", "b", "c"], y=y, training_frame=fr)
    assert str(m.device).startswith("cuda") and m.scores_from_raw()
    return m, metric


def frame_of(t):
    return t if isinstance(t, pd.DataFrame) else t.as_data_frame()


def loop_spread(monkeypatch, fn):
    """(the loop's table, largest relative difference of the numeric columns between two runs of the loop)."""
    monkeypatch.setenv("H2O_PERMVI_HIP", "0")
    a, b = frame_of(fn()), frame_of(fn())
    monkeypatch.delenv("H2O_PERMVI_HIP")
    assert list(a["Variable"]) == list(b["Variable"])
    x, y = a[NUMERIC].to_numpy(), b[NUMERIC].to_numpy()
    return a, float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300), initial=0.0))


def agree(monkeypatch, m, fn):
    calls = []
    inner = m.forest.predict_raw_permuted
    monkeypatch.setattr(m.forest, "predict_raw_permuted", lambda *a, **k: calls.append(1) or inner(*a, **k))
    old, spread = loop_spread(monkeypatch, fn)
    assert not calls, "H2O_PERMVI_HIP=0 ran the device path"
    new = frame_of(fn())
    assert calls, "the device path did not run"
    print(f"run-to-run relative spread of the loop: {spread:.3g}")
    assert list(new["Variable"]) == list(old["Variable"])
    x, y = new[NUMERIC].to_numpy(), old[NUMERIC].to_numpy()
    if spread == 0.0:
        assert np.array_equal(x, y)
    else:
        np.testing.assert_allclose(x, y, rtol=4 * spread, atol=0)


@pytest.mark.parametrize("n_repeats", [1, 2])
@pytest.mark.parametrize("which", ["AUTO", "named"])
def test_permutation_varimp_equals_loop(model, fr, which, n_repeats, monkeypatch):
    m, metric = model
    agree(monkeypatch, m, lambda: rapids._permutation_varimp(m, fr, "AUTO" if which == "AUTO" else metric,
                                                             n_repeats, seed=3))


def test_variant_chunks(model, fr, monkeypatch):
    """Two variants per chunk of the wiring: the permutations are still drawn in the loop's order."""
    m, metric = model
    monkeypatch.setattr(rapids, "PERMVI_CHUNK_BYTES", 2 * 1500 * (m.forest.K + 1) * 4)
    agree(monkeypatch, m, lambda: rapids._permutation_varimp(m, fr, "AUTO", 3, seed=5))


def test_permutation_importance_api(model, fr, monkeypatch):
    m, metric = model
    agree(monkeypatch, m, lambda: Api(m).permutation_importance(fr, n_repeats=2, features=["a", "c"], seed=3,
                                                                use_pandas=True))


def test_rapids_primitive(model, fr, monkeypatch):
    m, metric = model
    dkv.put("permvi_model", m)
    dkv.put("permvi_frame", fr)
    agree(monkeypatch, m, lambda: rapids.rapids("(PermutationVarImp permvi_model permvi_frame 'AUTO' -1 2 [] 3)"))


@pytest.mark.parametrize("algo", ["glm", "gbm_cpu"])
def test_other_models_keep_the_loop(fr, algo, monkeypatch):
    if algo == "glm":
        m = builder.train("glm", dict(), x=["a", "b", "c"], y="y", training_frame=fr)
        assert not m.scores_from_raw()
    else:
        m = builder.train("gbm", dict(ntrees=4, max_depth=3, seed=1), x=["a", "b", "c"], y="y", training_frame=fr)
        m.forest.invalidate()
        m.device = torch.device("cpu")
    calls = []
    monkeypatch.setattr(fo.Forest, "predict_raw_permuted", lambda *a, **k: calls.append(1))
    new = frame_of(rapids._permutation_varimp(m, fr, "AUTO", 2, seed=3))
    monkeypatch.setenv("H2O_PERMVI_HIP", "0")
    old = frame_of(rapids._permutation_varimp(m, fr, "AUTO", 2, seed=3))
    assert not calls
    assert list(new["Variable"]) == list(old["Variable"])
    if algo == "gbm_cpu":
        assert np.array_equal(new[NUMERIC].to_numpy(), old[NUMERIC].to_numpy())
    else:
        # the same loop twice on the device: equal up to the metric kernels' own run-to-run spread
        third = frame_of(rapids._permutation_varimp(m, fr, "AUTO", 2, seed=3))
        x, y, z = (t[NUMERIC].to_numpy() for t in (new, old, third))
        spread = float(np.max(np.abs(y - z) / np.maximum(np.abs(y), 1e-300), initial=0.0))
        if spread == 0.0:
            assert np.array_equal(x, y)
        else:
            np.testing.assert_allclose(x, y, rtol=4 * spread, atol=0)

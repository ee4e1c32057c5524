"""Path-decomposed TreeSHAP (ops/shap.py) on CPU tensors against the fp64 recursion ``explain.tree_shap``,
and the h2o-py ``top_n`` / ``bottom_n`` / ``compare_abs`` output of ``predict_contributions``."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from h2o.estimators import H2OGradientBoostingEstimator
from llama_github_io_amd import explain
from llama_github_io_amd.ops import shap

import shap_cases as sc

N_ROWS = 41


@pytest.fixture(scope="module", params=list(sc.CASES))
def case(request):
    kinds, forest = sc.make_case(request.param)
    X = sc.random_rows(1, kinds, N_ROWS)
    ref = explain.tree_shap(forest, X)
    ref.setflags(write=False)
    return request.param, kinds, forest, X, ref


def test_path_table_shape(case):
    name, kinds, forest, X, ref = case
    t = shap.forest_paths(forest)
    assert t.n_paths == sum(tr.n_leaves() for tr in forest.trees)
    assert t.G in (8, 16, 32, 64) and t.max_len <= t.G and t.max_len == int(t.len.max())
    # element 0 is the dummy root; elements of one path name distinct features; padding is inert
    assert (t.feat[:, 0] == -1).all() and (t.zf[:, 0] == 1.0).all()
    for p in range(t.n_paths):
        f = t.feat[p, 1:t.len[p]]
        assert (f >= 0).all() and len(set(f.tolist())) == len(f)
        assert (t.feat[p, t.len[p]:] == -1).all() and (t.zf[p, t.len[p]:] == 1.0).all()
    assert (t.cls == np.asarray(forest.tree_class)[t.tree]).all()
    assert shap.forest_paths(forest) is t                      # cached on the forest
    if name == "single_leaf":
        assert t.n_paths == 1 and t.max_len == 1
    if name == "f2_depth8":
        assert t.max_len == 3                                  # depth 8 over two features: merged intervals


def test_matches_oracle(case):
    name, kinds, forest, X, ref = case
    got = shap.path_shap(shap.forest_paths(forest), X, forest.K)
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape
    err = np.abs(got.numpy() - ref).max()
    print(name, "max |path - oracle| =", err, "max |phi| =", np.abs(ref).max())
    assert err <= 1e-12 * max(1.0, np.abs(ref).max())


def test_unused_feature_is_exactly_zero(case):
    name, kinds, forest, X, ref = case
    skip = sc.CASES[name][1].get("skip")
    if name == "single_leaf":
        unused = list(range(len(kinds)))
    elif skip is not None:
        unused = [skip]
    else:
        used = set(np.concatenate([t.feat for t in forest.trees]).tolist())
        unused = [f for f in range(len(kinds)) if f not in used]
    got = shap.path_shap(shap.forest_paths(forest), X, forest.K)
    for f in unused:
        assert (got[:, :, f] == 0.0).all()
    if name in ("single_leaf", "f3_unused", "f33"):
        assert unused


def test_rows_sum_to_prediction(case):
    name, kinds, forest, X, ref = case
    got = shap.path_shap(shap.forest_paths(forest), X, forest.K)
    raw = forest.predict_raw(X).double()
    assert (got.sum(-1) - raw).abs().max() < 1e-5


def test_tree_shap_device_on_cpu_tensor(case):
    name, kinds, forest, X, ref = case
    got = explain.tree_shap_device(forest, X)
    assert isinstance(got, torch.Tensor) and got.device.type == "cpu"
    assert np.abs(got.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_categorical_splits_of_different_width_on_one_path():
    """Two splits of feature 0 with 3 and 5 levels (and opposite NA directions) under each other: a code past a
    split's own width takes that split's NA direction."""
    from llama_github_io_amd.ops.forest import Forest, Tree
    i32, w = np.int32, lambda v: np.asarray([v], np.uint32)
    for nb_root, nb_child, nal_root, nal_child in [(3, 5, 1, 0), (5, 3, 0, 1), (3, 5, 0, 0), (70, 3, 1, 1)]:
        root_bits = w(0b101) if nb_root <= 32 else np.asarray([0x0F0F0F0F, 0x12345678, 0x2A], np.uint32)
        t = Tree(feat=np.asarray([0, 0, -1, 1, -1, -1, -1], i32), thr=np.asarray([0, 0, 0, 0.5, 0, 0, 0], np.float32),
                 bin=np.zeros(7, i32), na_left=np.asarray([nal_root, nal_child, 0, 1, 0, 0, 0], np.int8),
                 is_cat=np.asarray([1, 1, 0, 0, 0, 0, 0], np.int8),
                 cat_bits=[root_bits, w(0b10011 & ((1 << nb_child) - 1)), None, None, None, None, None],
                 cat_nbits=np.asarray([nb_root, nb_child, 0, 0, 0, 0, 0], i32),
                 left=np.asarray([1, 3, -1, 5, -1, -1, -1], i32), right=np.asarray([2, 4, -1, 6, -1, -1, -1], i32),
                 value=np.asarray([0, 0, 0.3, 0, -0.2, 0.7, -0.4], np.float32),
                 cover=np.asarray([10, 6, 4, 4, 2, 3, 1], np.float64), gain=np.zeros(7))
        forest = Forest([t], [0], 1)
        codes = np.asarray([np.nan, -1, 0, 1, 2, 3, 4, 5, 6, 33, 69, 70, 71], np.float32)
        X = torch.from_numpy(np.stack([codes, np.linspace(-1, 2, len(codes)).astype(np.float32)]))
        ref = explain.tree_shap(forest, X)
        got = shap.path_shap(shap.forest_paths(forest), X, 1).numpy()
        assert np.abs(got - ref).max() <= 1e-12
        assert np.abs(got.sum(-1)[:, 0] - forest.predict_raw(X)[:, 0].double().numpy()).max() < 1e-5


def test_cache_dropped_when_forest_changes():
    kinds, forest = sc.make_case("f3_unused")
    t = shap.forest_paths(forest)
    extra = sc.random_tree(np.random.default_rng(9), kinds, 3)
    forest.add(extra, 0)
    t2 = shap.forest_paths(forest)
    assert t2 is not t and t2.n_paths == t.n_paths + extra.n_leaves()
    forest.invalidate()
    assert shap.forest_paths(forest) is not t2


def test_over_length_falls_back_to_recursion(monkeypatch):
    kinds, forest = sc.make_case("f33")
    X = sc.random_rows(1, kinds, N_ROWS)
    assert shap.forest_paths(forest).max_len > 4
    monkeypatch.setattr(shap, "MAX_PATH_LEN", 4)
    with pytest.raises(ValueError):
        shap.path_shap(shap.forest_paths(forest), X, forest.K)
    got = explain.tree_shap_device(forest, X)
    assert np.array_equal(got.numpy(), explain.tree_shap(forest, X))


def test_feature_out_of_range_is_refused():
    kinds, forest = sc.make_case("f33")
    X = sc.random_rows(1, kinds, 8)
    with pytest.raises(ValueError):
        shap.path_shap(shap.forest_paths(forest), X[:20], forest.K)


# ---- top_n / bottom_n / compare_abs on a small trained GBM (continuous data: no ties)

@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    """The frames below are compared exactly, so on a machine with a GPU they take the host recursion: the device
    path sums with unordered atomics and two of its calls differ in the last bits (tests/test_shap_gpu.py has
    the device side of these checks)."""
    monkeypatch.setenv("H2O_SHAP_HIP", "0")


@pytest.fixture(scope="module")
def gbm():
    h2o.init(verbose=False)
    rng = np.random.default_rng(3)
    n = 400
    df = pd.DataFrame({c: rng.normal(size=n) for c in "abcde"})
    df["r"] = df.a * 2 - df.b + df.c * df.d + rng.normal(size=n) * 0.1
    fr = h2o.H2OFrame(df)
    m = H2OGradientBoostingEstimator(ntrees=6, seed=1, max_depth=4)
    m.train(x=list("abcde"), y="r", training_frame=fr)
    saved = os.environ.get("H2O_SHAP_HIP")
    os.environ["H2O_SHAP_HIP"] = "0"
    try:
        plain = m.predict_contributions(fr).as_data_frame()
    finally:
        if saved is None:
            del os.environ["H2O_SHAP_HIP"]
        else:
            os.environ["H2O_SHAP_HIP"] = saved
    return m, fr, plain


def _names(kind, n):
    return [f"{kind}_{w}_{i + 1}" for i in range(n) for w in ("feature", "value")]


def test_top_bottom_columns_and_order(gbm):
    m, fr, plain = gbm
    feats = list("abcde")
    out = m.predict_contributions(fr, top_n=2, bottom_n=1)
    assert out.names == _names("top", 2) + _names("bottom", 1) + ["BiasTerm"]
    assert out.types["top_feature_1"] == "enum" and out.types["top_value_1"] == "real"
    df = out.as_data_frame()
    phi = plain[feats].values
    assert (df["top_value_1"] >= df["top_value_2"]).all()
    assert np.array_equal(df["top_value_1"].values, phi.max(1))
    assert np.array_equal(df["bottom_value_1"].values, phi.min(1))
    assert list(df["top_feature_1"]) == [feats[i] for i in phi.argmax(1)]
    assert list(df["bottom_feature_1"]) == [feats[i] for i in phi.argmin(1)]
    assert np.array_equal(df["BiasTerm"].values, plain["BiasTerm"].values)


def test_compare_abs_picks_largest_magnitude(gbm):
    m, fr, plain = gbm
    feats = list("abcde")
    phi = plain[feats].values
    df = m.predict_contributions(fr, top_n=1, bottom_n=1, compare_abs=True).as_data_frame()
    rows = np.arange(len(phi))
    assert np.array_equal(df["top_value_1"].values, phi[rows, np.abs(phi).argmax(1)])
    assert np.array_equal(df["bottom_value_1"].values, phi[rows, np.abs(phi).argmin(1)])
    assert (phi < 0).any() and (df["top_value_1"] < 0).any()     # signed values are reported
    # compare_abs alone sorts every feature by magnitude
    alld = m.predict_contributions(fr, compare_abs=True)
    assert alld.names == _names("top", 5) + ["BiasTerm"]
    v = alld.as_data_frame()[[f"top_value_{i + 1}" for i in range(5)]].abs().values
    assert (np.diff(v, axis=1) <= 0).all()


@pytest.mark.parametrize("kw", [dict(top_n=-1), dict(bottom_n=-1), dict(top_n=3, bottom_n=2), dict(top_n=9)])
def test_all_features_sorted_descending(gbm, kw):
    m, fr, plain = gbm
    feats = list("abcde")
    out = m.predict_contributions(fr, **kw)
    assert out.names == _names("top", 5) + ["BiasTerm"]
    df = out.as_data_frame()
    v = df[[f"top_value_{i + 1}" for i in range(5)]].values
    assert (np.diff(v, axis=1) <= 0).all()
    assert np.array_equal(np.sort(v, axis=1), np.sort(plain[feats].values, axis=1))
    for i in range(5):
        picked = plain[feats].values[np.arange(len(df)), [feats.index(f) for f in df[f"top_feature_{i + 1}"]]]
        assert np.array_equal(picked, v[:, i])
    # every row's values plus BiasTerm still sum to the margin
    mm = m._model
    raw = mm.forest.predict_raw(fr.model_matrix(mm.info)[0])[:, 0].double().cpu().numpy()
    init = mm.init_f[0] if isinstance(mm.init_f, (list, tuple)) else mm.init_f
    assert np.abs(v.sum(1) + df["BiasTerm"].values - (raw + init)).max() < 1e-5


def test_unset_arguments_keep_the_plain_frame(gbm):
    m, fr, plain = gbm
    for kw in (dict(top_n=0, bottom_n=0), dict(top_n=None, compare_abs=False), dict(output_format="Compact")):
        out = m.predict_contributions(fr, **kw)
        assert out.names == list("abcde") + ["BiasTerm"]
        assert np.array_equal(out.as_data_frame().values, plain.values)


def test_bad_output_format_raises(gbm):
    m, fr, plain = gbm
    with pytest.raises(ValueError):
        m.predict_contributions(fr, output_format="Sparse")
    with pytest.raises(ValueError):
        explain.predict_contributions(m, fr, output_format="one_hot")

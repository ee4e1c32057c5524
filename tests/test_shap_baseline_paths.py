"""Baseline (interventional) SHAP on CPU tensors: the PyTorch evaluation of the path table
(``ops.shap.path_shap_baseline``) against the two oracles of shap_baseline_cases.py, and the
``background_frame`` / ``output_space`` / ``output_per_reference`` arguments of ``predict_contributions``.

Bound: 1e-12 relative to ``max(1, max |ref|)``; both sides are fp64 sums of a few hundred terms."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from h2o.estimators import H2OGradientBoostingEstimator
from llama_github_io_amd import explain
from llama_github_io_amd.ops import shap

import shap_baseline_cases as bc
import shap_cases as sc

N_ROWS, N_BG = 12, 9
SMALL = ["stump", "single_leaf", "f2_depth8", "f3_unused", "cats", "k3"]
# the spine forests of tests/test_shap_gpu.py (GPU_CASES), one per lane-group width above 8
F33 = [0] * 30 + [3, 33, 70]
LARGE = {
    "f33": sc.CASES["f33"],
    "f33_g16": (F33, dict(depth=12, ntrees=40, spine=True)),
    "f33_g32": (F33, dict(depth=20, ntrees=10, spine=True)),
    "f33_g64": (F33, dict(depth=33, ntrees=4, spine=True)),
}


# nonzero feature cells asked of the spine forests (test_cases_cover_every_branch): half of what the oracle gives
SPINE_FLOOR = {"f33_g16": 0.120, "f33_g32": 0.085, "f33_g64": 0.054}


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


@pytest.fixture(scope="module", params=SMALL + list(LARGE))
def case(request):
    name = request.param
    kinds, kw = sc.CASES[name] if name in SMALL else LARGE[name]
    forest = sc.random_forest(0, kinds, **kw)
    X, Bg = sc.random_rows(1, kinds, N_ROWS), sc.random_rows(2, kinds, N_BG)
    if name in SMALL:
        ref = bc.brute_force(forest, X.numpy(), Bg.numpy())
    else:
        ref = bc.node_recursion(forest, X.numpy(), Bg.numpy())
    ref.setflags(write=False)
    return name, kinds, kw, forest, X, Bg, ref


def per_pair(forest, X, Bg):
    got = shap.path_shap_baseline(shap.forest_paths(forest), X, Bg, forest.K, per_reference=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (X.shape[1] * Bg.shape[1], forest.K, X.shape[0] + 1)
    return got.view(X.shape[1], Bg.shape[1], forest.K, -1).numpy()


def test_walk_matches_predict_raw(case):
    name, kinds, kw, forest, X, Bg, ref = case
    raw = forest.predict_raw(X).double().numpy()
    mine = np.stack([bc.walk(forest, X[:, i].numpy()) for i in range(X.shape[1])])
    assert np.abs(mine - raw).max() < 1e-5


@pytest.mark.parametrize("name", SMALL)
def test_node_recursion_matches_brute_force(name):
    kinds, forest = sc.make_case(name)
    X, Bg = sc.random_rows(1, kinds, N_ROWS).numpy(), sc.random_rows(2, kinds, N_BG).numpy()
    assert rel_err(bc.node_recursion(forest, X, Bg), bc.brute_force(forest, X, Bg)) <= 1e-12


def test_per_reference_matches_oracle(case):
    name, kinds, kw, forest, X, Bg, ref = case
    got = per_pair(forest, X, Bg)
    err = rel_err(got, ref)
    print(name, "max |table - oracle| =", err, "max |phi| =", np.abs(ref).max())
    assert err <= 1e-12


def test_summed_matches_oracle(case):
    name, kinds, kw, forest, X, Bg, ref = case
    got = shap.path_shap_baseline(shap.forest_paths(forest), X, Bg, forest.K)
    assert tuple(got.shape) == (N_ROWS, forest.K, len(kinds) + 1)
    assert rel_err(got.numpy(), ref.sum(1)) <= 1e-12


def test_efficiency_and_bias(case):
    name, kinds, kw, forest, X, Bg, ref = case
    got = per_pair(forest, X, Bg)
    fx = np.stack([bc.walk(forest, X[:, i].numpy()) for i in range(N_ROWS)])
    fb = np.stack([bc.walk(forest, Bg[:, j].numpy()) for j in range(N_BG)])
    assert np.abs(got[..., :-1].sum(-1) - (fx[:, None] - fb[None])).max() <= 1e-12
    assert np.abs(got[..., -1] - fb[None]).max() <= 1e-12


def test_row_against_itself_is_exactly_zero(case):
    name, kinds, kw, forest, X, Bg, ref = case
    got = per_pair(forest, X, X)
    i = np.arange(N_ROWS)
    assert (got[i, i][..., :-1] == 0.0).all()


def test_unused_feature_is_exactly_zero(case):
    name, kinds, kw, forest, X, Bg, ref = case
    skip = kw.get("skip")
    unused = list(range(len(kinds))) if name == "single_leaf" else [] if skip is None else [skip]
    got = per_pair(forest, X, Bg)
    for f in unused:
        assert (got[..., f] == 0.0).all()
    if name in ("single_leaf", "f3_unused", "f33"):
        assert unused


def test_swapping_row_and_background_negates(case):
    name, kinds, kw, forest, X, Bg, ref = case
    a, b = per_pair(forest, X, Bg), per_pair(forest, Bg, X)
    assert np.array_equal(a[..., :-1], -np.swapaxes(b, 0, 1)[..., :-1])


def test_cases_cover_every_branch(case):
    """The rows must reach every branch of the closed form: mixed paths (elements held by x only and by b only
    together), dead paths (an element refuses both rows), and enough nonzero cells. At least 30 % of the reference's
    feature cells are nonzero in every case but the three spine forests (0.40 for f33, 0.55 - 0.87 for the
    brute-force cases). A spine forest cannot reach 30 %: all its trees split on feature d at level d, one child of
    every split is a leaf, and a pair stops contributing once both rows have left the spine, about two levels down;
    so the nonzero cells sit on the first few of the 33 features, and a depth-12 spine splits on 12 of them at all
    (a cap of 0.36). The oracle gives 0.240 / 0.171 / 0.109 for depth 12 / 20 / 33 with these seeds (the more trees,
    the more cells); those cases are held to half of that."""
    name, kinds, kw, forest, X, Bg, ref = case
    if name in ("stump", "single_leaf"):
        return
    assert (ref[..., :-1] != 0).mean() >= SPINE_FLOOR.get(name, 0.30)
    t = shap.forest_paths(forest)
    d = t.on("cpu")
    real = torch.from_numpy((np.arange(t.G)[None] >= 1) & (np.arange(t.G)[None] < t.len[:, None]))
    fidx = d["feat"].long().clamp(min=0)
    mx = (shap._elements_ok(d, X.T[:, fidx]) & real)[:, None]
    mb = (shap._elements_ok(d, Bg.T[:, fidx]) & real)[None]
    a, c = (mx & ~mb).sum(-1), (mb & ~mx).sum(-1)
    dead = (real & ~mx & ~mb).any(-1)
    assert bool(((a > 0) & (c > 0) & ~dead).any())
    assert bool(dead.any())


def test_weight_table():
    from math import factorial
    kinds, forest = sc.make_case("cats")
    t = shap.forest_paths(forest)
    T = t.baseline_weights("cpu")
    assert t.baseline_weights("cpu") is T and tuple(T.shape) == (t.G, t.G) and T.dtype == torch.float64
    for p in range(1, t.G):
        for q in range(t.G - p):
            assert T[p, q].item() == pytest.approx(factorial(p - 1) * factorial(q) / factorial(p + q), rel=1e-15)


def test_out_is_accumulated_into_and_validated():
    kinds, forest = sc.make_case("k3")
    X, Bg = sc.random_rows(1, kinds, 5), sc.random_rows(2, kinds, 3)
    t = shap.forest_paths(forest)
    ref = shap.path_shap_baseline(t, X, Bg, forest.K, per_reference=True)
    out = torch.ones(16, forest.K, len(kinds) + 1, dtype=torch.float64)
    res = shap.path_shap_baseline(t, X, Bg, forest.K, per_reference=True, out=out)
    assert res is out and torch.equal(out[:15], ref + 1.0) and bool((out[15] == 1.0).all())
    with pytest.raises(ValueError):
        shap.path_shap_baseline(t, X, Bg, forest.K, per_reference=True, out=torch.zeros(14, forest.K, len(kinds) + 1,
                                                                                      dtype=torch.float64))
    with pytest.raises(ValueError):
        shap.path_shap_baseline(t, X, Bg[:2], forest.K)
    with pytest.raises(ValueError):
        shap.path_shap_baseline(t, X[:1], Bg[:1], forest.K)


def test_over_length_forest_is_evaluated(monkeypatch):
    """No lane limit on the PyTorch evaluation."""
    kinds, kw = LARGE["f33"]
    forest = sc.random_forest(0, kinds, **kw)
    X, Bg = sc.random_rows(1, kinds, 4), sc.random_rows(2, kinds, 3)
    ref = shap.path_shap_baseline(shap.forest_paths(forest), X, Bg, forest.K)
    monkeypatch.setattr(shap, "MAX_PATH_LEN", 4)
    assert torch.equal(shap.path_shap_baseline(shap.forest_paths(forest), X, Bg, forest.K), ref)


# ---- predict_contributions(background_frame=...) on the host path

@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    """The frames below are compared closely, so on a machine with a GPU they take the PyTorch evaluation
    (tests/test_shap_baseline_gpu.py has the device side)."""
    monkeypatch.setenv("H2O_SHAP_HIP", "0")


@pytest.fixture(scope="module")
def frames():
    h2o.init(verbose=False)
    rng = np.random.default_rng(5)
    n = 300
    df = pd.DataFrame({c: rng.normal(size=n) for c in "abcde"})
    df.loc[::11, "b"] = np.nan
    df["r"] = df.a * 2 - np.nan_to_num(df.b) + df.c * df.d + rng.normal(size=n) * 0.1
    df["y"] = np.where(df.a - df.c + rng.normal(size=n) * 0.3 > 0, "1", "0")
    fr = h2o.H2OFrame(df, column_types={"y": "enum"})
    return fr, fr[:23, :], fr[250:257, :]


@pytest.fixture(scope="module")
def gbm_reg(frames):
    m = H2OGradientBoostingEstimator(ntrees=6, seed=1, max_depth=4)
    m.train(x=list("abcde"), y="r", training_frame=frames[0])
    return m


@pytest.fixture(scope="module")
def gbm_bin(frames):
    m = H2OGradientBoostingEstimator(ntrees=6, seed=1, max_depth=4)
    m.train(x=list("abcde"), y="y", training_frame=frames[0])
    return m


def margin(m, fr):
    mm = m._model
    raw = mm.forest.predict_raw(fr.model_matrix(mm.info)[0])[:, 0].double().cpu().numpy()
    return raw + (mm.init_f[0] if isinstance(mm.init_f, (list, tuple)) else mm.init_f)


def test_argument_validation(frames, gbm_reg):
    fr, test, bg = frames
    with pytest.raises(ValueError):
        gbm_reg.predict_contributions(test, output_space=True)
    with pytest.raises(ValueError):
        gbm_reg.predict_contributions(test, output_per_reference=True)
    with pytest.raises(ValueError):
        gbm_reg.predict_contributions(test, background_frame=bg[:0, :])
    with pytest.raises(ValueError):
        gbm_reg.predict_contributions(test, background_frame=bg, output_format="Sparse")
    with pytest.raises(ValueError):
        explain.predict_contributions(gbm_reg._model, test, output_per_reference=True)


def test_averaged_and_per_reference_frames(frames, gbm_reg):
    fr, test, bg = frames
    feats = list("abcde")
    N, B = test.nrows, bg.nrows
    avg = gbm_reg.predict_contributions(test, background_frame=bg)
    assert avg.names == feats + ["BiasTerm"] and avg.nrows == N
    per = gbm_reg.predict_contributions(test, background_frame=bg, output_per_reference=True)
    assert per.names == feats + ["BiasTerm", "RowIdx", "BackgroundRowIdx"] and per.nrows == N * B
    assert per.types["RowIdx"] == "int" and per.types["BackgroundRowIdx"] == "int"
    p = per.as_data_frame()
    assert np.array_equal(p["RowIdx"].values, np.repeat(np.arange(N), B))
    assert np.array_equal(p["BackgroundRowIdx"].values, np.tile(np.arange(B), N))
    fx, fb = margin(gbm_reg, test), margin(gbm_reg, bg)
    assert np.abs(p[feats].values.sum(1) - (np.repeat(fx, B) - np.tile(fb, N))).max() < 1e-5
    assert np.abs(p["BiasTerm"].values - np.tile(fb, N)).max() < 1e-5
    mean = p.groupby("RowIdx")[feats + ["BiasTerm"]].mean().values
    assert np.abs(avg.as_data_frame().values - mean).max() <= 1e-12
    # the path-dependent contributions of the same call are another quantity
    plain = gbm_reg.predict_contributions(test).as_data_frame().values
    assert np.abs(plain - mean).max() > 1e-3


def test_top_n_with_background(frames, gbm_reg):
    fr, test, bg = frames
    feats = list("abcde")
    plain = gbm_reg.predict_contributions(test, background_frame=bg).as_data_frame()
    out = gbm_reg.predict_contributions(test, background_frame=bg, top_n=2, bottom_n=1)
    assert out.names == ["top_feature_1", "top_value_1", "top_feature_2", "top_value_2", "bottom_feature_1",
                         "bottom_value_1", "BiasTerm"]
    df = out.as_data_frame()
    phi = plain[feats].values
    assert np.array_equal(df["top_value_1"].values, phi.max(1))
    assert np.array_equal(df["bottom_value_1"].values, phi.min(1))
    assert list(df["top_feature_1"]) == [feats[i] for i in phi.argmax(1)]
    assert np.array_equal(df["BiasTerm"].values, plain["BiasTerm"].values)
    per = gbm_reg.predict_contributions(test, background_frame=bg, top_n=1, output_per_reference=True)
    assert per.names == ["top_feature_1", "top_value_1", "BiasTerm", "RowIdx", "BackgroundRowIdx"]
    assert per.nrows == test.nrows * bg.nrows


def test_output_space_binomial_sums_to_probability(frames, gbm_bin):
    fr, test, bg = frames
    feats = list("abcde")
    N, B = test.nrows, bg.nrows
    p1 = gbm_bin.predict(test).as_data_frame()["1"].values          # p1: the column of level "1"
    pb = gbm_bin.predict(bg).as_data_frame()["1"].values
    per = gbm_bin.predict_contributions(test, background_frame=bg, output_space=True,
                                        output_per_reference=True).as_data_frame()
    assert np.abs(per[feats + ["BiasTerm"]].values.sum(1) - np.repeat(p1, B)).max() < 1e-5
    assert np.abs(per["BiasTerm"].values - np.tile(pb, N)).max() < 1e-5
    avg = gbm_bin.predict_contributions(test, background_frame=bg, output_space=True).as_data_frame()
    assert np.abs(avg.values.sum(1) - p1).max() < 1e-5
    assert np.abs(avg.values - per.groupby("RowIdx")[feats + ["BiasTerm"]].mean().values).max() <= 1e-12
    # in the margin space the same rows sum to the margin, not to the probability
    mar = gbm_bin.predict_contributions(test, background_frame=bg).as_data_frame()
    assert np.abs(mar.values.sum(1) - margin(gbm_bin, test)).max() < 1e-5
    # a row against itself: no feature moves, the bias is its own probability
    own = gbm_bin.predict_contributions(test[:3, :], background_frame=test[:1, :], output_space=True).as_data_frame()
    assert (own[feats].values[0] == 0.0).all() and abs(own["BiasTerm"].values[0] - p1[0]) < 1e-5


def test_output_space_leaves_regression_unchanged(frames, gbm_reg):
    fr, test, bg = frames
    for per in (False, True):
        a = gbm_reg.predict_contributions(test, background_frame=bg, output_per_reference=per).as_data_frame()
        b = gbm_reg.predict_contributions(test, background_frame=bg, output_per_reference=per,
                                          output_space=True).as_data_frame()
        assert np.array_equal(a.values, b.values)


def test_per_reference_size_limit(frames, gbm_reg, monkeypatch):
    fr, test, bg = frames
    monkeypatch.setenv("H2O_SHAP_MAX_OUT_BYTES", "4096")
    with pytest.raises(ValueError, match=f"{test.nrows} rows x {bg.nrows} background rows"):
        gbm_reg.predict_contributions(test, background_frame=bg, output_per_reference=True)
    assert gbm_reg.predict_contributions(test, background_frame=bg).nrows == test.nrows      # the average is not limited


def test_explain_passes_the_background_frame(frames, gbm_reg):
    fr, test, bg = frames
    from h2o.explanation import _explain as ex
    with_bg = ex.shap_explain_row_plot(gbm_reg, test, 2, background_frame=bg).data
    ref = gbm_reg.predict_contributions(test[2:3, :], background_frame=bg).as_data_frame().iloc[0]
    assert with_bg.attrs["bias"] == pytest.approx(ref["BiasTerm"], abs=1e-12)
    plain = ex.shap_explain_row_plot(gbm_reg, test, 2).data
    assert abs(plain.attrs["bias"] - with_bg.attrs["bias"]) > 1e-6
    out = ex.explain_row(gbm_reg, test, 2, include_explanations=["shap_explain_row"], background_frame=bg)
    assert out["shap_explain_row"].data.attrs["bias"] == pytest.approx(ref["BiasTerm"], abs=1e-12)


@pytest.mark.parametrize("algo", ["gbm", "xgboost"])
def test_output_space_log_link_sums_to_prediction(frames, algo):
    """Poisson: the models score ``exp(margin)``, so output-space rows sum to ``predict()`` and the bias is the
    background row's prediction."""
    from h2o.estimators import H2OXGBoostEstimator
    fr, test, bg = frames
    feats = list("abcde")
    counts = fr.as_data_frame()[feats].copy()
    counts["n"] = np.random.default_rng(7).poisson(np.exp(0.5 * counts.a - 0.3 * counts.c))
    cf = h2o.H2OFrame(counts)
    E = H2OGradientBoostingEstimator if algo == "gbm" else H2OXGBoostEstimator
    m = E(ntrees=6, seed=1, max_depth=3, distribution="poisson")
    m.train(x=feats, y="n", training_frame=cf)
    assert explain._margin_linkinv(m._model) is not None
    N, B = test.nrows, bg.nrows
    pred = m.predict(test).as_data_frame()["predict"].values
    pred_bg = m.predict(bg).as_data_frame()["predict"].values
    per = m.predict_contributions(test, background_frame=bg, output_space=True,
                                  output_per_reference=True).as_data_frame()
    tol = 1e-5 * max(1.0, np.abs(pred).max())                               # fp32 scoring
    assert np.abs(per[feats + ["BiasTerm"]].values.sum(1) - np.repeat(pred, B)).max() < tol
    assert np.abs(per["BiasTerm"].values - np.tile(pred_bg, N)).max() < tol
    avg = m.predict_contributions(test, background_frame=bg, output_space=True).as_data_frame()
    assert np.abs(avg.values.sum(1) - pred).max() < tol
    mar = m.predict_contributions(test, background_frame=bg).as_data_frame()
    assert np.abs(mar.values - avg.values).max() > 1e-3                     # the link changed something

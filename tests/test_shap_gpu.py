"""k_tree_shap (csrc/shap_kernels.hip) against the fp64 recursion ``explain.tree_shap``, and the device path of
``predict_contributions`` against the ``H2O_SHAP_HIP=0`` host path.

TOL: ``max |gpu - cpu| / max(1, max |cpu|)`` measured over the kernel cases below on an MI355X was 4.441e-16 in
one run and 5.551e-16 in the next (profiles/shap_gpu.md); the bound is 16x the larger, for the order of the fp64
atomics and FMA contraction.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from h2o.estimators import H2OGradientBoostingEstimator, H2ORandomForestEstimator, H2OXGBoostEstimator
from llama_github_io_amd import explain
from llama_github_io_amd.ops import _native as nat, shap

import shap_cases as sc

pytestmark = pytest.mark.gpu

MEASURED = 5.551e-16
TOL = 16 * MEASURED
R = shap.ROW_TILE
ROWS = [1, R - 1, R, R + 1, 4 * R + 1]

# name -> (kinds, forest kwargs, G the forest must land on). 256 / G paths fill one round of a block, and with
# few rows a block walks one round, so every forest here spans several path chunks of the grid.
GPU_CASES = {
    "f1": ([0], dict(depth=3, ntrees=3), 8),
    "f3_k3": ([0, 5, 0], dict(depth=5, ntrees=6, K=3), 8),
    "f33_g8": sc.CASES["f33"] + (8,),
    "f33_g16": ([0] * 30 + [3, 33, 70], dict(depth=12, ntrees=40, spine=True), 16),
    "f33_g32": ([0] * 30 + [3, 33, 70], dict(depth=20, ntrees=10, spine=True), 32),
    "f33_g64": ([0] * 30 + [3, 33, 70], dict(depth=33, ntrees=4, spine=True), 64),
    "f33_k3_phi_global": ([0] * 30 + [3, 33, 70], dict(depth=6, ntrees=6, K=3), 8),     # K * (F+1) * R * 8 > PHI_TILE_BYTES
    "f70_x_global": ([0] * 66 + [3, 33, 70, 0], dict(depth=6, ntrees=4, skip=5), 8),     # F * R * 4 > X_TILE_BYTES
}


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=list(GPU_CASES))
def case(request):
    kinds, kw, G = GPU_CASES[request.param]
    forest = sc.random_forest(0, kinds, **kw)
    X = sc.random_rows(1, kinds, max(ROWS))
    ref = explain.tree_shap(forest, X)
    ref.setflags(write=False)
    return request.param, kinds, forest, X, ref, G


def test_budget_branches():
    tiles = np.zeros(3, np.int32)
    nat.call("h2o_shap_tiles", tiles.ctypes.data)       # the Python constants mirror the compiled ones
    assert tiles.tolist() == [shap.ROW_TILE, shap.X_TILE_BYTES, shap.PHI_TILE_BYTES]
    F33, F70 = 33, 70
    assert F33 * R * 4 <= shap.X_TILE_BYTES < F70 * R * 4
    assert R * 1 * (F33 + 1) * 8 <= shap.PHI_TILE_BYTES < R * 3 * (F33 + 1) * 8


@pytest.mark.parametrize("N", ROWS)
def test_kernel_matches_oracle(case, dev, N):
    name, kinds, forest, X, ref, G = case
    paths = shap.forest_paths(forest)
    assert paths.G == G and (paths.n_paths > 256 // G or name == "f1")
    got = explain.tree_shap_device(forest, X[:, :N].contiguous().to(dev))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (N,) + ref.shape[1:]
    err = rel_err(got.cpu().numpy(), ref[:N])
    print(f"shap_err {name} N={N} G={G} P={paths.n_paths} err={err:.3e} maxphi={np.abs(ref).max():.3f}")
    assert err <= TOL


def test_several_rounds_per_block(case, dev):
    name, kinds, forest, X, ref, G = case
    got = shap.path_shap(shap.forest_paths(forest), X.to(dev), forest.K, rounds=3)
    err = rel_err(got.cpu().numpy(), ref)
    print(f"shap_err {name} rounds=3 err={err:.3e}")
    assert err <= TOL


def test_unused_column_zero_and_guard_row(case, dev):
    name, kinds, forest, X, ref, G = case
    F, K = len(kinds), forest.K
    for N in (R - 1, R + 1):
        out = torch.zeros(N + 1, K, F + 1, dtype=torch.float64, device=dev)
        out[N] = 7.25
        res = shap.path_shap(shap.forest_paths(forest), X[:, :N].contiguous().to(dev), K, out=out)
        assert res is out
        assert bool((out[N] == 7.25).all())                                  # rows beyond N are untouched
        assert rel_err(out[:N].cpu().numpy(), ref[:N]) <= TOL
        skip = GPU_CASES[name][1].get("skip")
        if skip is not None:
            assert bool((out[:N, :, skip] == 0.0).all())


def test_back_to_back_calls_agree(case, dev):
    name, kinds, forest, X, ref, G = case
    Xd = X.to(dev)
    a = explain.tree_shap_device(forest, Xd).cpu().numpy()
    b = explain.tree_shap_device(forest, Xd).cpu().numpy()
    assert rel_err(a, b) <= TOL and rel_err(b, ref) <= TOL


# ---- end to end: the frame recipe of tests/test_explain.py

@pytest.fixture(scope="module")
def fr():
    h2o.init(verbose=False)
    rng = np.random.default_rng(0)
    n = 1500
    df = pd.DataFrame({"a": rng.normal(size=n), "b": rng.normal(size=n), "c": rng.choice(list("xyz"), n)})
    df.loc[::13, "b"] = np.nan
    df["y"] = np.where(df.a + (df.c == "x") + rng.normal(size=n) * 0.3 > 0, "1", "0")
    df["r"] = df.a * 2 + np.nan_to_num(df.b) * df.a
    return h2o.H2OFrame(df, column_types={"y": "enum"})


@pytest.mark.parametrize("E,y", [(H2OGradientBoostingEstimator, "y"), (H2OGradientBoostingEstimator, "r"),
                                 (H2OXGBoostEstimator, "y"), (H2ORandomForestEstimator, "r")])
def test_predict_contributions_on_device(fr, E, y, monkeypatch):
    m = E(ntrees=8, seed=1, max_depth=5)
    m.train(x=["a", "b", "c"], y=y, training_frame=fr)
    mm = m._model
    assert torch.device(mm.device).type == "cuda"
    monkeypatch.delenv("H2O_SHAP_HIP", raising=False)
    out = m.predict_contributions(fr)
    assert out.names == ["a", "b", "c", "BiasTerm"]
    for n in out.names:
        d = out._col(n).data
        assert d.is_cuda and d.dtype == torch.float64
    srt = m.predict_contributions(fr, top_n=2, bottom_n=1)
    monkeypatch.setenv("H2O_SHAP_HIP", "0")
    host = m.predict_contributions(fr)
    assert not host._col("a").data.is_cuda
    host_srt = m.predict_contributions(fr, top_n=2, bottom_n=1).as_data_frame()
    monkeypatch.delenv("H2O_SHAP_HIP")
    g, c = out.as_data_frame().values, host.as_data_frame().values
    err = rel_err(g, c)
    print(f"shap_err e2e {E.__name__} {y} err={err:.3e} maxphi={np.abs(c).max():.3f}")
    assert err <= TOL
    raw = mm.forest.predict_raw(fr.model_matrix(mm.info)[0])[:, 0].double().cpu().numpy()
    if mm.algo == "drf":
        raw = raw / mm.ntrees_built()
    else:
        raw = raw + (mm.init_f[0] if isinstance(mm.init_f, (list, tuple)) else mm.init_f)
    assert np.abs(g.sum(1) - raw).max() < 1e-5
    # the sorted frame equals the one computed from the host contributions. With F = 3, top_n + bottom_n >= F, so
    # it is the all-features frame. Rows where two contributions are closer than 1e-9 could legitimately swap
    # places: there only the values are compared.
    s = srt.as_data_frame()
    assert list(s.columns) == list(host_srt.columns) == [f"top_{w}_{i}" for i in (1, 2, 3) for w in ("feature", "value")] + ["BiasTerm"]
    vals = [n for n in s.columns if "feature" not in n]
    assert rel_err(s[vals].values, host_srt[vals].values) <= TOL
    assert (np.diff(s[["top_value_1", "top_value_2", "top_value_3"]].values, axis=1) <= 0).all()
    gap = np.diff(np.sort(c[:, :3], axis=1), axis=1).min(1)
    clear = gap > 1e-9
    assert clear.mean() > 0.5
    for n in ("top_feature_1", "top_feature_2", "top_feature_3"):
        assert (s[n].values[clear] == host_srt[n].values[clear]).all()


def test_top_bottom_on_device_matches_host(dev, monkeypatch):
    """top_n=2, bottom_n=1 with more features than that (the frame above has three, so there every feature comes
    back): a five-feature GBM, sorted on device and from the host contributions."""
    h2o.init(verbose=False)
    rng = np.random.default_rng(3)
    n = 400
    df = pd.DataFrame({c: rng.normal(size=n) for c in "abcde"})
    df["r"] = df.a * 2 - df.b + df.c * df.d + rng.normal(size=n) * 0.1
    fr5 = h2o.H2OFrame(df)
    m = H2OGradientBoostingEstimator(ntrees=6, seed=1, max_depth=4)
    m.train(x=list("abcde"), y="r", training_frame=fr5)
    monkeypatch.delenv("H2O_SHAP_HIP", raising=False)
    srt = m.predict_contributions(fr5, top_n=2, bottom_n=1)
    assert srt._col("top_value_1").data.is_cuda and srt._col("top_feature_1").data.is_cuda
    s = srt.as_data_frame()
    monkeypatch.setenv("H2O_SHAP_HIP", "0")
    host = m.predict_contributions(fr5).as_data_frame()
    host_srt = m.predict_contributions(fr5, top_n=2, bottom_n=1).as_data_frame()
    assert list(s.columns) == list(host_srt.columns) == ["top_feature_1", "top_value_1", "top_feature_2", "top_value_2",
                                                         "bottom_feature_1", "bottom_value_1", "BiasTerm"]
    vals = [n for n in s.columns if "feature" not in n]
    assert rel_err(s[vals].values, host_srt[vals].values) <= TOL
    phi = host[list("abcde")].values
    clear = np.diff(np.sort(phi, axis=1), axis=1).min(1) > 1e-9
    assert clear.mean() > 0.5
    for n in ("top_feature_1", "top_feature_2", "bottom_feature_1"):
        assert (s[n].values[clear] == host_srt[n].values[clear]).all()
    assert (s["top_feature_1"].values[clear] == np.asarray(list("abcde"))[phi.argmax(1)][clear]).all()
    assert (s["bottom_feature_1"].values[clear] == np.asarray(list("abcde"))[phi.argmin(1)][clear]).all()

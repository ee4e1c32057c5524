"""k_shap_baseline (csrc/shap_baseline_kernels.hip) against the fp64 PyTorch evaluation of the same path table
(``ops.shap.path_shap_baseline`` on CPU tensors, itself held to two oracles in test_shap_baseline_paths.py), and
the device path of ``predict_contributions(background_frame=...)`` against the ``H2O_SHAP_HIP=0`` host path.

TOL: ``max |gpu - cpu| / max(1, max |cpu|)`` measured over the kernel cases below on an MI355X was 7.829e-16
in one run and 7.755e-16 in the next (profiles/shap_baseline_gpu.md); the bound is 16x the larger, for the
order of the fp64 atomics and FMA contraction, as in test_shap_gpu.py.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import h2o
from h2o.estimators import H2OGradientBoostingEstimator, H2ORandomForestEstimator, H2OXGBoostEstimator
from llama_github_io_amd.ops import _native as nat, shap

import shap_cases as sc

pytestmark = pytest.mark.gpu

MEASURED = 7.829e-16
TOL = 16 * MEASURED
R, BT = shap.BASELINE_ROW_TILE, shap.BG_TILE
ROWS = [1, R - 1, R + 1]
BGS = [1, BT - 1, BT + 1, 2 * BT + 1]

# the forests of tests/test_shap_gpu.py: name -> (kinds, forest kwargs, G the forest must land on)
F33 = [0] * 30 + [3, 33, 70]
GPU_CASES = {
    "f1": ([0], dict(depth=3, ntrees=3), 8),
    "f3_k3": ([0, 5, 0], dict(depth=5, ntrees=6, K=3), 8),
    "f33_g8": sc.CASES["f33"] + (8,),
    "f33_g16": (F33, dict(depth=12, ntrees=40, spine=True), 16),
    "f33_g32": (F33, dict(depth=20, ntrees=10, spine=True), 32),
    "f33_g64": (F33, dict(depth=33, ntrees=4, spine=True), 64),
    "f33_k3_phi_global": (F33, dict(depth=6, ntrees=6, K=3), 8),        # K * (F+1) * R * 8 > BASELINE_PHI_TILE_BYTES
    "f70_x_global": ([0] * 66 + [3, 33, 70, 0], dict(depth=6, ntrees=4, skip=5), 8),   # F * (R+BT) * 4 > ..._X_TILE_BYTES
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
    X, Bg = sc.random_rows(1, kinds, max(ROWS)), sc.random_rows(2, kinds, max(BGS))
    paths = shap.forest_paths(forest)
    ref = shap.path_shap_baseline(paths, X, Bg, forest.K, per_reference=True)
    ref = ref.view(max(ROWS), max(BGS), forest.K, len(kinds) + 1).numpy()       # [N, B, K, F+1]
    ref.setflags(write=False)
    return request.param, kinds, forest, paths, X, Bg, ref, G


def test_budget_branches():
    tiles = np.zeros(4, np.int32)
    nat.call("h2o_shap_baseline_tiles", tiles.ctypes.data)      # the Python constants mirror the compiled ones
    assert tiles.tolist() == [shap.BASELINE_ROW_TILE, shap.BG_TILE, shap.BASELINE_X_TILE_BYTES,
                              shap.BASELINE_PHI_TILE_BYTES]
    F33n, F70 = 33, 70
    assert F33n * (R + BT) * 4 <= shap.BASELINE_X_TILE_BYTES < F70 * (R + BT) * 4
    assert R * 1 * (F33n + 1) * 8 <= shap.BASELINE_PHI_TILE_BYTES < R * 3 * (F33n + 1) * 8


@pytest.mark.parametrize("per_reference", [False, True])
def test_kernel_matches_table_evaluation(case, dev, per_reference):
    name, kinds, forest, paths, X, Bg, ref, G = case
    assert paths.G == G and (paths.n_paths > 256 // G or name == "f1")
    worst = 0.0
    for N in ROWS:
        for B in BGS:
            got = shap.path_shap_baseline(paths, X[:, :N].contiguous().to(dev), Bg[:, :B].contiguous().to(dev),
                                          forest.K, per_reference=per_reference)
            assert got.is_cuda and got.dtype == torch.float64
            want = ref[:N, :B].reshape((N * B,) + ref.shape[2:]) if per_reference else ref[:N, :B].sum(1)
            assert tuple(got.shape) == want.shape
            err = rel_err(got.cpu().numpy(), want)
            print(f"sbase_err {name} per_ref={int(per_reference)} N={N} B={B} G={G} P={paths.n_paths} err={err:.3e} "
                  f"maxphi={np.abs(want).max():.3f}")
            worst = max(worst, err)
    assert worst <= TOL


@pytest.mark.parametrize("per_reference", [False, True])
def test_several_rounds_per_block(case, dev, per_reference):
    name, kinds, forest, paths, X, Bg, ref, G = case
    got = shap.path_shap_baseline(paths, X.to(dev), Bg.to(dev), forest.K, per_reference=per_reference, rounds=3)
    want = ref.reshape((-1,) + ref.shape[2:]) if per_reference else ref.sum(1)
    err = rel_err(got.cpu().numpy(), want)
    print(f"sbase_err {name} per_ref={int(per_reference)} rounds=3 err={err:.3e}")
    assert err <= TOL


def test_unused_column_zero_and_guard_row(case, dev):
    name, kinds, forest, paths, X, Bg, ref, G = case
    F, K = len(kinds), forest.K
    N, B = R + 1, BT + 1
    Xd, Bd = X[:, :N].contiguous().to(dev), Bg[:, :B].contiguous().to(dev)
    for per_reference, rows, want in ((False, N, ref[:N, :B].sum(1)), (True, N * B, ref[:N, :B].reshape(N * B, K, F + 1))):
        out = torch.zeros(rows + 1, K, F + 1, dtype=torch.float64, device=dev)
        out[rows] = 7.25
        res = shap.path_shap_baseline(paths, Xd, Bd, K, per_reference=per_reference, out=out)
        assert res is out
        assert bool((out[rows] == 7.25).all())                               # rows beyond the output are untouched
        assert rel_err(out[:rows].cpu().numpy(), want) <= TOL
        skip = GPU_CASES[name][1].get("skip")
        if skip is not None:
            assert bool((out[:rows, :, skip] == 0.0).all())


def test_back_to_back_calls_agree(case, dev):
    name, kinds, forest, paths, X, Bg, ref, G = case
    Xd, Bd = X.to(dev), Bg.to(dev)
    a = shap.path_shap_baseline(paths, Xd, Bd, forest.K).cpu().numpy()
    b = shap.path_shap_baseline(paths, Xd, Bd, forest.K).cpu().numpy()
    assert rel_err(a, b) <= TOL and rel_err(b, ref.sum(1)) <= TOL


def test_over_length_forest_takes_the_host_evaluation(dev, monkeypatch):
    kinds, kw, G = GPU_CASES["f33_g8"]
    forest = sc.random_forest(0, kinds, **kw)
    X, Bg = sc.random_rows(1, kinds, 5), sc.random_rows(2, kinds, 3)
    paths = shap.forest_paths(forest)
    ref = shap.path_shap_baseline(paths, X, Bg, forest.K)
    monkeypatch.setattr(shap, "MAX_PATH_LEN", 4)
    got = shap.path_shap_baseline(paths, X.to(dev), Bg.to(dev), forest.K)
    assert got.is_cuda and torch.equal(got.cpu(), ref)


# ---- end to end: the frame recipe of tests/test_shap_gpu.py, 37 background rows

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


def values(frame, names):
    return torch.stack([frame._col(n).data.double().cpu() for n in names], 1).numpy()


@pytest.mark.parametrize("E,y", [(H2OGradientBoostingEstimator, "y"), (H2OGradientBoostingEstimator, "r"),
                                 (H2OXGBoostEstimator, "y"), (H2ORandomForestEstimator, "r")])
def test_predict_contributions_with_background_on_device(fr, E, y, monkeypatch):
    m = E(ntrees=8, seed=1, max_depth=5)
    m.train(x=["a", "b", "c"], y=y, training_frame=fr)
    mm = m._model
    assert torch.device(mm.device).type == "cuda"
    bg = fr[700:737, :]
    N, B = fr.nrows, bg.nrows
    assert B == 37
    cells = ["a", "b", "c", "BiasTerm"]
    monkeypatch.delenv("H2O_SHAP_HIP", raising=False)
    per = m.predict_contributions(fr, background_frame=bg, output_per_reference=True)
    avg = m.predict_contributions(fr, background_frame=bg)
    assert per.names == cells + ["RowIdx", "BackgroundRowIdx"] and per.nrows == N * B
    assert avg.names == cells and avg.nrows == N
    for out in (per, avg):
        for n in cells:
            d = out._col(n).data
            assert d.is_cuda and d.dtype == torch.float64
    monkeypatch.setenv("H2O_SHAP_HIP", "0")
    host = m.predict_contributions(fr, background_frame=bg, output_per_reference=True)
    assert not host._col("a").data.is_cuda
    monkeypatch.delenv("H2O_SHAP_HIP")
    g, c = values(per, cells), values(host, cells)
    err = rel_err(g, c)
    print(f"sbase_err e2e {E.__name__} {y} err={err:.3e} maxphi={np.abs(c).max():.3f}")
    assert err <= TOL
    assert np.array_equal(values(per, ["RowIdx", "BackgroundRowIdx"]),
                          np.stack([np.repeat(np.arange(N), B), np.tile(np.arange(B), N)], 1))
    # the averaged frame is the mean of the per-reference rows of each row
    assert rel_err(values(avg, cells), g.reshape(N, B, 4).mean(1)) <= TOL
    # per pair: the features sum to f(x) - f(b), the bias is f(b)
    raw = mm.forest.predict_raw(fr.model_matrix(mm.info)[0])[:, 0].double().cpu().numpy()
    if mm.algo == "drf":
        raw = raw / mm.ntrees_built()
    else:
        raw = raw + (mm.init_f[0] if isinstance(mm.init_f, (list, tuple)) else mm.init_f)
    assert np.abs(g.sum(1) - np.repeat(raw, B)).max() < 1e-5
    assert np.abs(g[:, 3] - np.tile(raw[700:737], N)).max() < 1e-5
    # output space: rows sum to the prediction (p1 of a binomial GBM / XGBoost), per pair and averaged
    pred = m.predict(fr)
    p = values(pred, [pred.names[-1]])[:, 0] if y == "y" else values(pred, ["predict"])[:, 0]
    osp = values(m.predict_contributions(fr, background_frame=bg, output_space=True), cells)
    assert np.abs(osp.sum(1) - p).max() < 1e-5
    osp_per = values(m.predict_contributions(fr, background_frame=bg, output_space=True, output_per_reference=True), cells)
    assert np.abs(osp_per.sum(1) - np.repeat(p, B)).max() < 1e-5
    # (the two are not compared at TOL: the scale of a pair is (linkinv(fx) - linkinv(fb)) / d, a cancelling
    # difference whose rounding is relative to 1 / |d|, and two device calls round d differently)
    if y == "y":
        assert np.abs(osp - values(avg, cells)).max() > 1e-3            # the link changed something
    else:
        assert np.array_equal(osp_per, g) or rel_err(osp_per, g) <= TOL  # no link: the margin-space values

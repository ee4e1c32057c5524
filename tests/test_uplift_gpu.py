"""The Uplift DRF kernels (csrc/uplift_kernels.hip) against the NumPy references of uplift_cases.py, exactly: both
histogram variants on every window they accept, the node totals and the routing pass; and the forests of the HIP
level loop against those of the PyTorch loop under ``H2O_UPLIFT_HIP=0`` on the same device, bit for bit."""
import numpy as np
import pytest
import torch

from llama_github_io_amd.ops import _native as nat
from llama_github_io_amd.ops import uplift as up

import uplift_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def variants(W):
    return ("lds", "direct") if W <= up.LDS_MAX_WINDOW else ("direct",)


@pytest.mark.parametrize("F", uc.HIST_FEATURES)
@pytest.mark.parametrize("N", uc.HIST_ROWS)
def test_histogram_equals_add_at(N, F, dev):
    bins, node, treat, y = uc.hist_inputs(N, F)
    assert bins.shape[1] > F and (N < 1000 or (bins[:, :F] == uc.NA_BIN).any(0).all())
    ref = uc.hist_reference(bins, node, treat, y, F, uc.HIST_LEVEL)
    d = [torch.from_numpy(a).to(dev) for a in (bins, node, treat, y)]
    for n0, W in uc.HIST_WINDOWS:
        assert n0 > 0 and n0 + W <= uc.HIST_LEVEL
        want = torch.from_numpy(ref[n0:n0 + W])
        if N >= 1000:       # rows on both sides of the window and outside the level
            assert (node < n0).any() and (node >= n0 + W).any() and (node == -1).any()
        for v in variants(W):
            got = up.level_hist(*d, n0, W, F, variant=v)
            assert got.dtype == torch.int64 and got.shape == (W, F, 256, 4)
            assert torch.equal(got.cpu(), want), (N, F, n0, W, v)
        assert torch.equal(up.level_hist(*d, n0, W, F).cpu(), want)            # the host's own choice
    with pytest.raises(ValueError):
        up.level_hist(*d, 0, up.LDS_MAX_WINDOW + 1, F, variant="lds")


@pytest.mark.parametrize("ones", [1, 0])
def test_one_cell_takes_every_row_of_a_tile(ones, dev):
    """The worst case of a packed cell: a constant column, every row in the same node and arm with y = 1, more rows
    than a block's tile. A 16-bit count or sum that overflowed would show here."""
    N, F, n0 = 70001, 3, 5
    bins = np.full((N, F + 1), 7, np.uint8)
    node = np.full(N, n0, np.int32)
    treat = np.full(N, ones, np.uint8)
    y = np.ones(N, np.uint8)
    ref = uc.hist_reference(bins, node, treat, y, F, n0 + 1)[n0:]
    assert ref[0, 0, 7].tolist() == ([N, N, 0, 0] if ones else [0, 0, N, N]) and ref.sum() == 2 * N * F
    d = [torch.from_numpy(a).to(dev) for a in (bins, node, treat, y)]
    for v in ("lds", "direct"):
        assert torch.equal(up.level_hist(*d, n0, 1, F, variant=v).cpu(), torch.from_numpy(ref)), v


@pytest.mark.parametrize("N", uc.HIST_ROWS)
def test_node_totals_equal_the_histogram_summed_over_bins(N, dev):
    bins, node, treat, y = uc.hist_inputs(N, 3)
    ref = uc.hist_reference(bins, node, treat, y, 1, uc.HIST_LEVEL)[:, 0].sum(1)
    got = up.node_totals(*(torch.from_numpy(a).to(dev) for a in (node, treat, y)), uc.HIST_LEVEL)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(ref))
    # fewer slots than the level: the rows of the slots past them are left out, not written out of bounds
    got = up.node_totals(*(torch.from_numpy(a).to(dev) for a in (node, treat, y)), 11)
    assert torch.equal(got.cpu(), torch.from_numpy(ref[:11]))


@pytest.mark.parametrize("N", uc.ROUTE_ROWS)
def test_route_equals_the_row_loop(N, dev):
    bins, node, feat, tb, child = uc.route_inputs(N)
    ref = uc.route_reference(bins, node, feat, tb, child)
    if N >= 1000:           # leaves, rows outside the level, NA bins going right, both children
        na = (node >= 0) & (child[node] >= 0) & (bins[np.arange(N), feat[node]] == uc.NA_BIN)
        assert (child < 0).any() and (node == -1).any() and na.any() and (ref[na] % 2 == 1).all()
        assert (ref[ref >= 0] % 2 == 0).any() and ((ref == -1) & (node >= 0)).any()
    got = up.route(*(torch.from_numpy(a).to(dev) for a in (bins, node, feat, tb, child)), 5)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(ref))


def test_cpu_tensors_never_reach_the_kernels(monkeypatch, dev):
    def no_call(*a):
        raise AssertionError("a kernel was launched on CPU tensors")
    monkeypatch.setattr(nat, "call", no_call)
    bins, node, treat, y = (torch.from_numpy(a) for a in uc.hist_inputs(64, 3))
    for v in (None, "lds", "direct"):
        with pytest.raises(ValueError, match="CUDA"):
            up.level_hist(bins, node, treat, y, 0, 2, 3, variant=v)
    with pytest.raises(ValueError, match="CUDA"):
        up.level_hist(bins.to(dev), node, treat.to(dev), y.to(dev), 0, 2, 3)        # one CPU tensor is enough
    with pytest.raises(ValueError, match="CUDA"):
        up.node_totals(node, treat, y, 4)
    rb, rn, feat, tb, child = (torch.from_numpy(a) for a in uc.route_inputs(65))
    with pytest.raises(ValueError, match="CUDA"):
        up.route(rb, rn, feat, tb, child, 5)


# ---- the forest of the HIP level loop is the forest of the PyTorch loop
def _level_widths(tree):
    depth = np.zeros(len(tree.left), np.int64)
    for i in range(len(tree.left)):                 # children follow their parent in the node order
        if tree.left[i] >= 0:
            depth[tree.left[i]] = depth[tree.right[i]] = depth[i] + 1
    return np.bincount(depth)


def _train(fr, n_num, params, hip, monkeypatch):
    from llama_github_io_amd.models import builder
    calls = dict(hist=0, route=0)
    hist, route = up.level_hist, up.route

    def spy_hist(*a, **k):
        calls["hist"] += 1
        return hist(*a, **k)

    def spy_route(*a, **k):
        calls["route"] += 1
        return route(*a, **k)
    with monkeypatch.context() as mp:
        mp.setenv("H2O_UPLIFT_HIP", "1" if hip else "0")
        mp.setattr(up, "level_hist", spy_hist)
        mp.setattr(up, "route", spy_route)
        m = builder.train("upliftdrf", dict(treatment_column="trt", auuc_nbins=100, **params), x=uc.predictors(n_num),
                          y="y", training_frame=fr)
    assert m.device.type == "cuda"
    assert (calls["hist"] > 0 and calls["route"] > 0) if hip else calls == dict(hist=0, route=0)
    return m


def _assert_same_forest(a, b, fr):
    for fa, fb in ((a.f_t, b.f_t), (a.f_c, b.f_c)):
        assert len(fa.trees) == len(fb.trees)
        for ta, tb in zip(fa.trees, fb.trees):
            for k in ("feat", "left", "right"):
                assert np.array_equal(getattr(ta, k), getattr(tb, k)), k
            for k in ("thr", "value"):              # bit for bit, NaN-free by construction
                assert np.array_equal(getattr(ta, k).view(np.int32), getattr(tb, k).view(np.int32)), k
    pa, pb = (m.predict(fr).as_data_frame().to_numpy() for m in (a, b))
    assert np.array_equal(pa, pb)
    ma, mb = a.output["training_metrics"], b.output["training_metrics"]
    for k in ("AUUC", "qini", "lift", "gain", "auuc_normalized", "aecu", "ate", "att", "atc"):
        assert ma[k] == mb[k], k


@pytest.mark.parametrize("metric", ["kl", "euclidean", "chi_squared"])
def test_forest_equals_the_pytorch_forest(metric, monkeypatch):
    """mtries below F, sample_rate 0.632, NaNs in a numeric column and one categorical column."""
    n_num = 4
    fr = uc.frame(4000, n_num)
    params = dict(ntrees=3, max_depth=7, min_rows=10, mtries=2, sample_rate=0.632, seed=11, uplift_metric=metric)
    ref = _train(fr, n_num, params, False, monkeypatch)
    assert sum(len(t.feat) for t in ref.f_t.trees) > 3 * 15 and np.isnan(uc.frame_data(4000, n_num)["x1"]).any()
    _assert_same_forest(_train(fr, n_num, params, True, monkeypatch), ref, fr)


def test_deep_forest_crosses_the_lds_window_and_the_search_window(monkeypatch):
    """12000 rows, 32 predictors and min_rows = 2: the smallest of the frames tried whose reference tree has a
    searched level (one above the last) wider than the LDS variant's window and than one search window."""
    n_num, depth = 31, 10
    fr = uc.frame(12000, n_num)
    params = dict(ntrees=1, max_depth=depth, min_rows=2, mtries=8, sample_rate=0.632, seed=2, uplift_metric="euclidean")
    ref = _train(fr, n_num, params, False, monkeypatch)
    widths = _level_widths(ref.f_t.trees[0])
    assert len(widths) == depth + 1
    assert widths[:depth].max() > max(up.LDS_MAX_WINDOW, up.search_window(n_num + 1)), widths
    assert (widths[:depth] <= up.LDS_MAX_WINDOW).any() and up.search_window(n_num + 1) > up.LDS_MAX_WINDOW
    _assert_same_forest(_train(fr, n_num, params, True, monkeypatch), ref, fr)

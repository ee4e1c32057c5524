"""k_predict (csrc/predict_kernels.hip) against the PyTorch traversal ``Forest._predict_torch`` of the same flat
forest. test_pdp_gpu.py compares the grid kernel with ``k_predict``, but both call ``forest_go_left``
(csrc/forest_view.h), so an error in it would show in neither; the CPU traversal is written independently.

The checks are bitwise (``torch.equal``) on margins and leaf indices: both sides add the same fp32 leaf values in
forest order per class. The rows of shap_cases.py carry NaN, +-inf on numeric features and the categorical codes
-1, n and n + 1; the row counts sit around the launcher's 256-thread block."""
import pytest
import torch

import pdp_cases as pc

pytestmark = pytest.mark.gpu

ROWS = [1, 255, 256, 257]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_cache = {}


def case(name):
    """(forest, rows [F, 257] on the host), built once per module."""
    if name not in _cache:
        kinds, forest = pc.make_case(name)
        _cache[name] = (forest, pc.sc.random_rows(1, kinds, max(ROWS)))
    return _cache[name]


@pytest.mark.parametrize("name", list(pc.CASES))
def test_margins_and_leaves_equal_the_host_traversal(name, dev):
    forest, X = case(name)
    for N in ROWS:
        Xn = X[:, :N].contiguous()
        ref, ref_leaves = forest.predict_raw(Xn, return_leaves=True)
        got, leaves = forest.predict_raw(Xn.to(dev), return_leaves=True)
        assert got.is_cuda and leaves.is_cuda and leaves.dtype == torch.int32
        assert torch.equal(got.cpu(), ref), f"{name} N={N}"
        assert torch.equal(leaves.cpu(), ref_leaves), f"{name} N={N}"


@pytest.mark.parametrize("t0,t1", [(1, 5), (2, 3)])
def test_tree_ranges(t0, t1, dev):
    forest, X = case("k3")
    ref, ref_leaves = forest.predict_raw(X, t0, t1, return_leaves=True)
    got, leaves = forest.predict_raw(X.to(dev), t0, t1, return_leaves=True)
    assert tuple(leaves.shape) == (X.shape[1], t1 - t0)
    assert torch.equal(got.cpu(), ref) and torch.equal(leaves.cpu(), ref_leaves)


def test_out_is_accumulated_into(dev):
    forest, X = case("k3")
    N = X.shape[1]
    fill = torch.arange(N * forest.K, dtype=torch.float32).view(N, forest.K) * 0.125 - 3.0
    ref = forest.predict_raw(X, out=fill.clone())
    out = fill.to(dev)
    got = forest.predict_raw(X.to(dev), out=out)
    assert got is out
    assert torch.equal(got.cpu(), ref)
    assert not torch.equal(ref, forest.predict_raw(X))          # the fill changed something

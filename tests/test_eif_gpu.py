"""k_eif_path (csrc/eif_kernels.hip) against the ordered fp64 walk of eif_cases.py, bit for bit, on both row paths
(staged in LDS, read from X) and in both non-finite modes; the device scoring of the native model and of its MOJO
import against the PyTorch scoring under ``H2O_EIF_HIP=0``; and the peak memory of a call."""
import numpy as np
import pytest
import torch

from llama_github_io_amd.models.generic import GenericModel
from llama_github_io_amd.mojo.writer import write_mojo
from llama_github_io_amd.ops import _native as nat
from llama_github_io_amd.ops import eif as E

import eif_cases as ec

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("case", ec.ALL_CASES, ids=ec.case_id)
modes = pytest.mark.parametrize("mode", ["native", "mojo"])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


_packed = {}


def packed(case, mode):
    key = (ec.case_id(case), mode)
    if key not in _packed:
        trees = ec.reference(case, mode)[4]
        _packed[key] = E.pack(trees, keep_zeros=mode == "mojo")
    return _packed[key]


def check_kernel(case, mode, finite, dev, staged=None):
    """The kernel's sums equal the reference's on every row count; returns them per row count. ``staged``: sums of
    another row path that these must equal too."""
    X, sums, margin, leaves, trees = ec.reference(case, mode, finite)
    pk = packed(case, mode)
    Xd = X.to(dev)
    out = {}
    for n in ec.ROWS:
        got = E.path_length_sums(Xd[:, :n].contiguous(), pk, nan_to_zero=mode == "native")
        assert got.dtype == torch.float64 and got.shape == (n,)
        assert torch.equal(got.cpu(), torch.from_numpy(sums[:n])), (ec.case_id(case), mode, n)
        if staged is not None:
            assert torch.equal(got, staged[n])
        out[n] = got
    return out


@modes
@cases
def test_kernel_equals_the_ordered_walk(case, mode, dev):
    check_kernel(case, mode, True, dev)
    check_kernel(case, mode, False, dev)


@cases
def test_poisoned_row_ends_in_the_right_subtree(case, dev):
    """MOJO mode: a NaN in a feature whose normal component is zero at the root still sends the row right there
    (and on, at every node below). Dropping the zero components would not."""
    f = ec.root_zero_feature(ec.model_of(case))
    if f is None:
        return                                              # a fully extended root has no such feature
    X, sums, margin, leaves, trees = ec.reference(case, "mojo", finite=False)
    one = E.pack(trees[:1], keep_zeros=True)
    n = 0
    while one["left"][n] >= 0:
        n = int(one["right"][n])
    got = E.path_length_sums(X[:, :1].to(dev), one, nan_to_zero=False)
    assert float(got[0]) == float(one["value"][n])
    finite = ec.walk_reference(ec.rows_of(case)[:, :1], trees[:1], False, True, details=True)[2]
    assert finite[0, 0] != n                                # the NaN, not the row's other values, sent it there


@modes
@cases
def test_row_paths_agree(case, mode, dev, monkeypatch):
    """A byte cap of 0 and one byte short of the block's rows: the kernel reads X itself."""
    F = packed(case, mode)["n_features"]
    assert F * 256 * 4 <= E.EIF_ROW_LDS_BYTES               # the default stages these cases
    staged = check_kernel(case, mode, False, dev)
    for cap in (0, F * 256 * 4 - 1):
        monkeypatch.setattr(E, "EIF_ROW_LDS_BYTES", cap)
        check_kernel(case, mode, False, dev, staged)
        check_kernel(case, mode, True, dev)
    monkeypatch.setattr(E, "EIF_ROW_LDS_BYTES", F * 256 * 4)
    check_kernel(case, mode, False, dev, staged)


def check_excused(new, old, margin, case):
    """Bit equality, but for rows within 2^-40 of a hyperplane; test_eif_paths.py shows there is none."""
    differ = (new != old).any(1).cpu().numpy()
    if case == "dyadic":
        near = np.zeros_like(differ)                        # exact arithmetic: nothing to excuse, on a hyperplane or off
    else:
        near = margin <= ec.MARGIN
    assert not (differ & ~near).any(), int((differ & ~near).sum())
    assert int(near.sum()) == 0


@cases
def test_model_scoring_equals_the_torch_scoring_on_device(case, dev, monkeypatch, tmp_path):
    model = ec.model_of(case)
    X, sums, margin, leaves, trees = ec.reference(case, "native")
    Xd = X.to(dev)
    calls = []
    inner = nat.call
    monkeypatch.setattr(nat, "call", lambda name, *a: calls.append(name) or inner(name, *a))
    new = model._predict_tensor(Xd)
    assert calls == ["h2o_eif_path"] and new.shape == (X.shape[1], 2) and new.dtype == torch.float32
    assert torch.equal(new[:, 1].cpu(), (torch.from_numpy(sums) / len(trees)).float())
    generic = GenericModel.from_mojo(write_mojo(model, str(tmp_path / "eif.zip")))
    gnew = generic._predict_tensor(Xd)
    assert calls == ["h2o_eif_path"] * 2
    monkeypatch.setenv("H2O_EIF_HIP", "0")
    old, gold = model._predict_tensor(Xd), generic._predict_tensor(Xd)
    assert calls == ["h2o_eif_path"] * 2, "H2O_EIF_HIP=0 ran the kernel"
    check_excused(new, old, margin, case)
    check_excused(gnew, gold, ec.reference(case, "mojo")[2], case)
    assert torch.equal(old[:, 1].cpu(), model._predict_tensor(X)[:, 1])     # the device GEMMs decide as the host's


def test_no_rows_by_nodes_temporary(dev):
    case = (5, 4, 256, 9)
    pk = E.pack(ec.model_of(case).trees, keep_zeros=False)
    N = 65536
    X = torch.randn(5, N, generator=torch.Generator().manual_seed(7)).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = E.path_length_sums(X, pk, nan_to_zero=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak bytes", peak, "bound", 32 * N + E.packed_nbytes(pk))
    assert peak <= 32 * N + E.packed_nbytes(pk)
    ref = ec.walk_reference(X[:, :4096].cpu(), ec.model_of(case).trees, True, False)
    assert torch.equal(out[:4096].cpu(), torch.from_numpy(ref))

"""The packed Extended Isolation Forest (``ops/eif.py``) on the host: ``pack`` of both tree formats, the ordered fp64
walk of eif_cases.py against the PyTorch scoring, and which inputs take which path of ``path_length_sums``."""
import numpy as np
import pytest
import torch

from llama_github_io_amd.mojo import algos as A
from llama_github_io_amd.ops import _native as nat
from llama_github_io_amd.ops import eif as E

import eif_cases as ec

cases = pytest.mark.parametrize("case", ec.ALL_CASES, ids=ec.case_id)


@cases
def test_pack_round_trip_of_the_trainer_format(case):
    trees = ec.model_of(case).trees
    pk = E.pack(trees, keep_zeros=False)
    F = np.asarray(trees[0]["normal"]).shape[1]
    assert pk["n_trees"] == len(trees) and pk["n_features"] == F
    assert pk["n_nodes"] == sum(len(t["left"]) for t in trees) and len(pk["nz_begin"]) == pk["n_nodes"] + 1
    for name in E.EIF_ARRAYS:
        assert pk[name].dtype == E._DTYPES[name], name
    base = 0
    for t, tr in enumerate(trees):
        M = len(tr["left"])
        assert pk["roots"][t] == base
        split = np.asarray(tr["left"]) >= 0
        for side in ("left", "right"):
            assert np.array_equal(pk[side][base:base + M], np.where(split, np.asarray(tr[side]) + base, -1))
        assert np.array_equal(pk["off"][base:base + M][split], np.asarray(tr["offset"])[split])
        assert np.array_equal(pk["value"][base:base + M][~split], np.asarray(tr["value"])[~split])
        for i in range(M):
            k0, k1 = pk["nz_begin"][base + i], pk["nz_begin"][base + i + 1]
            nv = np.asarray(tr["normal"])[i]
            want = np.nonzero(nv)[0] if split[i] else np.zeros(0, np.int64)
            assert np.array_equal(pk["nz_feat"][k0:k1], want)          # ascending, zeros dropped, none for a leaf
            assert np.array_equal(pk["nz_val"][k0:k1], nv[want])
        base += M


@cases
def test_pack_of_the_mojo_format_keeps_zeros(case):
    model = ec.model_of(case)
    mt = ec.mojo_trees(model)
    pk = E.pack(mt, keep_zeros=True)
    F = pk["n_features"]
    base = 0
    for tr, orig in zip(mt, model.trees):
        M = len(tr["left"])
        split = tr["left"].numpy() >= 0
        assert np.array_equal(np.diff(pk["nz_begin"])[base:base + M], np.where(split, F, 0))
        nodes = np.nonzero(split)[0]
        k0 = pk["nz_begin"][base + nodes[0]]
        assert np.array_equal(pk["nz_feat"][k0:k0 + F], np.arange(F))
        assert np.array_equal(pk["nz_val"][k0:k0 + F], tr["normal"][nodes[0]].numpy())
        assert np.array_equal(pk["off"][base:base + M][split], (tr["normal"] * tr["point"]).sum(1).numpy()[split])
        # the leaves hold depth + c(rows): the same multiset of path lengths as the trainer's tree
        assert np.array_equal(np.sort(pk["value"][base:base + M][~split]),
                              np.sort(np.asarray(orig["value"])[np.asarray(orig["left"]) < 0]))
        for side in ("left", "right"):
            assert np.array_equal(pk[side][base:base + M], np.where(split, tr[side].numpy() + base, -1))
        base += M
    assert E.pack(model.trees, keep_zeros=True)["nz_begin"][-1] == F * int((pk["left"] >= 0).sum())


@cases
def test_walk_reference_equals_the_torch_scoring(case):
    """The ordered walk and the GEMM projection make the same decisions: no row of these inputs lies within 2^-40
    (relative) of a hyperplane it meets, so bit equality is a sound demand; the dyadic forest's arithmetic is exact
    in any order, rows on a hyperplane included."""
    model = ec.model_of(case)
    for mode in ("native", "mojo"):
        X, sums, margin, leaves, trees = ec.reference(case, mode)
        T = len(trees)
        if mode == "native":
            old = ec.old_path_lengths(trees, X)
            assert torch.equal(model._path_lengths(X), old)
            assert torch.equal(model._predict_tensor(X)[:, 1], old.float())
        else:
            old = ec.old_score_eif_mean(trees, X)
            st = dict(trees=trees, sample_size=model.output["sample_size"])
            assert torch.equal(A.score_eif(st, X)[:, 1], old.float())
            assert torch.equal(E.path_length_sums(X, st["_packed"], nan_to_zero=False) / T, old)
        assert torch.equal(torch.from_numpy(sums) / T, old)
        if case == "dyadic":            # rows on a hyperplane, decided alike: proj == 0 goes left
            assert mode == "mojo" or int((margin == 0).sum()) >= 48
        else:
            print(ec.case_id(case), mode, "smallest relative margin", float(margin.min()))
            assert float(margin.min()) > ec.MARGIN


def test_dyadic_rows_on_a_hyperplane_go_left():
    X, sums, margin, leaves, trees = ec.reference("dyadic", "native")
    for r in range(48):
        assert leaves[r % 3, r] in range(7, 11)             # the root's left subtree


@cases
def test_path_length_sums_on_cpu_is_the_old_scoring(case):
    model = ec.model_of(case)
    X = ec.with_non_finite(ec.rows_of(case))
    T = len(model.trees)
    pk = E.pack(model.trees, keep_zeros=False)
    old = ec.old_path_lengths(model.trees, X)              # the mean: the sum over the trees / T
    assert torch.equal(E.path_length_sums(X, pk, nan_to_zero=True) / T, old)
    assert torch.equal(E.path_length_sums(X.double(), pk, nan_to_zero=True) / T, old)
    mt = ec.mojo_trees(model)
    got = E.path_length_sums(X, E.pack(mt, keep_zeros=True), nan_to_zero=False)
    assert torch.equal(got / T, ec.old_score_eif_mean(mt, X))


def test_non_finite_cells_in_mojo_mode_send_the_row_right():
    """A NaN in a feature outside the root's hyperplane poisons the projection (every feature is listed)."""
    for case in ec.ALL_CASES:
        model = ec.model_of(case)
        f = ec.root_zero_feature(model)
        if f is None:
            continue
        X, sums, margin, leaves, trees = ec.reference(case, "mojo", finite=False)
        for t, tr in enumerate(trees):                      # all the way right in every tree
            n = 0
            while tr["left"][n] >= 0:
                n = int(tr["right"][n])
            assert leaves[t, 0] == n
        assert torch.equal(ec.old_score_eif_mean(trees, X)[:1], torch.from_numpy(sums[:1]) / len(trees))


def test_cpu_tensors_and_the_switch_take_the_torch_path(monkeypatch):
    calls = []
    monkeypatch.setattr(nat, "call", lambda name, *a: calls.append(name))
    model = ec.model_of("dyadic")
    X = ec.rows_of("dyadic", 65)
    model._predict_tensor(X)
    E.path_length_sums(X.double(), model._packed_forest(), nan_to_zero=True)
    assert calls == []
    assert E.hip_enabled()
    monkeypatch.setenv("H2O_EIF_HIP", "0")
    assert not E.hip_enabled()


def test_validation_and_empty_shapes():
    model = ec.model_of("dyadic")
    pk = model._packed_forest()
    assert pk is model._packed_forest()                     # packed once
    with pytest.raises(ValueError):
        E.path_length_sums(torch.zeros(3, 5), pk, nan_to_zero=True)
    assert E.path_length_sums(torch.zeros(4, 0), pk, nan_to_zero=True).shape == (0,)
    empty = E.pack([], keep_zeros=False)
    out = E.path_length_sums(torch.zeros(4, 5), empty, nan_to_zero=True)
    assert out.dtype == torch.float64 and not bool(out.any())
    assert E.packed_nbytes(pk) == sum(pk[k].nbytes for k in E.EIF_ARRAYS)

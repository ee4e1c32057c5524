"""``Forest.predict_stages`` on CPU tensors (staged margins and leaves against ``Forest.predict_raw``, feature
frequencies against a climb of the parent table), and ``predict_leaf_node_assignment`` / ``staged_predict_proba`` /
``feature_frequencies`` of the h2o facade on models, hand-built forests and a frame sharded over two gloo ranks."""
import json
import os
import socket
import sys

import numpy as np
import pandas as pd
import pytest
import torch
import torch.multiprocessing as mp

import h2o
from llama_github_io_amd.models.base import DataInfo
from llama_github_io_amd.models.shared_tree import SharedTreeModel
from llama_github_io_amd.ops import forest as fo

import forest_stages_cases as fs
import pdp_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def case(name):
    if name not in _cache:
        kinds, forest = pc.make_case(name)
        _cache[name] = (kinds, forest, pc.sc.random_rows(1, kinds, max(fs.ROWS)))
    return _cache[name]


@pytest.mark.parametrize("name", fs.ALL_CASES)
def test_stage_and_leaves_equal_predict_raw(name):
    kinds, forest, X = case(name)
    for n in fs.ROWS:
        fs.check_stages(forest, X[:, :n].contiguous())


@pytest.mark.parametrize("name", ["k3", "f2_depth8"])
def test_tree_sub_range(name):
    kinds, forest, X = case(name)
    T = len(forest.trees)
    for t0, t1 in [(1, T - 1), (2, 3), (1, T)]:
        fs.check_stages(forest, X[:, :65].contiguous(), t0, t1)


@pytest.mark.parametrize("name", fs.ALL_CASES)
def test_freq_equals_parent_climb(name):
    kinds, forest, X = case(name)
    skip = pc.CASES[name][1].get("skip")
    for n in fs.ROWS:
        fs.check_freq(forest, X[:, :n].contiguous(), skip)


@pytest.mark.parametrize("name", ["k3", "cats", "single_leaf"])
def test_output_subsets_and_out(name):
    kinds, forest, X = case(name)
    fs.check_subsets(forest, X[:, :65].contiguous())


def test_validation_and_empty_shapes():
    kinds, forest, X = case("k3")
    X = X[:, :5].contiguous()
    with pytest.raises(ValueError):
        forest.predict_stages(X[:2].contiguous())                # the forest splits on feature 2
    with pytest.raises(ValueError):
        forest.predict_stages(X, stage=False)
    with pytest.raises(ValueError):
        forest.predict_stages(X, out=torch.empty(6 * 5 - 1))
    with pytest.raises(ValueError):
        forest.predict_stages(X, out=torch.empty(6 * 5, dtype=torch.float64))
    st, lv, fq = forest.predict_stages(X[:, :0], leaves=True, freq=True)
    assert st.shape == (6, 0) and lv.shape == (6, 0) and fq.shape == (3, 0)
    st, lv, fq = forest.predict_stages(X, 2, 2, leaves=True, freq=True)
    assert st.shape == (0, 5) and lv.shape == (0, 5) and fq.shape == (3, 5) and not bool(fq.any())
    st, fq = fo.Forest([], [], 3).predict_stages(X, freq=True)
    assert st.shape == (0, 5) and fq.shape == (3, 5) and not bool(fq.any())


# ---- hand-built forests behind a model ----
def model_and_frame(name, n=65):
    kinds, forest, X = case(name)
    h2o.init(verbose=False)
    names = [f"x{i}" for i in range(len(kinds))]
    m = SharedTreeModel(f"stages_{name}", {}, DataInfo(names, np.zeros(len(kinds), np.int32), [None] * len(kinds)))
    m.forest, m.device = forest, torch.device("cpu")
    forest.invalidate()
    fr = h2o.H2OFrame(pd.DataFrame(X[:, :n].T.numpy().astype(np.float64), columns=names))
    return m, forest, fr, X[:, :n].contiguous()


def spine_rows(forest, F):
    """One row per tree that follows the tree's spine to its deepest level (level d splits on feature d mod F, so
    a depth-33 spine over 33 features fixes every feature once)."""
    rows = []
    for tree in forest.trees:
        x = np.zeros(F, dtype=np.float32)
        n = 0
        while tree.feat[n] >= 0:
            l, r = int(tree.left[n]), int(tree.right[n])
            left = tree.feat[l] >= 0 or tree.feat[r] < 0          # towards the child that splits on
            f = int(tree.feat[n])
            if tree.is_cat[n]:
                bits = tree.cat_bits[n]
                lv = [c for c in range(int(tree.cat_nbits[n])) if bool((int(bits[c >> 5]) >> (c & 31)) & 1) == left]
                x[f] = lv[0] if lv else (np.nan if bool(tree.na_left[n]) == left else None)
            elif left:
                x[f] = -2.0 if np.isfinite(tree.thr[n]) else 0.0
            else:
                x[f] = np.inf
            n = l if left else r
        rows.append(x)
    return torch.from_numpy(np.stack(rows, 1))


def test_spine33_paths_and_ids():
    m, forest, fr, X = model_and_frame("spine33", 29)
    X = torch.cat([X, spine_rows(forest, X.shape[0])], 1).contiguous()
    fr = h2o.H2OFrame(pd.DataFrame(X.T.numpy().astype(np.float64), columns=m.info.x))
    paths = m.predict_leaf_node_assignment_frame(fr, "Path")
    ids = m.predict_leaf_node_assignment_frame(fr, "Node_ID")
    assert paths.names == ids.names == ["T1.C1", "T2.C1", "T3.C1", "T4.C1"]
    leaves = forest.predict_raw(X, return_leaves=True)[1]
    base, longest = 0, 0
    for t, tree in enumerate(forest.trees):
        col = paths._col(t)
        assert col.type == "enum" and list(col.domain) == sorted(set(col.domain))
        codes = col.data.numpy()
        assert set(codes.tolist()) == set(range(len(col.domain)))
        order = [0]                                        # breadth-first ids, as tree_json numbers the nodes
        for k in order:
            if tree.feat[k] >= 0:
                order += [int(tree.left[k]), int(tree.right[k])]
        bfs = {k: i for i, k in enumerate(order)}
        for i in range(X.shape[1]):
            n = 0
            for ch in col.domain[codes[i]]:
                assert tree.feat[n] >= 0
                n = int(tree.left[n] if ch == "L" else tree.right[n])
            assert n == int(leaves[i, t]) - base and tree.feat[n] < 0
            assert int(ids._col(t).data[i]) == bfs[n]
        longest = max(longest, max(len(p) for p in col.domain))
        base += tree.n_nodes
    assert longest == 33


def test_single_leaf_gives_empty_path_and_id_0():
    m, forest, fr, X = model_and_frame("single_leaf", 9)
    p = m.predict_leaf_node_assignment_frame(fr, "Path")._col(0)
    assert p.type == "enum" and list(p.domain) == [""] and not bool(p.data.any())
    i = m.predict_leaf_node_assignment_frame(fr, "Node_ID")._col(0)
    assert i.type == "int" and not bool(i.data.any())
    with pytest.raises(ValueError):
        m.predict_leaf_node_assignment_frame(fr, "Leaf")


def test_k3_column_names():
    m, forest, fr, X = model_and_frame("k3", 9)
    assert m.stage_column_names() == ["T1.C1", "T1.C2", "T1.C3", "T2.C1", "T2.C2", "T2.C3"]
    assert m.predict_leaf_node_assignment_frame(fr, "Node_ID").names == m.stage_column_names()


def test_feature_frequency_tensor_of_a_model():
    m, forest, fr, X = model_and_frame("cats")
    got = m.feature_frequencies_tensor(X)
    lv = forest.predict_stages(X, stage=False, leaves=True)
    assert np.array_equal(got.numpy().astype(np.int64), fs.climb_counts(forest, lv, X.shape[0])[0].T)


# ---- trained models through the facade ----
@pytest.fixture(scope="module")
def fr():
    return fs.training_frame()


@pytest.fixture(scope="module")
def gbm_reg(fr):
    return fs.estimator("gbm", "r", fr)


def test_regression_gbm(gbm_reg, fr):
    sp = fs.check_staged_equals_raw(gbm_reg, fr)
    assert sp.names == fs.stage_names(6)
    pred = gbm_reg.predict(fr)
    assert torch.equal(sp._col("T6.C1").data, pred._col("predict").data)
    init = gbm_reg._model.init_f[0]
    ids, paths, total, abs_total = fs.check_leaf_assignment(gbm_reg, fr, init)
    # predict = fp32(fp32 sum of 6 leaves + fp32(init_f)): 6 + 1 adds and the rounding of init_f, each at most
    # 2^-24 of sum |leaf| + |init_f|
    p = pred._col("predict").data.cpu().numpy()
    assert np.all(np.abs(total - p) <= 8 * 2.0 ** -24 * (abs_total + abs(init)))


def test_binomial_gbm(fr):
    est = fs.estimator("gbm", "y", fr)
    sp = fs.check_staged_equals_raw(est, fr)
    pred = est.predict(fr)
    first = est._model.info.response_domain[0]
    assert torch.equal(sp._col("T6.C1").data, pred._col(str(first)).data)
    fs.check_leaf_assignment(est, fr, est._model.init_f[0])


def test_multinomial_gbm(fr):
    est = fs.estimator("gbm", "y3", fr)
    sp = fs.check_staged_equals_raw(est, fr)
    assert sp.names == fs.stage_names(6, 3)
    pred = est.predict(fr)
    dom = est._model.info.response_domain
    for n in range(1, 7):
        s = sum(sp._col(f"T{n}.C{c + 1}").data for c in range(3))
        assert float((s - 1).abs().max()) <= 3 * 2.0 ** -23       # three fp32 probabilities, each rounded once
    for c, d in enumerate(dom):
        assert torch.equal(sp._col(f"T6.C{c + 1}").data, pred._col(str(d)).data)
    names = est.predict_leaf_node_assignment(fr, "Node_ID").names
    assert names == fs.stage_names(6, 3)


def test_drf_leaf_assignment_and_refusals(fr):
    est = fs.estimator("drf", "r", fr)
    fs.check_leaf_assignment(est, fr)
    with pytest.raises(ValueError, match="GBM"):
        est.staged_predict_proba(fr)
    with pytest.raises(ValueError):
        est.predict_leaf_node_assignment(fr, type="Leaf")
    with pytest.raises(ValueError):
        est.predict_leaf_node_assignment(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        est.staged_predict_proba(None)


def test_glm_refuses_both(fr):
    from h2o.estimators import H2OGeneralizedLinearEstimator
    glm = H2OGeneralizedLinearEstimator(family="gaussian")
    glm.train(x=fs.X_COLS, y="r", training_frame=fr)
    with pytest.raises(ValueError, match="trees"):
        glm.predict_leaf_node_assignment(fr)
    with pytest.raises(ValueError):
        glm.staged_predict_proba(fr)


def test_switch_restores_the_old_paths(gbm_reg, fr, monkeypatch):
    m = gbm_reg._model
    calls = []
    inner = m.forest.predict_stages
    monkeypatch.setattr(m.forest, "predict_stages", lambda *a, **k: calls.append(1) or inner(*a, **k))
    new_sp, new_ff = gbm_reg.staged_predict_proba(fr), gbm_reg.feature_frequencies(fr)
    n_new = len(calls)
    assert n_new >= 1
    monkeypatch.setenv("H2O_STAGES_HIP", "0")
    old_sp, old_ff = gbm_reg.staged_predict_proba(fr), gbm_reg.feature_frequencies(fr)
    assert len(calls) == n_new, "H2O_STAGES_HIP=0 called predict_stages"
    fs.frames_equal(new_sp, old_sp)
    fs.frames_equal(new_ff, old_ff)
    X, _ = fs.model_matrix(gbm_reg, fr)
    lv = inner(X, stage=False, leaves=True)
    ref = fs.climb_counts(m.forest, lv, X.shape[0])[0].T
    assert np.array_equal(np.stack([new_ff._col(n).data.cpu().numpy() for n in new_ff.names], 1), ref.astype(np.float64))


# ---- a frame sharded over two gloo ranks ----
def _sharded_worker(rank, world, port, csv, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), H2O_AMD_DEVICE="cpu", OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    import h2o as h
    from h2o.estimators import H2OGradientBoostingEstimator
    from llama_github_io_amd.parallel import collectives as coll, dframe
    h.init(verbose=False)
    fr = h.import_file(csv)
    assert fr._shard is not None and fr._shard.n_local < fr._shard.n_global
    res = {"cloud_size": h.cluster().cloud_size}
    for y in ("yr", "y3"):
        est = H2OGradientBoostingEstimator(ntrees=3, max_depth=3, seed=5)
        est.train(x=["x0", "x1", "x2", "x3", "cat"], y=y, training_frame=fr)
        whole = dframe.gather_frame(fr)
        assert whole._shard is None
        for call in (lambda f: est.predict_leaf_node_assignment(f, "Path"),
                     lambda f: est.predict_leaf_node_assignment(f, "Node_ID"), lambda f: est.staged_predict_proba(f)):
            a = call(fr)
            assert a._shard is not None
            a, b = a.as_data_frame(), call(whole).as_data_frame()
            assert list(a.columns) == list(b.columns) and len(a) == fr.nrows
            assert a.equals(b), y
        res[y] = list(a.columns)
    if coll.rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def test_sharded_frame_gives_the_unsharded_result(tmp_path):
    from test_distributed_api import _write_csv
    csv, out = str(tmp_path / "data.csv"), str(tmp_path / "out.json")
    _write_csv(csv, n=400)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, csv, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    with open(out) as f:
        res = json.load(f)
    assert res["cloud_size"] == 2
    assert res["yr"] == fs.stage_names(3) and res["y3"] == fs.stage_names(3, 3)

"""Staged predictions, leaf node assignment and feature frequencies on one GPU (profiles/forest_stages_gpu.md).

A GBM (bernoulli, 100 trees, depth 6, 28 numeric features) is trained per row count. Then, per row count:

* ``model.staged_predict_proba(fr)`` and ``model.feature_frequencies(fr)`` with the device path and with
  ``H2O_STAGES_HIP=0`` (one forest pass per stage; the NumPy walk on the host): a warm-up and the median of
  ``--runs`` synchronised runs; the NumPy walk takes ``--host-runs`` runs and no warm-up (it compiles and caches nothing);
* ``model.predict_leaf_node_assignment(fr, type)`` for both types (new: nothing to compare with), next to what the
  tensor method did before: ``Forest.predict_raw(return_leaves=True)``, with and without the transpose to columns;
* the forest calls alone, by device events over ``--reps`` back-to-back calls: ``Forest.predict_stages`` per
  output and for all three, ``Forest.predict_raw`` (k_predict) with and without leaves, and the loop of one
  ``predict_raw`` per stage that the staged call replaces.

    python scripts/bench_forest_stages.py --rows 10000 100000 1000000
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from h2o.estimators import H2OGradientBoostingEstimator  # noqa: E402
from llama_github_io_amd.frame import Column, H2OFrame  # noqa: E402

F = 28


def make_frame(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(F, n, device=dev, generator=g)
    logit = 2 * X[0] - X[1] + X[2] * X[3] + 0.5 * torch.sin(3 * X[4]) + (X[5] > 0.3).float() * X[6]
    y = (torch.rand(n, device=dev, generator=g) < torch.sigmoid(logit)).to(torch.int32)
    cols = [Column(f"x{i}", "real", X[i].double()) for i in range(F)]
    cols.append(Column("y", "enum", y, ["0", "1"]))
    return H2OFrame._from_columns(cols)


def timed(fn, runs=5, warm=True):
    """Median wall-clock milliseconds of ``fn`` between device synchronisations."""
    if warm:
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def device_ms(fn, reps=20):
    """Milliseconds per call by device events around ``reps`` back-to-back calls (after one warm-up call)."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--ntrees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forest_stages.py measures the device path: no GPU found")
    dev = torch.device(a.device)
    for n in a.rows:
        fr = make_frame(n, dev)
        est = H2OGradientBoostingEstimator(ntrees=a.ntrees, max_depth=a.depth, seed=1)
        est.train(x=[f"x{i}" for i in range(F)], y="y", training_frame=fr)
        m = est._model
        forest = m.forest
        T = len(forest.trees)
        res = dict(rows=n, ntrees=T, depth=a.depth, F=F)
        for hip in ("1", "0"):
            os.environ["H2O_STAGES_HIP"] = hip
            res[f"staged_predict_proba_hip{hip}_ms"] = timed(lambda: est.staged_predict_proba(fr), a.runs)
            if hip == "1":
                res["feature_frequencies_hip1_ms"] = timed(lambda: est.feature_frequencies(fr), a.runs)
            elif a.host_runs > 0:
                res["feature_frequencies_hip0_ms"] = timed(lambda: est.feature_frequencies(fr), a.host_runs, warm=False)
        os.environ.pop("H2O_STAGES_HIP")
        for ty in ("Path", "Node_ID"):
            res[f"leaf_node_assignment_{ty}_ms"] = timed(lambda: est.predict_leaf_node_assignment(fr, ty), a.runs)
        X, _ = fr.model_matrix(m.info, device=m.device)
        res["tensor_leaves_k_predict_ms"] = timed(lambda: m.predict_leaf_node_assignment(X), a.runs)
        res["tensor_leaves_k_predict_transposed_ms"] = timed(
            lambda: m.predict_leaf_node_assignment(X).T.contiguous(), a.runs)
        # the forest calls alone
        ev = lambda fn: device_ms(fn, a.reps)
        res["k_predict_ms"] = ev(lambda: forest.predict_raw(X))
        res["k_predict_leaves_ms"] = ev(lambda: forest.predict_raw(X, return_leaves=True))
        res["k_predict_leaves_transposed_ms"] = ev(lambda: forest.predict_raw(X, return_leaves=True)[1].T.contiguous())
        res["k_predict_per_stage_loop_ms"] = device_ms(
            lambda: [forest.predict_raw(X, 0, t + 1) for t in range(T)], max(1, a.reps // 10))
        res["stages_stage_ms"] = ev(lambda: forest.predict_stages(X))
        res["stages_leaves_ms"] = ev(lambda: forest.predict_stages(X, stage=False, leaves=True))
        res["stages_freq_ms"] = ev(lambda: forest.predict_stages(X, stage=False, freq=True))
        res["stages_all_ms"] = ev(lambda: forest.predict_stages(X, leaves=True, freq=True))
        res["fill_T_x_N_floats_ms"] = ev(lambda: torch.empty(T, n, device=dev).fill_(1.0))
        # same results on the timed inputs
        st = forest.predict_stages(X)
        assert torch.equal(st[T - 1], forest.predict_raw(X)[:, 0])
        assert torch.equal(forest.predict_stages(X, stage=False, leaves=True),
                           forest.predict_raw(X, return_leaves=True)[1].T.contiguous())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

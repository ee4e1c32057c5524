"""Partial dependence / Friedman H timings on one GPU (profiles/pdp_gpu.md).

A GBM (bernoulli, 100 trees, depth 6, 28 numeric features) is trained per row count; then ``model.partial_plot``
(1-D, nbins 20; one 2-D pair, nbins 20) and ``model.h`` (two variables) are timed: one warm-up, then the median
of 5 synchronised runs. Only public model methods are timed, so the script runs on commits from before the grid
kernel as well; there the kernel-only lines are skipped.

Kernel-only: ``Forest.predict_raw_grid`` (k_pd_node_masks + k_predict_grid) against G x ``Forest.predict_raw``
(k_predict) on the same tuples, and the mean number of distinct leaves per (row, tree) over the tuples, which is
the number of walks the grid kernel does where the loop does G.

    python scripts/bench_pdp.py --rows 100000 1000000
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llama_github_io_amd.frame import Column, H2OFrame  # noqa: E402
from llama_github_io_amd.models import builder  # noqa: E402

F = 28


def make_frame(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(F, n, device=dev, generator=g)
    logit = 2 * X[0] - X[1] + X[2] * X[3] + 0.5 * torch.sin(3 * X[4]) + (X[5] > 0.3).float() * X[6]
    y = (torch.rand(n, device=dev, generator=g) < torch.sigmoid(logit)).to(torch.int32)
    cols = [Column(f"x{i}", "real", X[i].double()) for i in range(F)]
    cols.append(Column("y", "enum", y, ["0", "1"]))
    return H2OFrame._from_columns(cols)


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def timed(fn, runs=5):
    fn()
    ts = []
    for _ in range(runs):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def distinct_leaves(forest, X, js, V, sample=20000):
    Xs = X[:, :sample].contiguous()
    leaves = []
    for g in range(V.shape[1]):
        Xg = Xs.clone()
        for s, j in enumerate(js):
            Xg[j] = V[s, g]
        leaves.append(forest.predict_raw(Xg, return_leaves=True)[1])
    srt = torch.stack(leaves).sort(0).values
    return float((1 + (srt[1:] != srt[:-1]).sum(0)).double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--ntrees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    for n in a.rows:
        fr = make_frame(n, dev)
        m = builder.train("gbm", dict(ntrees=a.ntrees, max_depth=a.depth, seed=1), x=[f"x{i}" for i in range(F)], y="y",
                          training_frame=fr)
        res = dict(rows=n, ntrees=a.ntrees, depth=a.depth, F=F, hip=os.environ.get("H2O_PDP_HIP", "1"),
                   grid_kernel=hasattr(m.forest, "predict_raw_grid"))
        res["pdp_1d_ms"] = timed(lambda: m.partial_plot(fr, ["x0"], nbins=20))
        res["pdp_2d_ms"] = timed(lambda: m.partial_plot(fr, [], nbins=20, col_pairs_2dpdp=[["x2", "x3"]]))
        res["h_ms"] = timed(lambda: m.h(fr, ["x2", "x3"]))
        X, _ = fr.model_matrix(m.info, device=m.device)
        for name, js in (("x0", [0]), ("x1", [1]), ("x20", [20]), ("x2_x3", [2, 3])):
            lo, hi = X[js].min(1).values, X[js].max(1).values
            ax = [torch.linspace(float(l), float(h), 20, device=dev) for l, h in zip(lo, hi)]
            V = ax[0][None] if len(js) == 1 else torch.stack([ax[0].repeat_interleave(20), ax[1].repeat(20)])
            V = V.float().contiguous()
            G = V.shape[1]
            res[f"leaves_{name}"] = distinct_leaves(m.forest, X, js, V)

            def loop():
                Xg = X.clone()
                for g in range(G):
                    for s, j in enumerate(js):
                        Xg[j] = V[s, g]
                    m.forest.predict_raw(Xg)
            res[f"k_predict_x{G}_{name}_ms"] = timed(loop)
            if res["grid_kernel"]:
                step = max(1, (256 << 20) // (G * m.forest.K * 4))
                res[f"k_predict_grid_{name}_ms"] = timed(
                    lambda: [m.forest.predict_raw_grid(X[:, r:r + step], js, V) for r in range(0, n, step)])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

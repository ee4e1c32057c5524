"""Permutation importance timings on one GPU (profiles/permvi_gpu.md).

A GBM (bernoulli, 100 trees, depth 6, 28 numeric features) is trained per row count; then
``model.permutation_importance(fr, n_samples=-1, n_repeats=r)`` is timed for r = 1 and 5, with the device path and
with ``H2O_PERMVI_HIP=0`` (the re-scoring loop): one warm-up, then the median of 5 synchronised runs. Only public
model methods are timed, so the script runs on commits from before the kernel as well; there the variable has no
effect and the kernel-only and host-side lines are skipped.

Kernel-only: ``Forest.predict_raw_permuted`` (k_predict_permuted, variants in chunks of 256 MiB of margins and
indices, per chunk size of the kernel) against J x (clone of X + overwrite + ``Forest.predict_raw``) on the same
index rows, and the mean number of diverging variants per (row, tree): the extra sub-walks the kernel makes where
the loop makes J full walks. Host side: the time to draw the J permutations with ``torch.randperm`` on the CPU
and copy them to the device as int32, which stays on the host on both paths.

    python scripts/bench_permvi.py --rows 10000 100000 1000000
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
from llama_github_io_amd.ops import forest as fo  # noqa: E402

F = 28
CHUNK_BYTES = 256 << 20


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


def draw(n, J, dev, seed=1234):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.stack([torch.randperm(n, generator=g).to(torch.int32) for _ in range(J)]).to(dev)


def diverging(forest, X, feats, src, sample=20000):
    """Mean number of variants per (row, tree) that reach a leaf other than the row's own, on the first rows
    (the index rows are taken modulo the sample)."""
    Xs = X[:, :sample].contiguous()
    n = Xs.shape[1]
    own = forest.predict_raw(Xs, return_leaves=True)[1]
    tot = torch.zeros_like(own, dtype=torch.int64)
    for j, f in enumerate(feats):
        Xp = Xs.clone()
        Xp[f] = Xs[f][(src[j, :n].long() % n)]
        tot += forest.predict_raw(Xp, return_leaves=True)[1] != own
    return float(tot.double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--ntrees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--repeats", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--chunks", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    dev = torch.device(a.device)
    for n in a.rows:
        fr = make_frame(n, dev)
        est = H2OGradientBoostingEstimator(ntrees=a.ntrees, max_depth=a.depth, seed=1)
        est.train(x=[f"x{i}" for i in range(F)], y="y", training_frame=fr)
        m = est._model
        kernel = hasattr(m.forest, "predict_raw_permuted")
        res = dict(rows=n, ntrees=a.ntrees, depth=a.depth, F=F, kernel=kernel)
        for r in a.repeats:
            for hip in ("1", "0"):
                os.environ["H2O_PERMVI_HIP"] = hip
                res[f"permvi_r{r}_hip{hip}_ms"] = timed(
                    lambda: est.permutation_importance(fr, n_samples=-1, n_repeats=r, seed=1))
            os.environ.pop("H2O_PERMVI_HIP")
        if kernel:
            X, _ = fr.model_matrix(m.info, device=m.device)
            K = m.forest.K
            for r in a.repeats:
                J = F * r
                feats = [j // r for j in range(J)]
                res[f"host_randperm_h2d_J{J}_ms"] = timed(lambda: draw(n, J, dev))
                src = draw(n, J, dev)
                res[f"diverging_J{J}"] = diverging(m.forest, X, feats, src)

                def loop():
                    for j, f in enumerate(feats):
                        Xp = X.clone()
                        Xp[f] = X[f][src[j].long()]
                        m.forest.predict_raw(Xp)
                res[f"clone_k_predict_x{J}_ms"] = timed(loop)
                step = max(1, CHUNK_BYTES // (n * (K + 1) * 4))
                default = fo.PV_CHUNK
                for c in a.chunks:
                    fo.PV_CHUNK = c
                    res[f"k_predict_permuted_J{J}_chunk{c}_ms"] = timed(
                        lambda: [m.forest.predict_raw_permuted(X, feats[v:v + step], src[v:v + step])
                                 for v in range(0, J, step)])
                fo.PV_CHUNK = default
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""TreeSHAP on device against the host recursion: kernel time, end-to-end ``predict_contributions`` time and
the time of the ``H2O_SHAP_HIP=0`` host path for the same call, in one process.

Synthetic full trees over F = 28 numeric features: 100 trees x depth 6 and 50 trees x depth 12; N = 1k / 100k /
1M rows on the GPU, 1k / 100k on the host (the host rate is per row; a host run projected from the 1k rate to
take longer than ``--cpu-seconds`` is not run, its projected time is printed with a ``~``).

    python scripts/bench_shap.py [--rows 1000,100000,1000000] [--forests 100x6,50x12] [--out profiles/shap_gpu.md]
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llama_github_io_amd import explain  # noqa: E402
from llama_github_io_amd.frame import H2OFrame  # noqa: E402
from llama_github_io_amd.models.base import DataInfo  # noqa: E402
from llama_github_io_amd.ops import _native as nat, shap  # noqa: E402
from llama_github_io_amd.ops.forest import Forest, Tree  # noqa: E402

F = 28


def full_tree(rng, depth: int) -> Tree:
    """A full binary tree in heap order (children of i: 2i+1, 2i+2), random numeric splits, positive covers."""
    n_int, n = (1 << depth) - 1, (1 << (depth + 1)) - 1
    feat = np.full(n, -1, np.int32)
    feat[:n_int] = rng.integers(0, F, n_int)
    thr = np.zeros(n, np.float32)
    thr[:n_int] = rng.normal(size=n_int)
    idx = np.arange(n)
    left = np.where(idx < n_int, 2 * idx + 1, -1).astype(np.int32)
    right = np.where(idx < n_int, 2 * idx + 2, -1).astype(np.int32)
    cover = np.zeros(n, np.float64)
    cover[n_int:] = rng.uniform(1.0, 10.0, n - n_int)
    for i in range(n_int - 1, -1, -1):
        cover[i] = cover[2 * i + 1] + cover[2 * i + 2]
    value = np.zeros(n, np.float32)
    value[n_int:] = rng.normal(size=n - n_int) * 0.1
    return Tree(feat=feat, thr=thr, bin=np.zeros(n, np.int32), na_left=rng.integers(0, 2, n).astype(np.int8),
                is_cat=np.zeros(n, np.int8), cat_bits=[None] * n, cat_nbits=np.zeros(n, np.int32), left=left, right=right,
                value=value, cover=cover, gain=np.zeros(n, np.float64))


def fake_model(forest, dev):
    names = [f"x{i}" for i in range(F)]
    info = DataInfo(names, np.zeros(F, np.int32), [None] * F, "y", None)
    return SimpleNamespace(forest=forest, info=info, model_category="Regression", algo="gbm", init_f=0.25, device=dev,
                           ntrees_built=lambda: len(forest.trees))


def kernel_ms(paths, X, K):
    """One launch of h2o_tree_shap between two events, after a launch that warmed it up."""
    Fx, N = X.shape
    d = paths.on(X.device)
    out = torch.zeros(N, K, Fx + 1, dtype=torch.float64, device=X.device)

    def launch():
        nat.call("h2o_tree_shap", X.data_ptr(), N, Fx, K, d["view"], 0, out.data_ptr(), nat.stream_ptr(X.device))

    if N <= 100_000:
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000,100000,1000000")
    ap.add_argument("--forests", default="100x6,50x12")
    ap.add_argument("--cpu-rows", default="1000,100000")
    ap.add_argument("--cpu-seconds", type=float, default=45.0)
    ap.add_argument("--out", default=None, help="append the table (markdown) to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = [int(x) for x in a.rows.split(",")]
    cpu_rows = {int(x) for x in a.cpu_rows.split(",") if x}
    lines = ["| forest | paths | G | N | kernel ms | predict_contributions ms (device) | host path ms | host / device |",
             "|---|---|---|---|---|---|---|---|"]
    for spec in a.forests.split(","):
        nt, depth = (int(x) for x in spec.split("x"))
        rng = np.random.default_rng(nt * 100 + depth)
        forest = Forest([full_tree(rng, depth) for _ in range(nt)], [0] * nt, 1)
        t0 = time.perf_counter()
        paths = shap.forest_paths(forest)
        t_paths = time.perf_counter() - t0
        print(f"# {spec}: {paths.n_paths} paths, longest {paths.max_len} elements, G = {paths.G}, "
              f"path table built on the host in {t_paths:.2f} s (once per forest)", flush=True)
        model = fake_model(forest, dev)
        g = torch.Generator(device=dev).manual_seed(1)
        cpu_rate = None                      # ms per row of the host path, from the first host run
        warm = H2OFrame.from_tensor(torch.randn(1000, F, device=dev, generator=g), model.info.x)
        explain.predict_contributions(model, warm)
        for N in rows:
            Xt = torch.randn(N, F, device=dev, generator=g)
            fr = H2OFrame.from_tensor(Xt, model.info.x)
            X = Xt.T.contiguous().float()
            k_ms = kernel_ms(paths, X, 1)
            os.environ.pop("H2O_SHAP_HIP", None)
            e2e_ms, out = wall(lambda: explain.predict_contributions(model, fr))
            assert out._col("x0").data.is_cuda
            host = ""
            ratio = ""
            if N in cpu_rows:
                if cpu_rate is not None and cpu_rate * N / 1e3 > a.cpu_seconds:
                    host, ratio = f"~{cpu_rate * N:.0f}", f"~{cpu_rate * N / e2e_ms:.1f}"
                else:
                    os.environ["H2O_SHAP_HIP"] = "0"
                    h_ms, ref = wall(lambda: explain.predict_contributions(model, fr))
                    os.environ.pop("H2O_SHAP_HIP")
                    cpu_rate = h_ms / N
                    err = max(float((out._col(n).data.cpu() - ref._col(n).data).abs().max()) for n in out.names)
                    host, ratio = f"{h_ms:.1f}", f"{h_ms / e2e_ms:.1f}"
                    print(f"#   N={N}: max |device - host| = {err:.2e}", flush=True)
            line = f"| {spec} | {paths.n_paths} | {paths.G} | {N} | {k_ms:.2f} | {e2e_ms:.1f} | {host} | {ratio} |"
            print(line, flush=True)
            lines.append(line)
            del Xt, fr, X, out
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

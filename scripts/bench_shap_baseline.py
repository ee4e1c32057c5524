"""Baseline SHAP on device against the PyTorch evaluation of the same path table on the host, in one process:
time of the ``h2o_tree_shap_baseline`` launcher, of ``predict_contributions(background_frame=...)`` end to end, and
of ``ops.shap.path_shap_baseline`` on CPU tensors.

The forest of scripts/bench_shap.py: 100 full trees of depth 6 over F = 28 numeric features (6400 paths, G = 8),
standard-normal rows. N x B = 1k x 100 and 1k x 1k averaged over the background, 1k x 100 per reference. The host
evaluation of a case with more than ``--cpu-pairs`` pairs runs on its first rows only and is scaled up (printed
with a ``~``; its cost is per pair).

    python scripts/bench_shap_baseline.py [--cases 1000x100,1000x1000,1000x100r] [--out profiles/shap_baseline_gpu.md]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_shap import F, fake_model, full_tree, wall  # noqa: E402
from llama_github_io_amd import explain  # noqa: E402
from llama_github_io_amd.frame import H2OFrame  # noqa: E402
from llama_github_io_amd.ops import shap  # noqa: E402
from llama_github_io_amd.ops.forest import Forest  # noqa: E402


def kernel_ms(paths, X, Bg, per_reference, reps=3):
    """Median time of one call of the launcher (all its launches) between two events, after a warm-up call."""
    rows = X.shape[1] * (Bg.shape[1] if per_reference else 1)
    out = torch.zeros(rows, 1, F + 1, dtype=torch.float64, device=X.device)
    shap.path_shap_baseline(paths, X, Bg, 1, per_reference=per_reference, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        out.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        shap.path_shap_baseline(paths, X, Bg, 1, per_reference=per_reference, out=out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1000x100,1000x1000,1000x100r", help="NxB, a trailing r = per reference")
    ap.add_argument("--cpu-pairs", type=int, default=20_000)
    ap.add_argument("--out", default=None, help="append the table (markdown) to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nt, depth = 100, 6
    rng = np.random.default_rng(nt * 100 + depth)
    forest = Forest([full_tree(rng, depth) for _ in range(nt)], [0] * nt, 1)
    paths = shap.forest_paths(forest)
    P = paths.n_paths
    print(f"# {nt}x{depth}: {P} paths, longest {paths.max_len} elements, G = {paths.G}", flush=True)
    model = fake_model(forest, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    lines = ["| N x B | output | kernel ms | ps per (row, background row, path) | predict_contributions ms (device) | "
             "host evaluation ms | host / kernel | max abs device - host |",
             "|---|---|---|---|---|---|---|---|"]
    for spec in a.cases.split(","):
        per_ref = spec.endswith("r")
        N, B = (int(x) for x in spec.rstrip("r").split("x"))
        Xt, Bt = torch.randn(N, F, device=dev, generator=g), torch.randn(B, F, device=dev, generator=g)
        X, Bg = Xt.T.contiguous().float(), Bt.T.contiguous().float()
        k_ms, out = kernel_ms(paths, X, Bg, per_ref)
        fr, bg = H2OFrame.from_tensor(Xt, model.info.x), H2OFrame.from_tensor(Bt, model.info.x)
        os.environ.pop("H2O_SHAP_HIP", None)
        explain.predict_contributions(model, fr, background_frame=bg, output_per_reference=per_ref)
        e2e_ms, res = wall(lambda: explain.predict_contributions(model, fr, background_frame=bg,
                                                                 output_per_reference=per_ref))
        assert res._col("x0").data.is_cuda
        n_cpu = N if N * B <= a.cpu_pairs else max(1, a.cpu_pairs // B)
        Xc, Bc = X[:, :n_cpu].cpu(), Bg.cpu()
        t = time.perf_counter()
        ref = shap.path_shap_baseline(paths, Xc, Bc, 1, per_reference=per_ref)
        c_ms = (time.perf_counter() - t) * 1e3 * (N / n_cpu)
        err = float((out[:ref.shape[0]].cpu() - ref).abs().max())
        mark = "" if n_cpu == N else "~"
        line = (f"| {N} x {B} | {'per reference' if per_ref else 'averaged'} | {k_ms:.2f} | {k_ms * 1e9 / (N * B * P):.1f} | "
                f"{e2e_ms:.1f} | {mark}{c_ms:.0f} | {mark}{c_ms / k_ms:.0f} | {err:.2e} |")
        print(line, flush=True)
        lines.append(line)
        del Xt, Bt, X, Bg, out, res, fr, bg
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Shared cases and NumPy references of the Uplift DRF tests (test_uplift_paths.py, test_uplift_gpu.py): the level
histogram (``np.add.at`` into int64), the row routing (a loop over the rows), the uplift metric formulas written
independently of ``models/uplift.py`` and the frames the forests are grown from."""
import functools

import numpy as np

NA_BIN = 255
HIST_ROWS = (1, 63, 64, 65, 1000, 70001)        # 70001: 18 row tiles of the LDS variant, the last one partial
HIST_FEATURES = (1, 3, 28, 33)                  # 33: more features than one block's feature group at any window
# (first slot, nodes): one node, a few, the LDS variant's limit and one past it, 64 / 65, a wide level; all with n0 > 0
HIST_WINDOWS = ((3, 1), (1, 2), (2, 7), (5, 32), (4, 33), (1, 64), (2, 65), (3, 300))
HIST_LEVEL = 305                                # node slots of the level the windows are cut from
ROUTE_ROWS = (1, 65, 1000, 70001)


def hist_inputs(N, F, seed=0):
    """bins uint8 [N, stride > F], node int32 [N] in [-1, HIST_LEVEL), treat / y uint8 [N]. About a tenth of the rows
    are outside the level, bin 255 is populated in every feature, and the columns past F hold 255s that must not be
    read as features."""
    rng = np.random.default_rng(1000 * F + N + seed)
    stride = F + 1 + (F % 3)
    bins = rng.integers(0, 256, (N, stride), dtype=np.uint8)
    bins[:, F:] = 255
    bins[rng.random((N, stride)) < 0.05] = NA_BIN
    node = rng.integers(0, HIST_LEVEL, N).astype(np.int32)
    node[rng.random(N) < 0.1] = -1
    treat = rng.integers(0, 2, N, dtype=np.uint8)
    y = rng.integers(0, 2, N, dtype=np.uint8)
    return bins, node, treat, y


def hist_reference(bins, node, treat, y, F, A):
    """int64 [A, F, 256, 4] = (n_treat, y_treat, n_ctrl, y_ctrl) per node slot, feature and bin."""
    H = np.zeros((A, F, 256, 4), np.int64)
    rows = np.nonzero((node >= 0) & (node < A))[0]
    t, yy = treat[rows].astype(np.int64), y[rows].astype(np.int64)
    stats = np.stack([t, t * yy, 1 - t, (1 - t) * yy], 1)
    for f in range(F):
        np.add.at(H, (node[rows], f, bins[rows, f]), stats)
    return H


def route_inputs(N, F=5, A=37, seed=0):
    """bins, node and a route table with leaves (child -1), thresholds at both ends of the bin range, rows outside the
    level and NA bins."""
    rng = np.random.default_rng(77 * N + seed)
    bins = rng.integers(0, 40, (N, F + 2), dtype=np.uint8)
    bins[rng.random((N, F + 2)) < 0.1] = NA_BIN
    node = rng.integers(0, A, N).astype(np.int32)
    node[rng.random(N) < 0.15] = -1
    split_feat = rng.integers(0, F, A).astype(np.int32)
    split_bin = rng.integers(1, 41, A).astype(np.int32)
    split_bin[0], split_bin[1] = 1, 255
    child = np.full(A, -1, np.int32)
    keep = np.nonzero(rng.random(A) < 0.7)[0]
    child[keep] = 2 * np.arange(keep.size, dtype=np.int32)
    return bins, node, split_feat, split_bin, child


def route_reference(bins, node, split_feat, split_bin, child):
    out = np.full(node.shape, -1, np.int32)
    for r in range(node.size):
        n = node[r]
        if n >= 0 and child[n] >= 0:
            out[r] = child[n] + (0 if bins[r, split_feat[n]] < split_bin[n] else 1)
    return out


def uplift_metrics_reference(uplift, y, treat, nbins, kind):
    """The metric formulas from the curves up: thresholds are the uplift values at ``nbins`` evenly spaced descending
    ranks, a threshold's counts are those of the rows scoring at or above it."""
    u = np.asarray(uplift, np.float64)
    y, t = np.asarray(y, np.float64), np.asarray(treat, np.float64)
    N = u.size
    m = min(nbins, N)
    idx = np.clip(np.linspace(0, N - 1, m).astype(np.int64), 0, N - 1)
    thr = np.sort(u)[::-1][idx]
    nt = np.array([t[u >= h].sum() for h in thr])
    nc = np.array([(1 - t)[u >= h].sum() for h in thr])
    yt = np.array([(y * t)[u >= h].sum() for h in thr])
    yc = np.array([(y * (1 - t))[u >= h].sum() for h in thr])
    lift = yt / np.maximum(nt, 1) - yc / np.maximum(nc, 1)
    curves = dict(qini=yt - yc * nt / np.maximum(nc, 1), lift=lift, gain=lift * (nt + nc))
    n = nt + nc
    random = {k: c[-1] * n / n[-1] for k, c in curves.items()}
    normalized = {k: (c / abs(c[-1]) if k != "lift" and c[-1] != 0 else c) for k, c in curves.items()}
    out = dict(thresholds=thr, n=n, curves=curves, random=random, normalized=normalized,
               auuc={k: c.mean() for k, c in curves.items()},
               auuc_normalized={k: c.mean() for k, c in normalized.items()},
               auuc_random={k: c.mean() for k, c in random.items()},
               ate=u.mean(), att=u[t == 1].mean(), atc=u[t == 0].mean())
    out["aecu"] = {k: out["auuc"][k] - out["auuc_random"][k] for k in curves}
    out["kind"] = kind
    return out


@functools.lru_cache(maxsize=None)
def frame_data(n, n_num, seed=0):
    """Columns of a synthetic uplift frame: ``n_num`` numeric predictors (x1 with NaNs), one categorical, a 0/1
    treatment whose effect depends on x0 and on the category, and a binary response."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, n_num))
    cat = np.array(["p", "q", "r", "s"])[rng.integers(0, 4, n)]
    t = rng.integers(0, 2, n)
    logit = 0.6 * X[:, 0] - 0.4 * X[:, 1] + t * (0.9 * (X[:, 0] > 0) + 0.5 * (cat == "q") - 0.3) - 0.2
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(int)
    X[rng.random(n) < 0.07, 1] = np.nan
    cols = {f"x{j}": X[:, j] for j in range(n_num)}
    cols.update(c=cat, trt=np.where(t == 1, "treat", "ctrl"), y=np.where(y == 1, "yes", "no"))
    return cols


def frame(n, n_num, seed=0):
    import pandas as pd

    import h2o
    fr = h2o.H2OFrame(pd.DataFrame(frame_data(n, n_num, seed)))
    for c in ("c", "trt", "y"):
        fr[c] = fr[c].asfactor()
    return fr


def predictors(n_num):
    return [f"x{j}" for j in range(n_num)] + ["c", "trt"]

"""Model explanation (reference: ``hex/genmodel/algos/tree/TreeSHAP.java`` + ``SharedTreeModel.
scoreContributions`` (predict_contributions), ``hex/PartialDependence.java`` (partial_plot),
``hex/tree/FriedmanPopescusH.java`` (h statistic), ``hex/FeatureInteractions*.java``).

* ``predict_contributions``: exact path-dependent TreeSHAP; on a CUDA model the path-decomposed HIP kernel
  of ``ops/shap.py`` / ``csrc/shap_kernels.hip``, else the native runtime (``csrc/treeshap.cpp``,
  one thread per row range) over the flat forest; output columns = features + ``BiasTerm`` in the
  link (margin) space, summing to the raw prediction (GBM adds init_f, DRF averages trees), or the
  sorted ``top_n`` / ``bottom_n`` pairs of h2o-py. With a ``background_frame``: baseline (interventional) SHAP
  against its rows (``csrc/shap_baseline_kernels.hip`` on a CUDA model), averaged or per reference, in the margin
  or the output space.
* ``partial_plot``: mean, sd, std err of the response with a column (or a column pair) set to each grid value
  (equally spaced over [min, max] / levels); multinomial targets, ICE rows, weights. A tree model on a CUDA
  device (GBM, DRF, XGBoost tree boosters, isolation forest) gets the margins of every (grid tuple, row) from one
  pass of the grid-forking kernel (``Forest.predict_raw_grid`` / ``csrc/pdp_kernels.hip``: no copy of the model
  matrix, one tree walk per distinct leaf) and the response from ``Model.score_from_raw``; ``H2O_PDP_HIP=0``,
  CPU models and every other model overwrite the column and re-score the frame once per grid value.
* ``h``: Friedman–Popescu H² from centred partial dependences on the training rows (same two paths; the grid
  tuples are the sampled rows' own values).
* ``feature_interaction``: xgbfi statistics of split-feature paths (gain, F-score, weighted F-score,
  expected gain, ranks), leaf statistics and split-value histograms.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from .frame import Column, H2OFrame


def _rt():
    from .ops import _native
    lib = _native.rt()
    if not getattr(lib, "_shap_bound", False):
        c = ctypes
        lib.h2o_treeshap.argtypes = [c.c_void_p, c.c_longlong, c.c_int, c.c_int, c.c_int] + [c.c_void_p] * 14 + [c.c_int]
        lib.h2o_treeshap.restype = c.c_int
        lib._shap_bound = True
    return lib


def tree_shap(forest, X: torch.Tensor, nthreads: int = 0) -> np.ndarray:
    """X [F, N] -> contributions [N, K, F+1] (float64, margin space, per-tree sums)."""
    fl = forest.flatten()
    cover = np.concatenate([t.cover.astype(np.float64) for t in forest.trees]) if forest.trees else np.zeros(1)
    depth = np.array([t.depth() for t in forest.trees], dtype=np.int32)
    Xr = np.ascontiguousarray(X.detach().float().cpu().numpy().T)
    N, F = Xr.shape
    K = forest.K
    out = np.zeros((N, K, F + 1), dtype=np.float64)
    arrs = [fl["roots"], fl["cls"], depth, fl["feat"], fl["thr"], fl["left"], fl["right"], fl["na_left"], fl["cat_off"],
            fl["cat_bits"], fl["cat_nbits"], fl["value"], cover]
    arrs = [np.ascontiguousarray(a) for a in arrs]
    _rt().h2o_treeshap(Xr.ctypes.data, N, F, K, len(forest.trees), *[a.ctypes.data for a in arrs], out.ctypes.data,
                       int(nthreads))
    return out


def tree_shap_device(forest, X: torch.Tensor) -> torch.Tensor:
    """X [F, N] -> contributions [N, K, F+1] (float64, margin space, per-tree sums) on X's device, through the
    path table of ``ops/shap.py``: the HIP kernel for CUDA tensors, its PyTorch reference for CPU tensors. A
    path needs a lane per element, so a forest whose longest path has more than ``ops.shap.MAX_PATH_LEN`` (64)
    elements stays on the CPU recursion (:func:`tree_shap`) and only the result is moved to X's device."""
    from .ops import shap
    paths = shap.forest_paths(forest)
    if paths.max_len > shap.MAX_PATH_LEN:
        return torch.from_numpy(tree_shap(forest, X)).to(X.device)
    return shap.path_shap(paths, X, forest.K)


def _sorted_contributions(c: torch.Tensor, names, top_n, bottom_n, compare_abs):
    """h2o-py ``top_n`` / ``bottom_n`` / ``compare_abs``: per row the feature contributions sorted descending (by
    magnitude with ``compare_abs``), as ``top_feature_i, top_value_i`` pairs, then ``bottom_*`` pairs (smallest
    first), then ``BiasTerm``. A negative count, ``top_n + bottom_n >= F``, or ``compare_abs`` with neither count,
    returns every feature as ``top_*``."""
    F = len(names)
    top, bot = int(top_n or 0), int(bottom_n or 0)
    if top < 0 or bot < 0 or top + bot >= F or top + bot == 0:      # compare_abs alone: everything, by magnitude
        top, bot = F, 0
    phi = c[:, :F]
    order = torch.sort(phi.abs() if compare_abs else phi, dim=1, descending=True, stable=True).indices
    vals = torch.gather(phi, 1, order)
    cols = []
    for kind, n, pos in (("top", top, lambda i: i), ("bottom", bot, lambda i: F - 1 - i)):
        for i in range(n):
            cols.append(Column(f"{kind}_feature_{i + 1}", "enum", order[:, pos(i)].to(torch.int32), list(names)))
            cols.append(Column(f"{kind}_value_{i + 1}", "real", vals[:, pos(i)].contiguous()))
    cols.append(Column("BiasTerm", "real", c[:, F].contiguous()))
    return H2OFrame._from_columns(cols)


def _margin_linkinv(m):
    """What the model applies to its margin when scoring, as a tensor function; None when it applies nothing
    (identity links, DRF), so that output-space contributions equal the margin-space ones."""
    if m.algo == "gbm":
        d = m.distribution
        if d.name in ("bernoulli", "quasibinomial", "modified_huber"):
            return torch.sigmoid
        if d.link == "identity":
            return None
        if d.name == "custom":
            raise NotImplementedError("output_space is not available for a custom distribution")
        return d.linkinv
    if m.algo == "xgboost":
        d = m.output.get("distribution")
        if d == "bernoulli":
            return torch.sigmoid
        if d in ("poisson", "gamma", "tweedie"):
            return torch.exp
    return None


def _to_output_space(c: torch.Tensor, linkinv) -> torch.Tensor:
    """In place, per row of ``c`` (one (row, background row) pair: features..., bias): the feature cells are scaled
    so that they sum to ``linkinv(f(x)) - linkinv(f(b))`` and the bias becomes ``linkinv(f(b))``. Where the
    features sum to (almost) nothing the scale is the slope of ``linkinv`` at ``f(b)``."""
    F = c.shape[1] - 1
    d = c[:, :F].sum(1)
    fb = c[:, F].clone()
    h = 1e-6
    flat = d.abs() < 1e-12
    secant = (linkinv(fb + d) - linkinv(fb)) / torch.where(flat, torch.ones_like(d), d)
    slope = (linkinv(fb + h) - linkinv(fb - h)) / (2 * h)
    c[:, :F] *= torch.where(flat, slope, secant)[:, None]
    c[:, F] = linkinv(fb)
    return c


def _baseline_contributions(m, frame, background_frame, output_space, per_reference, top_n, bottom_n, compare_abs):
    """Baseline SHAP of ``frame`` against ``background_frame`` (``ops/shap.py`` :func:`path_shap_baseline`): the mean
    over the background rows, or one row per (row, background row)."""
    from .ops import shap
    if m.model_category == "Multinomial":
        raise NotImplementedError("contributions for multinomial models are not supported (as in H2O)")
    dev = torch.device(getattr(m, "device", None) or "cpu")
    if dev.type != "cuda" or os.environ.get("H2O_SHAP_HIP", "1") == "0":
        dev = torch.device("cpu")
    X, _ = frame.model_matrix(m.info, device=dev)
    Bg, _ = background_frame.model_matrix(m.info, device=dev)
    N, B, F = int(X.shape[1]), int(Bg.shape[1]), int(X.shape[0])
    if B == 0:
        raise ValueError("background_frame has no rows")
    limit = int(os.environ.get("H2O_SHAP_MAX_OUT_BYTES", 8 << 30))
    if per_reference and N * B * (F + 3) * 8 > limit:
        raise ValueError(f"output_per_reference: {N} rows x {B} background rows x {F + 3} columns of 8 bytes exceed "
                         f"H2O_SHAP_MAX_OUT_BYTES = {limit}")
    paths = shap.forest_paths(m.forest)
    K = m.forest.K
    scale = 1.0 / max(1, m.ntrees_built()) if m.algo == "drf" else 1.0
    init = getattr(m, "init_f", 0.0)
    init = float((init[0] if isinstance(init, (list, tuple)) else init) or 0.0)
    linkinv = _margin_linkinv(m) if output_space else None

    def pairs(Bc):
        """[N * b, F+1]: every pair of a row with a background row of Bc, DRF average and init_f applied."""
        c = shap.path_shap_baseline(paths, X, Bc, K, per_reference=True)[:, 0, :]
        if scale != 1.0:
            c = c * scale
        c[:, -1] += init
        return _to_output_space(c, linkinv) if linkinv is not None else c

    if per_reference:
        c = pairs(Bg)
    elif linkinv is None:
        c = shap.path_shap_baseline(paths, X, Bg, K)[:, 0, :] * (scale / B)
        c[:, -1] += init
    else:
        # the link is applied per pair: per-reference values of a background chunk in a bounded temporary
        step = max(1, min(B, (256 << 20) // max(1, N * (F + 1) * 8)))
        c = torch.zeros(N, F + 1, dtype=torch.float64, device=dev)
        for b0 in range(0, B, step):
            c += pairs(Bg[:, b0:b0 + step]).view(N, -1, F + 1).sum(1)
        c /= B
    names = list(m.info.x)
    if top_n or bottom_n or compare_abs:
        out = _sorted_contributions(c, names, top_n, bottom_n, compare_abs)
        cols = [out._col(n) for n in out.names]
    else:
        cols = [Column(n, "real", c[:, i]) for i, n in enumerate(names + ["BiasTerm"])]
    if per_reference:
        pair = torch.arange(N * B, device=dev)
        cols.append(Column("RowIdx", "int", torch.div(pair, B, rounding_mode="floor").double()))
        cols.append(Column("BackgroundRowIdx", "int", (pair % B).double()))
    return H2OFrame._from_columns(cols)


def predict_contributions(model, frame, output_format="Original", top_n=None, bottom_n=None, compare_abs=False,
                          background_frame=None, output_space=False, output_per_reference=False):
    """TreeSHAP contributions of every row, in the margin space: ``features..., BiasTerm``.

    A model on a CUDA device is explained on that device (model matrix, ``ops/shap.py`` path kernel, DRF
    averaging and ``init_f``; the columns are float64 CUDA tensors) unless ``H2O_SHAP_HIP=0``; otherwise the
    host recursion of ``csrc/treeshap.cpp`` runs. ``top_n`` / ``bottom_n`` / ``compare_abs`` follow h2o-py
    (:func:`_sorted_contributions`). ``output_format`` is ``"Original"`` or ``"Compact"``: the two differ in the
    reference only for one-hot encoded XGBoost models, and this engine never one-hot encodes, so they are
    identical here.

    With a ``background_frame`` the contributions are baseline (interventional) SHAP: per row ``x`` and background
    row ``b`` the Shapley values of ``v(S) = f(x_S, b_~S)``, so the features sum to ``f(x) - f(b)`` and ``BiasTerm``
    is ``f(b)``; returned as the mean over the background rows, or with ``output_per_reference=True`` as one row
    per (row, background row) in that order, followed by the int columns ``RowIdx`` and ``BackgroundRowIdx`` (refused
    with ``ValueError`` past ``H2O_SHAP_MAX_OUT_BYTES``, default 8 GiB). ``output_space=True`` rescales every
    pair, before averaging, so that it sums to the model's prediction (the probability of a binomial GBM / XGBoost)
    instead of the margin (``NotImplementedError`` for a custom distribution with a link). A CUDA model runs
    ``k_shap_baseline`` (``csrc/shap_baseline_kernels.hip``); a CPU model, or ``H2O_SHAP_HIP=0``, the fp64 PyTorch
    evaluation of the same path table."""
    m = getattr(model, "_model", model)
    if not hasattr(m, "forest") or m.forest is None:
        raise NotImplementedError("predict_contributions is available for tree models (GBM, DRF, XGBoost)")
    if str(output_format).lower() not in ("original", "compact"):
        raise ValueError(f"output_format must be 'Original' or 'Compact', got {output_format!r}")
    if background_frame is not None:
        return _baseline_contributions(m, frame, background_frame, bool(output_space), bool(output_per_reference),
                                       top_n, bottom_n, compare_abs)
    if output_space or output_per_reference:
        raise ValueError("output_space and output_per_reference need a background_frame")
    init = getattr(m, "init_f", 0.0)
    init = init[0] if isinstance(init, (list, tuple)) else init
    dev = torch.device(getattr(m, "device", None) or "cpu")
    if dev.type == "cuda" and os.environ.get("H2O_SHAP_HIP", "1") != "0":
        if m.model_category == "Multinomial":
            raise NotImplementedError("contributions for multinomial models are not supported (as in H2O)")
        X, _ = frame.model_matrix(m.info, device=dev)
        c = tree_shap_device(m.forest, X)[:, 0, :]
        if m.algo == "drf":
            c = c / max(1, m.ntrees_built())
        c[:, -1] += float(init or 0.0)
    else:
        X, _ = frame.model_matrix(m.info, device=torch.device("cpu"))
        phi = tree_shap(m.forest, X)
        if m.model_category == "Multinomial":
            raise NotImplementedError("contributions for multinomial models are not supported (as in H2O)")
        c = phi[:, 0, :]
        if m.algo == "drf":
            c = c / max(1, m.ntrees_built())
        c[:, -1] += float(init or 0.0)
        c = torch.as_tensor(c)
    if top_n or bottom_n or compare_abs:
        return _sorted_contributions(c, list(m.info.x), top_n, bottom_n, compare_abs)
    names = list(m.info.x) + ["BiasTerm"]
    cols = [Column(n, "real", c[:, i]) for i, n in enumerate(names)]
    return H2OFrame._from_columns(cols)


def _pdp_grid(col, nbins, user_splits, include_na):
    """PartialDependence.extractColValues: categorical -> every level; numeric -> ``nbins`` equally
    spaced values over [min, max] (unit steps for an integer column with fewer distinct values)."""
    if col.type == "enum":
        vals = [float(i) for i in range(len(col.domain))]
        labels = list(col.domain)
    elif user_splits is not None:
        vals = [float(v) for v in user_splits]
        labels = list(vals)
    else:
        v = col.as_float().double()
        v = v[~torch.isnan(v)]
        lo, hi = (float(v.min()), float(v.max())) if v.numel() else (0.0, 0.0)
        nb = int(nbins)
        if col.type == "int" and hi - lo + 1 < nb:
            nb = int(hi - lo + 1)
        delta = 0.0 if nb <= 1 else (hi - lo) / (nb - 1)
        vals = [lo + j * delta for j in range(max(nb, 1))]
        labels = list(vals)
    if include_na:
        vals.append(float("nan"))
        labels.append(".missing(NA)" if col.type == "enum" else float("nan"))
    return vals, labels


def _pd_stats(r, w):
    """(mean, sd, se) of the responses ``r`` [n] float64, weighted by ``w`` [n] float64 when given."""
    if w is None:
        mu = float(r.mean())
        sd = float(r.std()) if r.numel() > 1 else 0.0
        return mu, sd, sd / math.sqrt(max(r.numel(), 1))
    ws = float(w.sum())
    mu = float((w * r).sum() / ws)
    sd = math.sqrt(float((w * (r - mu) ** 2).sum()) / max(ws - 1.0, 1e-300))
    return mu, sd, sd / math.sqrt(max(ws, 1e-300))


PDP_CHUNK_BYTES = 256 << 20     # margins [G, n, K] fp32 of one row chunk of the device path


def _pdp_on_device(m, X) -> bool:
    """The grid kernel path: a CUDA model matrix, a model that scores from forest margins, no ``H2O_PDP_HIP=0``."""
    ok = getattr(m, "scores_from_raw", None)
    return bool(X.is_cuda and os.environ.get("H2O_PDP_HIP", "1") != "0" and ok is not None and ok())


def _grid_response(m, X, off, js, V, pick):
    """Response ``[G, n]`` float64 of the rows of X under every grid tuple (``V[s][g]`` replaces feature
    ``js[s]``): ``Forest.predict_raw_grid`` margins, ``Model.score_from_raw``; the offset broadcasts over tuples."""
    raw = m.forest.predict_raw_grid(X, js, V)
    G, n, K = raw.shape
    P = m.score_from_raw(raw.view(G * n, K), None if off is None else off.repeat(G))
    return pick(P).double().view(G, n)


def _grid_stats(m, X, off, w, js, V, pick):
    """(mean, sd, se) per grid tuple. Rows go in chunks whose margins stay under :data:`PDP_CHUNK_BYTES`; one chunk
    uses :func:`_pd_stats` (the expressions of the re-scoring path) per tuple, several are merged as (weight, mean, M2) in
    fp64 with Chan's update."""
    G, N = int(V.shape[1]), int(X.shape[1])
    step = max(1, PDP_CHUNK_BYTES // max(1, G * m.forest.K * 4))
    if step >= N:
        r = _grid_response(m, X, off, js, V, pick)
        return [_pd_stats(r[g], w) for g in range(G)]
    W = np.zeros(G)
    mu = np.zeros(G)
    M2 = np.zeros(G)
    for r0 in range(0, N, step):
        r = _grid_response(m, X[:, r0:r0 + step], None if off is None else off[r0:r0 + step], js, V, pick)
        if w is None:
            wb = torch.full((G,), float(r.shape[1]), dtype=torch.float64, device=r.device)
            mb = r.mean(1)
            sb = ((r - mb[:, None]) ** 2).sum(1)
        else:
            wc = w[r0:r0 + step]
            wb = wc.sum().expand(G)
            mb = (wc * r).sum(1) / wb
            sb = (wc * (r - mb[:, None]) ** 2).sum(1)
        wb, mb, sb = (t.cpu().numpy() for t in (wb, mb, sb))
        tot = W + wb
        d = mb - mu
        f = np.divide(wb, tot, out=np.zeros(G), where=tot != 0)
        mu = mu + d * f
        M2 = M2 + sb + d * d * W * f
        W = tot
    out = []
    for g in range(G):
        if w is None:
            sd = math.sqrt(M2[g] / (N - 1)) if N > 1 else 0.0
            out.append((float(mu[g]), sd, sd / math.sqrt(max(N, 1))))
        else:
            sd = math.sqrt(M2[g] / max(W[g] - 1.0, 1e-300))
            out.append((float(mu[g]), sd, sd / math.sqrt(max(W[g], 1e-300))))
    return out


def partial_plot(model, frame, cols=None, nbins=20, targets=None, include_na=False, user_splits=None,
                 weight_column=None, row_index=-1, col_pairs_2dpdp=None):
    """Partial dependence (reference ``hex/PartialDependence.java``): for each grid value the column
    (or column pair) is set to it for every row and the frame scored; mean, weighted standard deviation and
    standard error of the response (device path and ``H2O_PDP_HIP``: module docstring). ``targets`` picks classes of a multinomial
    model (one table per column and class), ``row_index`` >= 0 gives an ICE curve of that row.
    Returns ``{name: [row dicts]}`` with name = column, ``"a|b"`` for pairs, ``"col|class"`` with targets."""
    m = getattr(model, "_model", model)
    cols = [] if cols is None else ([cols] if isinstance(cols, str) else list(cols))
    X, off = frame.model_matrix(m.info, device=m.device)
    w = None
    if weight_column is not None and weight_column != -1:
        wn = frame.names[weight_column] if isinstance(weight_column, int) else weight_column
        w = frame._col(wn).as_float().double().to(X.device)
    if row_index is not None and int(row_index) >= 0:
        X = X[:, int(row_index):int(row_index) + 1]
        off = None if off is None else off[int(row_index):int(row_index) + 1]
        w = None if w is None else w[int(row_index):int(row_index) + 1]
    dom = m.info.response_domain
    if m.model_category == "Multinomial":
        if not targets:
            raise ValueError("targets are required for a multinomial model's partial dependence")
        tidx = [(t, dom.index(t)) for t in targets]
    else:
        tidx = [(None, 1 if m.model_category == "Binomial" else 0)]
    user_splits = user_splits or {}

    def pick(P, k):
        if P.dim() == 1:
            return P.double()
        return P[:, k].double() if m.model_category in ("Binomial", "Multinomial") else P[:, 0].double()

    def response(Xg, k):
        return pick(m.score_tensor(Xg, off), k)

    def stats(r):
        return _pd_stats(r, w)

    out = {}
    jobs = [(c,) for c in cols] + [tuple(pr) for pr in (col_pairs_2dpdp or [])]
    for cc in jobs:
        js = [m.info.x.index(c) for c in cc]
        grids = [_pdp_grid(frame._col(c), nbins, user_splits.get(c), include_na) for c in cc]
        for tname, k in tidx:
            rows = []
            if len(cc) == 1:
                combos = [((v,), (lab,)) for v, lab in zip(*grids[0])]
            else:
                combos = [((v1, v2), (l1, l2)) for v1, l1 in zip(*grids[0]) for v2, l2 in zip(*grids[1])]
            on_device = _pdp_on_device(m, X) and len(set(js)) == len(js)
            if on_device:
                V = torch.tensor([[float(v[s]) for v, _ in combos] for s in range(len(js))], dtype=torch.float32,
                                 device=X.device).view(len(js), len(combos))
                done = _grid_stats(m, X, off, w, js, V, lambda P: pick(P, k))
            for ci, (vals, labs) in enumerate(combos):
                if on_device:
                    mu, sd, se = done[ci]
                else:
                    Xg = X.clone()
                    for j, v in zip(js, vals):
                        Xg[j] = float(v)
                    mu, sd, se = stats(response(Xg, k))
                row = dict(value=labs[0], mean_response=mu, stddev_response=sd, std_error_mean_response=se)
                if len(cc) == 2:
                    row["value2"] = labs[1]
                rows.append(row)
            key = "|".join(cc) + (f"|{tname}" if tname is not None else "")
            out[key] = rows
    return out


def _pd_rows(m, X, off, cols, jidx):
    """Partial dependence of the columns ``cols`` evaluated AT each training row's own values."""
    N = X.shape[1]
    if N and _pdp_on_device(m, X) and len(set(jidx)) == len(jidx):
        # the tuples are the rows' own values of the columns; one mean per tuple, reduced as the loop below does
        r = _grid_response(m, X, off, jidx, X[jidx], lambda P: P[:, -1] if P.dim() == 2 else P)
        res = torch.stack([r[i].mean() for i in range(N)])
        return res - res.mean()
    res = torch.zeros(N, dtype=torch.float64, device=X.device)
    vals = X[jidx].T  # [N, len]
    for i in range(N):
        Xg = X.clone()
        for k, j in enumerate(jidx):
            Xg[j] = vals[i, k]
        P = m.score_tensor(Xg, off)
        r = P[:, -1] if P.dim() == 2 else P
        res[i] = r.double().mean()
    return res - res.mean()


def h(model, frame, variables, max_rows=200):
    """Friedman–Popescu H² for the given variables (sample of ``max_rows`` rows, like the reference)."""
    m = getattr(model, "_model", model)
    X, off = frame.model_matrix(m.info, device=m.device)
    if X.shape[1] > max_rows:
        X = X[:, :max_rows]
        off = None if off is None else off[:max_rows]
    jidx = [m.info.x.index(v) for v in variables]
    f_joint = _pd_rows(m, X, off, variables, jidx)
    f_single = [_pd_rows(m, X, off, [v], [j]) for v, j in zip(variables, jidx)]
    num = ((f_joint - sum(f_single)) ** 2).sum()
    den = (f_joint ** 2).sum()
    return float(num / den) if den > 0 else float("nan")


class _FI:
    __slots__ = ("name", "depth", "gain", "cover", "fscore", "wfscore", "expected_gain", "tree_index", "tree_depth",
                 "has_leaf", "leaf_vl", "leaf_cl", "leaf_vr", "leaf_cr", "split_hist")

    def __init__(self, name, depth, gain, cover, proba, tree_depth, tree_index, split_value=None):
        self.name, self.depth, self.gain, self.cover = name, depth, gain, cover
        self.fscore, self.wfscore, self.expected_gain = 1.0, proba, gain * proba
        self.tree_index, self.tree_depth = float(tree_index), float(tree_depth)
        self.has_leaf, self.leaf_vl, self.leaf_cl, self.leaf_vr, self.leaf_cr = False, 0.0, 0.0, 0.0, 0.0
        self.split_hist = {}
        if depth == 0 and split_value is not None:
            self.split_hist[split_value] = 1


def feature_interaction(model, max_interaction_depth=100, max_tree_depth=100, max_deepening=-1):
    """xgbfi-style feature interactions (reference ``hex/FeatureInteractions.java``
    ``collectFeatureInteractions``): every path of split features (up to ``max_interaction_depth``+1
    features) accumulates gain, cover, an F-score, the path-probability weighted F-score and the
    expected gain; leaf statistics and split-value histograms of single features. Returns
    ``{"tables": [per-depth row dicts], "leaf_statistics": [...], "split_value_histograms": {name: {v: n}}}``;
    the legacy list view (``[{interaction, gain, fscore, cover, depth}]``) is under ``"flat"``."""
    m = getattr(model, "_model", model)
    names = m.info.x
    fis: dict = {}
    for ti, t in enumerate(m.forest.trees):
        memo: set = set()

        def split_value(n):
            return None if t.is_cat[n] else float(t.thr[n])

        def collect(n, path, cur_gain, cur_cover, proba, depth, deepening):
            if t.feat[n] < 0 or depth == max_tree_depth:
                return
            path = path + [n]
            cur_gain += float(max(t.gain[n], 0.0))
            cur_cover += float(t.cover[n])
            L, R = int(t.left[n]), int(t.right[n])
            cw = float(t.cover[n]) or 1.0
            ppl, ppr = proba * float(t.cover[L]) / cw, proba * float(t.cover[R]) / cw
            order = sorted(path, key=lambda q: names[int(t.feat[q])])
            name = "|".join(names[int(t.feat[q])] for q in order)
            if depth < max_deepening or max_deepening < 0:
                collect(L, [], 0.0, 0.0, ppl, depth + 1, deepening + 1)
                collect(R, [], 0.0, 0.0, ppr, depth + 1, deepening + 1)
            key = "-".join(str(q) for q in sorted(path))
            fi = fis.get(name)
            if fi is None:
                fis[name] = _FI(name, len(path) - 1, cur_gain, cur_cover, proba, depth, ti, split_value(path[0]))
                memo.add(key)
            else:
                if key in memo:
                    return
                memo.add(key)
                fi.gain += cur_gain
                fi.cover += cur_cover
                fi.fscore += 1
                fi.wfscore += proba
                fi.expected_gain += cur_gain * proba
                fi.tree_depth += depth
                fi.tree_index += ti
                if len(path) == 1 and split_value(path[0]) is not None:
                    sv = split_value(path[0])
                    fi.split_hist[sv] = fi.split_hist.get(sv, 0) + 1
            if len(path) - 1 == max_interaction_depth:
                return
            fi = fis[name]
            if t.feat[L] < 0 and deepening == 0:
                fi.leaf_vl += float(t.value[L])
                fi.leaf_cl += float(t.cover[L])
                fi.has_leaf = True
            if t.feat[R] < 0 and deepening == 0:
                fi.leaf_vr += float(t.value[R])
                fi.leaf_cr += float(t.cover[R])
                fi.has_leaf = True
            # the reference passes the running gain as the cover here as well
            collect(L, path, cur_gain, cur_gain, ppl, depth + 1, deepening)
            collect(R, path, cur_gain, cur_gain, ppr, depth + 1, deepening)

        if t.n_nodes:
            collect(0, [], 0.0, 0.0, 1.0, 0, 0)
    tables = []
    maxd = max((f.depth for f in fis.values()), default=-1)
    for d in range(maxd + 1):
        lst = [f for f in fis.values() if f.depth == d]

        def rank(key):
            srt = sorted(lst, key=lambda f: -key(f))
            return {f.name: i + 1 for i, f in enumerate(srt)}
        rk = [rank(lambda f: f.gain), rank(lambda f: f.fscore), rank(lambda f: f.wfscore),
              rank(lambda f: f.wfscore / f.fscore), rank(lambda f: f.gain / f.fscore), rank(lambda f: f.expected_gain)]
        rows = []
        for f in lst:
            r = [x[f.name] for x in rk]
            rows.append({"Interaction": f.name, "Gain": f.gain, "FScore": f.fscore, "wFScore": f.wfscore,
                         "Average wFScore": f.wfscore / f.fscore, "Average Gain": f.gain / f.fscore,
                         "Expected Gain": f.expected_gain, "Gain Rank": r[0], "FScore Rank": r[1],
                         "wFScore Rank": r[2], "Avg wFScore Rank": r[3], "Avg Gain Rank": r[4],
                         "Expected Gain Rank": r[5], "Average Rank": sum(r) / 6.0,
                         "Average Tree Index": f.tree_index / f.fscore, "Average Tree Depth": f.tree_depth / f.fscore})
        tables.append(rows)
    leaf = [{"Interaction": f.name, "Sum Leaf Values Left": f.leaf_vl, "Sum Leaf Values Right": f.leaf_vr,
             "Sum Leaf Covers Left": f.leaf_cl, "Sum Leaf Covers Right": f.leaf_cr} for f in fis.values() if f.has_leaf]
    hists = {f.name: dict(sorted(f.split_hist.items())) for f in fis.values() if f.depth == 0}
    flat = sorted(({"interaction": f.name, "gain": f.gain, "fscore": f.fscore, "cover": f.cover, "depth": f.depth + 1}
                   for f in fis.values()), key=lambda r: -r["gain"])
    return {"tables": tables, "leaf_statistics": leaf, "split_value_histograms": hists, "flat": flat}


def explain(model, frame, columns=None, top_n_features=5):
    """Compact explanation bundle (the plotting-free part of ``h2o.explain``)."""
    m = getattr(model, "_model", model)
    vi = m.varimp() or []
    cols = columns or [r[0] for r in vi[:top_n_features]]
    res = dict(varimp=vi, pdp=partial_plot(m, frame, cols))
    if hasattr(m, "forest") and m.forest is not None and m.model_category in ("Binomial", "Regression"):
        sub = frame._rows(torch.arange(min(frame.nrows, 1000)))
        c = predict_contributions(m, sub).as_data_frame()
        res["shap_summary"] = c.abs().mean().sort_values(ascending=False).to_dict()
    return res

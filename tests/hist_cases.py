"""Shared helpers of the level-histogram tests (test_hist_levels_paths.py on the CPU, test_hist_levels_gpu.py on
the device): synthetic inputs, the case table, an fp64 reference of every node histogram of a built tree, and the
error bound of the tree engine's fixed-point histograms (csrc/tree_kernels.hip). Nothing here needs a GPU.

Inputs are made as uint8 bins directly (no float X, no fit_binning), so the row stride, every column's cardinality,
the NA rows and the same-address collisions are chosen here. Column layout of every synthetic case (F >= 8):

    0: 200 bins, carries signal        1: 3 bins  (4 bin replicas when no row is NA)
    2: 60 bins  (4 replicas)           3: 100 bins (2 replicas)
    4: 255 bins (no replica)           5: categorical, 7 levels (level 6 rare: a handful of rows)
    6: constant (every row in bin 0: the most same-address atomics, the largest count field of a packed window)
    F-1: 200 bins, carries signal (the last word of the row)          the rest: 200 bins of noise

The bound ``tol`` (per histogram entry of a BUILT node; n rows in the entry, S = sum |v_i| over them, M = max |v|
of the plane over all N rows, which is what k_amax / k_qscale see), from the kernels' arithmetic:

    mode                          w plane                                    wY plane
    unpacked (packed=False)       n M_w 2^-40 + 2 2^-24 S_w                  n M 2^-40 + 2 2^-24 S
    packed count (unit or mask)   exact                                      n M 2^-30 + 2 2^-24 S
    packed=2 (FPACK)              n PACK_MAX M_w / (2 0.99 2^32) + 2 2^-24 S_w    n PACK_MAX M / (2 0.99 2^31) + 2 2^-24 S

The first term is the conversion to fixed point (one truncation, FPACK one rounding, per row, in units of 1 / scale;
k_qscale caps every scale at 2^127, and the bound uses the capped scale), the second the fp32 product v * (float)scale
(the product and the scale are each rounded once). Added on top: 2^-50 S for the fp64 sums of the reference and of
k_hist_reduce; with fp32 block partials (H2O_PARTIAL_F32=1) (1 + windows per block) 2^-24 S, the count plane staying
exact while a block's count is below 2^24. A node whose histogram is DERIVED (parent - built sibling, k_hist_reduce)
gets tol(parent entry) + tol(built sibling entry), recursively up the chain.

nayy[f] and the node's wyy are fp32 sums in scheduling order: (k + e) 2^-24 sum(yy), k the rows contributing, plus the
fp32-partial term. e = 6 where rows carry float weights: the kernel evaluates yy = b * b * rcp(a) (v_rcp_f32, 1 ulp)
and the reference float32(b * b / a), which differ by up to 6 2^-24 yy per row; e = 0 where every weight is 0 or 1
(both are exactly b * b). This bound is LOOSE: it only catches gross errors (a dropped NA tally, a missing window).
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from llama_github_io_amd.ops import tree as T

TILE = 2048            # rows per work tile (csrc: TILE)
PACK_MAX = 63488       # rows per packed flush window (csrc: PACK_MAX, 31 tiles)
QS_CAP = 2.0 ** 127    # k_qscale's cap of every fixed-point scale
U24 = 2.0 ** -24
PLUS_M = 0.5           # |wY| of the all-equal flush-window cases

MODES = ("unpacked", "count", "unit", "fpack")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    N: int = 20000
    F: int = 28
    stride: int = 32
    mode: str = "unpacked"        # unpacked | count (0/1 mask) | unit | fpack (packed=2, float hessians)
    na: bool = False
    grid: int = 256
    min_w: float = 10.0
    wy: str = "uniform"           # uniform | narrow | plus | minus | range | tiny
    env: tuple = ()               # ((name, value), ...) set before the builder is constructed
    stress: bool = False          # one of the two named quantisation stress cases (exempt from non-vacuity)
    kind: str = "synthetic"       # synthetic | root16 (wide-bin layout from fit_binning, fine-plane root pass)
    depths: tuple = (1, 2, 3, 4, 5)
    seed: int = 0

    @property
    def packed(self):
        return {"unpacked": False, "count": True, "unit": True, "fpack": 2}[self.mode]

    @property
    def unit(self):
        return self.mode == "unit"

    @property
    def pf32(self):
        return dict(self.env).get("H2O_PARTIAL_F32") == "1"


def _cases():
    c = []
    # modes x NA (N = 20,000, F = 28, stride 32): NONA kernels and 4x / 2x / 1x bin replicas without NA rows, the
    # per-word NA test and the NA tail with them
    for mode in MODES:
        for na in (False, True):
            c.append(Case(f"mode-{mode}-{'na' if na else 'nona'}", mode=mode, na=na))
    # flush windows (N = 200,000 = 98 tiles): grid 1 -> one block, four packed windows; grid 3 -> 33 tiles per block,
    # two windows. Every row's wY is +M resp. -M (the constant column's entry takes the whole window: the largest
    # low field; all-negative values borrow from the count field in unpack). With one response value the SE modes
    # cannot split, so the count-mode trees are the root alone; FPACK (Newton gain, hessians that follow column 4)
    # grows a tree. 'win-*-narrow' runs the same windows through a real tree: the filtered level 1 counts its
    # PARENT's tiles into the window (since += r1 - r0)
    for mode in ("count", "fpack"):
        for grid in (1, 3):
            c.append(Case(f"win-{mode}-g{grid}-plus", N=200000, mode=mode, grid=grid, wy="plus"))
            c.append(Case(f"win-{mode}-g{grid}-minus", N=200000, mode=mode, grid=grid, wy="minus", stress=True))
        c.append(Case(f"win-{mode}-g3-narrow", N=200000, mode=mode, grid=3, wy="narrow"))
    # dynamic range: one row of |wY| = 1e6 among +-U(0.05, 0.95) 1e-3 (packed: most rows truncate to 0)
    c.append(Case("range-unpacked", mode="unpacked", wy="range", stress=True))
    c.append(Case("range-unit", mode="unit", wy="range", stress=True))
    # small shapes (0/1 weights at N = 1 and 7: see the yy note in the module docstring) and ragged nodes
    c.append(Case("small-1", N=1, mode="unit"))
    c.append(Case("small-7", N=7, mode="count"))
    c.append(Case("small-2049-unpacked", N=2049, mode="unpacked", na=True))
    c.append(Case("small-2049-unit", N=2049, mode="unit"))
    c.append(Case("ragged-minw1-unpacked", mode="unpacked", min_w=1.0, na=True))
    c.append(Case("ragged-minw1-count", mode="count", min_w=1.0))
    c.append(Case("grid3-unpacked", mode="unpacked", grid=3, na=True))
    c.append(Case("grid3-unit", mode="unit", grid=3))
    # layouts: row strides 8 / 12 (generic byte route), 16, 32, 48 (never made by fit_binning), 64 row-major,
    # planar with 2 and 3 planes (the last one holds 6 columns)
    for mode in ("unit", "unpacked"):
        for name, F, stride, env in (("s8", 8, 8, ()), ("s12", 11, 12, ()), ("s16", 14, 16, ()), ("s32", 28, 32, ()),
                                     ("s48", 44, 48, ()), ("s64-rowmajor", 50, 64, (("H2O_BINS_ROWMAJOR", "1"),)),
                                     ("planar2", 40, 64, ()), ("planar3", 70, 96, ())):
            c.append(Case(f"layout-{name}-{mode}", F=F, stride=stride, mode=mode, env=env, na=(mode == "unpacked")))
    # fp32 block partials (|wY| from +-U(0.5, 0.95): with 200,000 rows in the constant column's entry the fp32 terms
    # of the bound would pass half of 0.05)
    for mode in ("count", "unpacked"):
        c.append(Case(f"pf32-{mode}", N=200000, mode=mode, grid=3, wy="narrow", env=(("H2O_PARTIAL_F32", "1"),)))
    # fine-plane root pass (k_hist_root16 rebuilds the engine columns in its flush): the root alone
    for mode in ("unit", "count"):
        c.append(Case(f"root16-{mode}", N=30000, F=0, stride=0, mode=mode, kind="root16", depths=(1,)))
    # scale overflow: max |wY|, |num|, |den| ~ 1e-30, where 2^40 / max is past FLT_MAX
    c.append(Case("tiny-unpacked", N=2049, mode="unpacked", wy="tiny"))
    c.append(Case("tiny-unit", N=2049, mode="unit", wy="tiny"))
    return c


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
ORDINARY = [c for c in CASES if not c.stress]


def min_levels(c: Case) -> int:
    """Levels the case's depth-5 tree must have for the case to reach what it is for: all 5 for ordinary inputs;
    the all-equal responses split only under FPACK's Newton gain; tiny shapes, the scale-overflow and the
    dynamic-range inputs promise the root alone."""
    if c.kind != "synthetic" or c.N < 2049 or c.wy in ("tiny", "range"):
        return 1
    if c.wy in ("plus", "minus"):
        return 2 if c.mode == "fpack" else 1
    return 5


def case(name: str) -> Case:
    return CASES[CASE_IDS.index(name)]


# ---------------------------------------------------------------------------------------------------------------
# inputs
@dataclasses.dataclass
class Inputs:
    bins: torch.Tensor            # [N, stride] uint8, row-major, CPU
    F: int
    nbins_f: np.ndarray
    iscat_f: np.ndarray
    aux: torch.Tensor             # [N, 4] float32: w, wY, gamma numerator, gamma denominator
    params: T.SplitParams
    groups: tuple | None = None   # (vmap, n_low, n_mid) of the wide-bin layout (set_feature_groups)
    planar_input: bool = False    # hand the builder planar bins (apply_binning(planar=True) layout)

    def builder_bins(self, device):
        b = self.bins.to(device)
        if self.planar_input:
            b = b.view(b.shape[0], b.shape[1] // 32, 32).permute(1, 0, 2).contiguous()
        return b


def columns(F: int):
    """(nbins_f, iscat_f) of the synthetic column layout (module docstring)."""
    assert F >= 8
    nb = np.full(F, 200, dtype=np.int32)
    ic = np.zeros(F, dtype=np.int32)
    nb[1], nb[2], nb[3], nb[4], nb[5], nb[6] = 3, 60, 100, 255, 7, 1
    ic[5] = 1
    return nb, ic


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _synthetic(c: Case) -> Inputs:
    rng = np.random.default_rng(1000 + c.seed + 7 * CASE_IDS.index(c.name))
    N, F = c.N, c.F
    nb, ic = columns(F)
    b = np.zeros((N, c.stride), dtype=np.uint8)
    for f in range(F):
        b[:, f] = rng.integers(0, 6 if f == 5 and N >= 100 else nb[f], N)
    rare = rng.choice(N, max(1, N // 4000), replace=False) if N >= 100 else np.zeros(0, np.int64)
    b[rare, 5] = 6
    if c.na:
        r = max(1, N // 50)
        b[:r, 3] = T.NA_BIN
        b[r:2 * r, 5] = T.NA_BIN
        b[2 * r:3 * r, F - 1] = T.NA_BIN
        b[3 * r:3 * r + r // 4 + 1, 0] = T.NA_BIN
    logit = (1.5 * (b[:, 0].astype(np.float64) - 100) / 60 - 1.0 * (b[:, F - 1] > 120) + 0.8 * (b[:, 5] == 2)
             + 0.6 * (b[:, 3] == T.NA_BIN) - 0.5 * (b[:, 2] > 30))
    sign = np.where(rng.random(N) < _sigmoid(logit), 1.0, -1.0)
    lo = 0.5 if c.wy == "narrow" else 0.05
    z = sign * rng.uniform(lo, 0.95, N)
    z[rare] = 0.95
    num = np.where(rng.random(N) < 0.5, 1.0, -1.0) * rng.uniform(0.05, 0.95, N)
    den = rng.uniform(0.05, 0.95, N)
    if c.wy == "plus":
        z[:] = PLUS_M
    elif c.wy == "minus":
        z[:] = -PLUS_M
    elif c.wy == "range":
        z *= 1e-3
        z[N // 2] = 1e6
    elif c.wy == "tiny":
        z *= 1e-30
        num *= 1e-30
        den *= 1e-30
    if c.mode == "unpacked":
        w = rng.uniform(0.5, 1.5, N)
    elif c.mode == "count":
        w = (rng.random(N) < 0.7).astype(np.float64)
        if c.wy == "range":
            w[N // 2] = 1.0
        if c.wy in ("plus", "minus"):      # every row counted: the fullest count field a window can hold
            w[:] = 1.0
        z = z * w
    elif c.mode == "unit":
        w = np.ones(N)
    else:       # float hessians in (0, 0.25] that follow column 4 (so that equal gradients still split)
        w = 0.25 * (0.15 + 0.85 * _sigmoid((b[:, 4].astype(np.float64) - 127) / 50)) * (1.0 - 0.3 * rng.random(N))
    aux = torch.from_numpy(np.stack([w, z, num, den], 1).astype(np.float32)).contiguous()
    if c.mode == "fpack":
        p = T.SplitParams(min_w=1.0, lam=1.0, mode=T.MODE_NEWTON)
    else:
        p = T.SplitParams(min_w=c.min_w)
    return Inputs(torch.from_numpy(b), F, nb, ic, aux, p)


def _root16(c: Case) -> Inputs:
    """The setup of test_gpu_root16_matches_reference: 10 features binned to 1016 fine bins (several engine columns
    per numeric feature), planar bins, UniformAdaptive lattices with node ranges."""
    from llama_github_io_amd.ops.binning import apply_binning, fit_binning
    import test_tree_engine as tte
    X, y, info = tte._data(N=c.N, F=10, cat=True, seed=11)
    b = fit_binning(X, info.iscat, info.nlevels, max_bins=1016)
    assert b.vmap is not None and b.stride >= 64 and b.n_low == X.shape[0]
    bins = apply_binning(b, X)
    rng = np.random.default_rng(5)
    g = (y.numpy() - 0.5) * 2 * rng.uniform(0.05, 0.95, c.N)
    w = np.ones(c.N) if c.mode == "unit" else (rng.random(c.N) < 0.8).astype(np.float64)
    aux = torch.from_numpy(np.stack([w, w * g, w * g, w], 1).astype(np.float32)).contiguous()
    p = T.SplitParams(min_w=10, adapt_nbins=20, adapt_top=1024, edges=tte._edge_tab(b), vrange=tte._vr(b, X))
    return Inputs(bins, int(b.F), np.asarray(b.nbins, dtype=np.int32), np.asarray(b.iscat, dtype=np.int32), aux, p,
                  groups=(b.vmap, b.n_low, b.n_mid), planar_input=True)


@functools.lru_cache(maxsize=4)
def make_inputs(c: Case) -> Inputs:
    return _root16(c) if c.kind == "root16" else _synthetic(c)


def ref_builder(c: Case, inp: Inputs, depth: int) -> T.RefTreeBuilder:
    ref = T.RefTreeBuilder(inp.bins, inp.F, inp.nbins_f, inp.iscat_f, None, depth, inp.params)
    if inp.groups is not None:
        ref.set_feature_groups(*inp.groups)
    return ref


def leaf_fn(ls):
    return (ls[:, 0] / ls[:, 1].abs().clamp(min=1e-300)).float()


# ---------------------------------------------------------------------------------------------------------------
# the tree's row sets and plan
def node_rows(tl: T.TreeLevels, bins):
    """Per level the row index set of every node (list of lists of int64 arrays), walking the decoded tree's own
    ``decs`` / ``child_l`` / ``child_r`` with dec_go_left_np, and the leaf of every row. A child >= 0 is the node index
    at the next level, a negative one the leaf -1 - child."""
    b = bins.numpy() if isinstance(bins, torch.Tensor) else np.asarray(bins)
    N = b.shape[0]
    levels = [[np.arange(N, dtype=np.int64)]]
    leaf = np.full(N, -1, dtype=np.int64)
    for d in range(len(tl.decs)):
        dec, cl, cr = tl.decs[d], tl.child_l[d], tl.child_r[d]
        assert len(dec) == len(levels[d]), (d, len(dec), len(levels[d]))
        nxt = {}
        for i, rows in enumerate(levels[d]):
            dd = dec[i]
            if dd["feat"] < 0:
                leaf[rows] = -1 - int(cl[i])
                continue
            f = int(dd["feat"])
            col = b[rows, f:f + 4] if int(dd["is_cat"]) == T.GROUP_CAT else b[rows, f]
            gl = T.dec_go_left_np(dd, col.astype(np.int64))
            for ch, r in ((int(cl[i]), rows[gl]), (int(cr[i]), rows[~gl])):
                if ch >= 0:
                    assert ch not in nxt
                    nxt[ch] = r
                else:
                    leaf[r] = -1 - ch
        if not nxt or d + 1 >= len(tl.decs):
            assert not nxt or d + 1 < len(tl.decs), "children past the last decoded level"
            break
        assert sorted(nxt) == list(range(len(nxt)))
        levels.append([nxt[k] for k in range(len(nxt))])
    return levels, leaf


PLAN_DT = np.dtype([("parent", "<i4"), ("build", "<i4"), ("sib", "<i4"), ("dir", "<i4")])


def plan_nodes(tl: T.TreeLevels):
    """Per level (parent, build, sib, dir) of every node as k_plan writes them: of two continuing children the one
    with the smaller weight is histogrammed (the left one on a tie), the other derived as parent - sibling; an only
    continuing child is built."""
    out = [np.array([(-1, 1, -1, 0)], dtype=PLAN_DT)]
    for d in range(len(tl.decs)):
        dec, cl, cr = tl.decs[d], tl.child_l[d], tl.child_r[d]
        nn = int((cl >= 0).sum() + (cr >= 0).sum())
        if nn == 0:
            break
        arr = np.zeros(nn, dtype=PLAN_DT)
        for i in range(len(dec)):
            if dec[i]["feat"] < 0:
                continue
            li, ri = int(cl[i]), int(cr[i])
            if li >= 0 and ri >= 0:
                bl = bool(dec[i]["wl"] <= dec[i]["wr"])
                arr[li] = (i, int(bl), ri, 0)
                arr[ri] = (i, int(not bl), li, 1)
            elif li >= 0:
                arr[li] = (i, 1, -1, 0)
            elif ri >= 0:
                arr[ri] = (i, 1, -1, 1)
        out.append(arr)
    return out


# ---------------------------------------------------------------------------------------------------------------
# fp64 reference of a node histogram
def _bincount_feat(bf, wts):
    """[256, F] sums of ``wts`` (None: counts) by bin, 16 features per bincount (RefTreeBuilder._hist's order)."""
    F = bf.shape[1]
    out = np.zeros((256, F))
    for f0 in range(0, F, 16):
        f1 = min(F, f0 + 16)
        k = f1 - f0
        key = (bf[:, f0:f1] + 256 * np.arange(k)[None, :]).T.reshape(-1)
        out[:, f0:f1] = np.bincount(key, weights=None if wts is None else np.tile(wts, k),
                                    minlength=256 * k).reshape(k, 256).T
    return out


def _yy(aux, rows):
    a32, b32 = aux[rows, 0], aux[rows, 1]
    with np.errstate(under="ignore"):
        return np.where(a32 > 0, (b32 * b32 / np.where(a32 > 0, a32, 1)).astype(np.float32), 0).astype(np.float64)


def _np_aux(aux):
    return aux.numpy() if isinstance(aux, torch.Tensor) else np.asarray(aux)


def _np_bins(bins):
    return bins.numpy() if isinstance(bins, torch.Tensor) else np.asarray(bins)


def ref_node_hist(rows, bins, aux, F, shift=None):
    """fp64 histogram of the rows of one node: ``h[256][F][2]`` = (w, wY) by (bin, feature), ``nayy[F]`` (yy of the
    rows whose feature is NA) and ``wyy``; yy exactly as RefTreeBuilder._hist (the float32 ``b * b / a`` where a > 0).
    ``shift = (row, f)`` makes a deliberately WRONG reference: that row counts in the neighbouring bin of feature f."""
    b, a = _np_bins(bins), _np_aux(aux)
    bf = b[rows, :F].astype(np.int64)
    if shift is not None:
        r, f = shift
        at = np.nonzero(rows == r)[0]
        assert at.size == 1
        v = bf[at[0], f]
        bf[at[0], f] = v + 1 if v < 254 else v - 1
    h = np.zeros((256, F, 2))
    h[:, :, 0] = _bincount_feat(bf, a[rows, 0].astype(np.float64))
    h[:, :, 1] = _bincount_feat(bf, a[rows, 1].astype(np.float64))
    yy = _yy(a, rows)
    nayy = np.array([yy[bf[:, f] == T.NA_BIN].sum() for f in range(F)])
    return h, nayy, yy.sum()


def ref_node_abs(rows, bins, aux, F):
    """What the bound needs of a node: per entry the row count n[256][F] and the sums of |w|, |wY|; per feature the
    number of NA rows; the number of rows with w > 0 (the rows whose yy is not 0 by definition)."""
    b, a = _np_bins(bins), _np_aux(aux)
    bf = b[rows, :F].astype(np.int64)
    n = _bincount_feat(bf, None)
    sw = _bincount_feat(bf, np.abs(a[rows, 0].astype(np.float64)))
    sy = _bincount_feat(bf, np.abs(a[rows, 1].astype(np.float64)))
    return n, sw, sy, n[T.NA_BIN].copy(), float((a[rows, 0] > 0).sum())


def min_abs_wy(rows, bins, aux, F):
    """[256][F]: the smallest non-zero |wY| of a row in the entry (inf where there is none)."""
    b, a = _np_bins(bins), _np_aux(aux)
    ay = np.abs(a[rows, 1].astype(np.float64))
    keep = ay > 0
    order = np.argsort(-ay[keep], kind="stable")         # descending: the smallest is assigned last
    r, v = rows[keep][order], ay[keep][order]
    out = np.full((256, F), np.inf)
    for f in range(F):
        out[b[r, f].astype(np.int64), f] = v
    return out


# ---------------------------------------------------------------------------------------------------------------
# the bound
def windows_per_block(N: int, grid: int, packed) -> int:
    """Flush windows of the fullest histogram block (the root's: no level gives a block more rows)."""
    if not packed:
        return 1
    tiles = (N + TILE - 1) // TILE
    per = (tiles + grid - 1) // grid
    return max(1, math.ceil(min(N, per * TILE) / PACK_MAX))


def quantum(mode: str, plane: int, M: float) -> float:
    """Largest error of one row's conversion to fixed point, in the plane's units (plane 0 = w, 1 = wY)."""
    if not (M > 0):
        return 0.0
    if mode == "unpacked":
        return 1.0 / min(2.0 ** 40 / M, QS_CAP)
    if mode in ("count", "unit"):
        return 0.0 if plane == 0 else 1.0 / min(2.0 ** 30 / M, QS_CAP)
    assert mode == "fpack"
    return 0.5 / min(0.99 * 2.0 ** (32 - plane) / (PACK_MAX * M), QS_CAP)


def tol(mode: str, plane: int, n, S, M: float, pf32_windows: int = 0):
    """Bound of |entry - fp64 reference| for an entry of a built node (module docstring). n, S: arrays or scalars."""
    n, S = np.asarray(n, dtype=np.float64), np.asarray(S, dtype=np.float64)
    if mode in ("count", "unit") and plane == 0:
        return np.zeros_like(S)
    t = n * quantum(mode, plane, M) + 2 * U24 * S + 2.0 ** -50 * S
    if pf32_windows:
        t = t + (1 + pf32_windows) * U24 * S
    return t


def tol_yy(k, syy, float_w: bool, pf32_windows: int = 0):
    k, syy = np.asarray(k, dtype=np.float64), np.asarray(syy, dtype=np.float64)
    t = (k + (6.0 if float_w else 0.0)) * U24 * syy + 2.0 ** -50 * syy
    if pf32_windows:
        t = t + (1 + pf32_windows) * U24 * syy
    return t


def leaf_tol(N: int, n, S, M: float):
    """k_leaf_assign's fixed-point leaf sums: n M 2^-lb + 2 2^-24 S, lb = max(8, 61 - N.bit_length())."""
    lb = max(8, 61 - int(N).bit_length())
    q = 1.0 / min(2.0 ** lb / M, QS_CAP) if M > 0 else 0.0
    S = np.asarray(S, dtype=np.float64)
    return np.asarray(n, dtype=np.float64) * q + 2 * U24 * S + 2.0 ** -50 * S


class TreeRef:
    """References and bounds of the nodes of a case's trees; nodes are cached by their row set, so the depth-1 .. 5
    builds of one case (the same tree, one level deeper each time) share them."""

    def __init__(self, c: Case, inp: Inputs):
        self.c, self.inp = c, inp
        a = inp.aux.numpy()
        self.Mw = float(np.abs(a[:, 0]).max())
        self.My = float(np.abs(a[:, 1]).max())
        self.win = windows_per_block(c.N, c.grid, c.packed) if c.pf32 else 0
        self.float_w = c.mode in ("unpacked", "fpack")
        self._cache = {}

    def node(self, rows):
        key = (rows.size, hash(rows.tobytes()))
        if key not in self._cache:
            inp, c = self.inp, self.c
            h, nayy, wyy = ref_node_hist(rows, inp.bins, inp.aux, inp.F)
            n, sw, sy, nak, kpos = ref_node_abs(rows, inp.bins, inp.aux, inp.F)
            t = dict(w=tol(c.mode, 0, n, sw, self.Mw, self.win), wy=tol(c.mode, 1, n, sy, self.My, self.win),
                     nayy=tol_yy(nak, nayy, self.float_w, self.win), wyy=tol_yy(kpos, wyy, self.float_w, self.win))
            self._cache[key] = dict(h=h, nayy=nayy, wyy=wyy, n=n, tol=t)
        return self._cache[key]

    def level_tols(self, levels, plan):
        """tols[d][i]: the bound of node i of level d — its own when built, else parent + built sibling."""
        tols = []
        for d, rows_d in enumerate(levels):
            cur = []
            for i, rows in enumerate(rows_d):
                pl = plan[d][i]
                if pl["build"]:
                    cur.append(self.node(rows)["tol"])
                else:
                    cur.append(None)
            for i in range(len(rows_d)):
                if cur[i] is None:
                    pl = plan[d][i]
                    sib, par = int(pl["sib"]), int(pl["parent"])
                    assert sib >= 0 and plan[d][sib]["build"] and int(plan[d][sib]["parent"]) == par
                    tp, ts = tols[d - 1][par], cur[sib]
                    cur[i] = {k: tp[k] + ts[k] for k in tp}
            tols.append(cur)
        return tols


def split_slot(slot: np.ndarray, F: int):
    """A node histogram slot (flush_partial / k_split_find layout) -> h[256][F][2], nayy[F], wyy."""
    return slot[:512 * F].reshape(256, F, 2), slot[512 * F:512 * F + F], float(slot[512 * F + F])


def compare_node(got, ref, tl, nbins_f, no_na: bool):
    """``got`` = (h, nayy, wyy) of the engine, ``ref`` = the node's reference dict, ``tl`` its bound.
    Returns (ratios, problems): the worst err / tol per plane ('w', 'wy', 'nayy', 'wyy'; inf where the bound is 0
    and the entry differs) with the place of the worst entry, and the violations as text."""
    gh, gn, gw = got
    F = gh.shape[1]
    ratios, bad = {}, []

    def ratio(err, t):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(err == 0, 0.0, np.where(t > 0, err / t, np.inf))
    for r, name in ((0, "w"), (1, "wy")):
        err = np.abs(gh[:, :, r] - ref["h"][:, :, r])
        q = ratio(err, tl[name])
        q = np.where(np.isnan(gh[:, :, r]), np.inf, q)
        t, f = np.unravel_index(int(np.argmax(q)), q.shape)
        ratios[name] = float(q[t, f])
        if not q[t, f] <= 1.0:
            bad.append(f"plane {name} feature {f} bin {t}: got {gh[t, f, r]!r} want {ref['h'][t, f, r]!r} "
                       f"tol {tl[name][t, f]!r} ({int((q > 1).sum())} entries over)")
    q = ratio(np.abs(gn - ref["nayy"]), tl["nayy"])
    q = np.where(np.isnan(gn), np.inf, q)
    f = int(np.argmax(q))
    ratios["nayy"] = float(q[f])
    if not q[f] <= 1.0:
        bad.append(f"nayy feature {f}: got {gn[f]!r} want {ref['nayy'][f]!r} tol {tl['nayy'][f]!r}")
    q = float(ratio(np.abs(gw - ref["wyy"]), tl["wyy"])) if gw == gw else np.inf
    ratios["wyy"] = q
    if not q <= 1.0:
        bad.append(f"wyy: got {gw!r} want {ref['wyy']!r} tol {float(tl['wyy'])!r}")
    # exact zeros: data bins at or past a column's bin count; the NA bin and the NA tail when no row is NA
    for f in range(F):
        nb = min(int(nbins_f[f]), T.NA_BIN)
        if np.any(gh[nb:T.NA_BIN, f, :] != 0):
            bad.append(f"feature {f}: non-zero entry in a bin >= nbins {nb}")
    if no_na and (np.any(gh[T.NA_BIN] != 0) or np.any(gn != 0)):
        bad.append("no NA row, but the NA bin or nayy is not exactly 0")
    return ratios, bad


def gpu_level_hist(gb, d: int) -> np.ndarray:
    """Level d's node histograms of a GpuTreeBuilder as [node][slot] doubles on the host. After ``build`` with
    max_depth D only levels D - 1 and D - 2 survive in the two ping-pong buffers. In a single process k_split_find
    only reads the slots; a sibling's slot was written by k_hist_reduce as parent - built child."""
    torch.cuda.synchronize()
    return gb.hist[d & 1].view(-1, gb.slot).cpu().numpy()

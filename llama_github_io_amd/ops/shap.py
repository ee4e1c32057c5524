"""Path-decomposed TreeSHAP (formulation: Mitchell, Frank, Holmes, "GPUTreeShap: massively parallel
exact calculation of SHAP scores for tree ensembles", 2020; recursion being replaced: ``csrc/treeshap.cpp``).

:func:`forest_paths` turns a :class:`~.forest.Forest` into a flat table of root-to-leaf paths, once per
forest on the host. A path is one leaf and has one element per DISTINCT feature on the way down:

* ``zero_fraction``: product of ``cover[child] / cover[node]`` over the path's splits on that feature;
* the merged condition that tells whether a row follows the path at that feature: numeric splits
  intersect to an interval ``lo <= x < hi`` (``x >= thr`` goes right, so ``lo`` is the largest threshold
  passed on the right and ``hi`` the smallest passed on the left; an element with no left split has no
  upper bound and accepts ``+inf``), categorical splits AND their level bitsets (complemented within the
  split's ``cat_nbits`` when the path goes right; codes past a split's ``cat_nbits`` take that split's NA
  direction);
* ``na_ok``: NaN (or a code < 0 / >= the merged width) follows the path only if every split on the
  feature sends NA toward it.

Element 0 of every path is the dummy root (``feature = -1``, both fractions 1); a single-leaf tree is a
path of that element alone. The bias column is ``sum(value * prod(zero_fraction))`` per class, in fp64.

:func:`path_shap` evaluates the table: CUDA tensors run the HIP kernel ``k_tree_shap``
(``csrc/shap_kernels.hip``), CPU tensors a vectorised PyTorch evaluation of the same table (the CPU
suite's check of the decomposition). A path needs one lane per element, so forests whose longest path has
more than :data:`MAX_PATH_LEN` (64) elements are not evaluated here: :func:`path_shap` raises for them and
``explain.tree_shap_device`` keeps them on the CPU recursion.

:func:`path_shap_baseline` evaluates the same table for baseline (interventional) SHAP: the Shapley values of
the game ``v(S) = f(x_S, b_~S)`` of a row ``x`` against a background row ``b``. Per path, with the elements
whose condition holds for ``x`` only (``a`` of them) and for ``b`` only (``c`` of them): nothing if some element
holds for neither row; else a feature of the first set gets ``+value * T[a][c]``, one of the second
``-value * T[c][a]``, and the bias cell gets ``value`` when ``a == 0`` (``b`` reaches the leaf), with
``T[p][q] = (p-1)! q! / (p+q)!``. CUDA tensors run ``k_shap_baseline`` (``csrc/shap_baseline_kernels.hip``), CPU
tensors a vectorised fp64 PyTorch evaluation with no lane limit.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

from . import _native as nat

c_int, c_ll, c_void_p = nat.c_int, nat.c_ll, nat.c_void_p

PATH_ARRAYS = ("feat", "zf", "lo", "hi", "flags", "cat_off", "cat_nbits", "cat_bits", "len", "value", "cls")


class PathView(ctypes.Structure):
    """``PathView`` of ``csrc/path_table.h``: the device pointers of a :class:`PathTable`'s arrays."""
    _fields_ = [(n, c_void_p) for n in PATH_ARRAYS] + [("P", c_int), ("G", c_int)]


_view_p = ctypes.POINTER(PathView)
nat.register_hip_signatures({
    # X, N, F, K, paths, rounds, out, stream
    "h2o_tree_shap": [c_void_p, c_ll, c_int, c_int, _view_p, c_int, c_void_p, c_void_p],
    # X, N, Bg, B, F, K, paths, T, rounds, per_reference, out, stream
    "h2o_tree_shap_baseline": [c_void_p, c_ll, c_void_p, c_ll, c_int, c_int, _view_p, c_void_p, c_int, c_int, c_void_p,
                               c_void_p],
    "h2o_shap_tiles": [c_void_p],               # int32 [3]: ROW_TILE, X_TILE_BYTES, PHI_TILE_BYTES as compiled
    "h2o_shap_baseline_tiles": [c_void_p],      # int32 [4]: BASELINE_ROW_TILE, BG_TILE, BASELINE_X / PHI_TILE_BYTES
})

MAX_PATH_LEN = 64       # one wave lane per path element
ROW_TILE = 64           # rows per block of k_tree_shap (SHAP_R in csrc/shap_kernels.hip)
X_TILE_BYTES = 16384    # the block stages X in LDS when F * ROW_TILE * 4 fits (SHAP_X_BYTES)
PHI_TILE_BYTES = 32768  # ... and accumulates phi in LDS when ROW_TILE * K * (F+1) * 8 fits (SHAP_PHI_BYTES)
BASELINE_ROW_TILE = 32        # rows per block of k_shap_baseline (SB_R in csrc/shap_baseline_kernels.hip)
BG_TILE = 32                  # ... and background rows per block (SB_BT)
BASELINE_X_TILE_BYTES = 12288    # X and background staged in LDS when F * (row tile + BG_TILE) * 4 fits (SB_X_BYTES)
BASELINE_PHI_TILE_BYTES = 16384  # summed mode: phi in LDS when row tile * K * (F+1) * 8 fits (SB_PHI_BYTES)

NA_OK, IS_CAT, HAS_HI = 1, 2, 4


@dataclass
class PathTable:
    """Paths padded to ``G`` elements, row-major ``[P, G]`` element arrays and ``[P]`` path arrays."""
    G: int
    max_len: int
    n_features: int                 # 1 + largest feature index used by any split
    K: int
    feat: np.ndarray                # int32 [P, G], -1 = dummy root / padding
    zf: np.ndarray                  # float64 [P, G]
    lo: np.ndarray                  # float32 [P, G]
    hi: np.ndarray                  # float32 [P, G]
    flags: np.ndarray               # int32 [P, G]: NA_OK | IS_CAT | HAS_HI
    cat_off: np.ndarray             # int32 [P, G] word offset into cat_bits
    cat_nbits: np.ndarray           # int32 [P, G]
    cat_bits: np.ndarray            # uint32 words
    len: np.ndarray                 # int32 [P] elements of the path (dummy included)
    value: np.ndarray               # float64 [P]
    cls: np.ndarray                 # int32 [P]
    tree: np.ndarray                # int32 [P]
    bias: np.ndarray                # float64 [K]
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def n_paths(self) -> int:
        return int(self.len.shape[0])

    def on(self, device) -> dict:
        key = str(device)
        if key not in self._dev:
            d = {}
            for n in PATH_ARRAYS + ("bias",):
                a = np.ascontiguousarray(getattr(self, n))
                if a.dtype == np.uint32:
                    a = a.view(np.int32)
                d[n] = torch.from_numpy(a).to(device)
            # the launchers' view of these tensors: cached with them, so one dict keeps both alive
            d["view"] = PathView(*(d[n].data_ptr() for n in PATH_ARRAYS), P=self.n_paths, G=self.G)
            self._dev[key] = d
        return self._dev[key]

    def baseline_weights(self, device) -> torch.Tensor:
        """``T[p][q] = (p-1)! q! / (p+q)!`` as float64 ``[G, G]`` on ``device`` (row 0 is unused and 0): exact
        rationals rounded once. A path has at most ``G - 1`` real elements, so ``p + q <= G - 1`` is all that is
        ever read."""
        d = self.on(device)
        if "T" not in d:
            G = max(int(self.G), 1)
            T = np.zeros((G, G), np.float64)
            for p in range(1, G):
                t = Fraction(1, p)
                for q in range(G):
                    if q:
                        t = t * q / (p + q)
                    T[p, q] = float(t)
            d["T"] = torch.from_numpy(T).to(device)
        return d["T"]


class _Elem:
    __slots__ = ("feature", "zf", "cat", "lo", "hi", "has_hi", "na_ok", "mask", "nbits")

    def copy(self):
        e = _Elem()
        for s in self.__slots__:
            setattr(e, s, getattr(self, s))
        return e


def _merge(e: _Elem | None, f: int, frac: float, is_cat: bool, thr: float, bits: int, nbits: int, na_left: bool,
           go_left: bool) -> _Elem:
    """AND one split (taken toward ``go_left``) into the path's element of feature ``f``."""
    toward = na_left if go_left else not na_left
    if e is None:
        e = _Elem()
        e.feature, e.zf, e.cat = f, 1.0, is_cat
        e.lo, e.hi, e.has_hi, e.na_ok = float("-inf"), float("inf"), False, True
        e.mask, e.nbits = 0, 0                        # zero-width bitset: every code takes the NA side
    else:
        e = e.copy()
        if e.cat != is_cat:
            raise ValueError(f"feature {f} is split both as numeric and as categorical")
    e.zf *= frac
    was_ok, e.na_ok = e.na_ok, e.na_ok and toward
    if is_cat:
        full = (1 << nbits) - 1
        m = bits & full if go_left else ~bits & full
        w = max(e.nbits, nbits)
        # codes past a split's own width take that split's NA direction
        if toward and nbits < w:
            m |= ((1 << w) - 1) ^ full
        old = e.mask
        if was_ok and e.nbits < w:
            old |= ((1 << w) - 1) ^ ((1 << e.nbits) - 1)
        e.mask, e.nbits = old & m, w
    elif go_left:
        # x < thr; a NaN threshold sends every value right, so nothing goes left
        t = float("-inf") if thr != thr else thr
        e.hi, e.has_hi = (min(e.hi, t) if e.has_hi else t), True
    elif thr == thr:
        e.lo = max(e.lo, thr)
    return e


def forest_paths(forest) -> PathTable:
    """Path table of ``forest`` (cached on it; dropped with the flat arrays when the forest changes)."""
    cache = forest.__dict__.setdefault("_paths", {})
    if "table" in cache:
        return cache["table"]
    fl = forest.flatten()
    cover = np.concatenate([t.cover.astype(np.float64) for t in forest.trees]) if forest.trees else np.zeros(0)
    feat, thr, left, right = fl["feat"].tolist(), fl["thr"].astype(np.float64).tolist(), fl["left"].tolist(), fl["right"].tolist()
    nal, coff, cnb = fl["na_left"].tolist(), fl["cat_off"].tolist(), fl["cat_nbits"].tolist()
    words, val, cov = fl["cat_bits"], fl["value"].astype(np.float64).tolist(), cover.tolist()
    paths = []          # (tree, cls, value, [elements])
    for ti, (root, cls) in enumerate(zip(fl["roots"].tolist(), fl["cls"].tolist())):
        stack = [(root, {})]
        while stack:
            n, els = stack.pop()
            f = feat[n]
            if f < 0:
                paths.append((ti, cls, val[n], list(els.values())))
                continue
            cn = cov[n] if cov[n] > 0 else 1.0
            is_cat = coff[n] >= 0
            bits = 0
            if is_cat:
                nw = (cnb[n] + 31) >> 5
                for k, wd in enumerate(words[coff[n]:coff[n] + nw].tolist()):
                    bits |= int(wd) << (32 * k)
            for child, go_left in ((left[n], True), (right[n], False)):
                nxt = dict(els)
                nxt[f] = _merge(els.get(f), f, cov[child] / cn, is_cat, thr[n], bits, cnb[n], bool(nal[n]), go_left)
                stack.append((child, nxt))
    P = len(paths)
    max_len = 1 + max((len(p[3]) for p in paths), default=0)
    G = next((g for g in (8, 16, 32, 64) if g >= max_len), max_len)
    shape = (P, G)
    t = PathTable(G=G, max_len=max_len, n_features=0, K=int(forest.K),
                  feat=np.full(shape, -1, np.int32), zf=np.ones(shape, np.float64),
                  lo=np.full(shape, -np.inf, np.float32), hi=np.full(shape, np.inf, np.float32),
                  flags=np.full(shape, NA_OK, np.int32), cat_off=np.zeros(shape, np.int32),
                  cat_nbits=np.zeros(shape, np.int32), cat_bits=np.zeros(1, np.uint32),
                  len=np.ones(P, np.int32), value=np.zeros(P, np.float64), cls=np.zeros(P, np.int32),
                  tree=np.zeros(P, np.int32), bias=np.zeros(max(int(forest.K), 1), np.float64))
    cat_words = []
    nw_total = 0
    for p, (ti, cls, v, els) in enumerate(paths):
        t.tree[p], t.cls[p], t.value[p], t.len[p] = ti, cls, v, 1 + len(els)
        w = v
        for j, e in enumerate(els, start=1):
            t.feat[p, j], t.zf[p, j] = e.feature, e.zf
            w *= e.zf
            fg = NA_OK if e.na_ok else 0
            if e.cat:
                nw = max(1, (e.nbits + 31) >> 5)
                cat_words.extend((e.mask >> (32 * k)) & 0xFFFFFFFF for k in range(nw))
                t.cat_off[p, j], t.cat_nbits[p, j] = nw_total, e.nbits
                nw_total += nw
                fg |= IS_CAT
            else:
                t.lo[p, j] = e.lo
                if e.has_hi:
                    t.hi[p, j] = e.hi
                    fg |= HAS_HI
            t.flags[p, j] = fg
        t.bias[cls] += w
    if cat_words:
        t.cat_bits = np.asarray(cat_words, dtype=np.uint32)
    t.n_features = int(t.feat.max()) + 1 if P else 0
    cache["table"] = t
    return t


def _check_shap_args(paths: PathTable, X: torch.Tensor, K: int, rows: int, out: torch.Tensor | None) -> torch.Tensor:
    """The checks of :func:`path_shap` and :func:`path_shap_baseline`; returns ``out``, or a new zeroed one if None."""
    F = X.shape[0]
    if paths.n_features > F:
        raise ValueError(f"the forest splits on feature {paths.n_features - 1}, X has {F} rows")
    if int(paths.cls.max(initial=0)) >= K:
        raise ValueError("a tree's class is outside [0, K)")
    if out is None:
        return torch.zeros(rows, K, F + 1, dtype=torch.float64, device=X.device)
    if (out.dtype != torch.float64 or out.device != X.device or not out.is_contiguous() or out.dim() != 3
            or out.shape[0] < rows or tuple(out.shape[1:]) != (K, F + 1)):
        raise ValueError(f"out must be a contiguous float64 [>= {rows}, {K}, {F + 1}] tensor on {X.device}")
    return out


def path_shap(paths: PathTable, X: torch.Tensor, K: int, rounds: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """X: float32 ``[F, N]`` column-major model matrix -> contributions ``[N, K, F+1]`` float64 on X's
    device (margin space, per-tree sums, last column = bias). ``rounds`` > 0 fixes how many groups of
    paths one block of the kernel walks (0: chosen from the grid size). ``out``: a contiguous float64
    ``[>= N, K, F+1]`` tensor on X's device to accumulate into (its first N rows) instead of a new one."""
    if paths.max_len > MAX_PATH_LEN:
        raise ValueError(f"longest path has {paths.max_len} elements, more than the {MAX_PATH_LEN} lanes of a wave")
    F, N = X.shape
    out = _check_shap_args(paths, X, K, N, out)
    if N == 0:
        return out
    Xc = X.contiguous().float()
    d = paths.on(X.device)
    if paths.n_paths:
        if X.is_cuda:
            nat.call("h2o_tree_shap", Xc.data_ptr(), N, F, K, d["view"], int(rounds), out.data_ptr(),
                     nat.stream_ptr(X.device))
        else:
            _path_shap_torch(d, paths.G, Xc, K, out[:N])
    out[:N, :paths.bias.shape[0], F] += d["bias"][:K]
    return out


def _elements_ok(d: dict, x: torch.Tensor) -> torch.Tensor:
    """The kernels' condition test: x ``[n, P, G]`` holds, per path element, the row's value of the element's
    feature -> bool ``[n, P, G]``. NaN and out-of-range categorical codes take ``na_ok``."""
    flags, cnb, coff, bits = d["flags"], d["cat_nbits"].long(), d["cat_off"].long(), d["cat_bits"].long() & 0xFFFFFFFF
    na_ok, is_cat, has_hi = (flags & NA_OK) != 0, (flags & IS_CAT) != 0, (flags & HAS_HI) != 0
    isnan = torch.isnan(x)
    code = torch.nan_to_num(x, nan=-1.0, posinf=-1.0, neginf=-1.0).clamp(-1.0, 2.0 ** 30).long()
    inr = (code >= 0) & (code < cnb)
    cs = torch.where(inr, code, torch.zeros_like(code))
    word = bits[(coff + (cs >> 5)).clamp(max=bits.numel() - 1)]
    catok = torch.where(inr, ((word >> (cs & 31)) & 1) != 0, na_ok)
    numok = (x >= d["lo"]) & (~has_hi | (x < d["hi"]))
    return torch.where(isnan, na_ok, torch.where(is_cat, catok, numok))


def _path_shap_torch(d: dict, G: int, X: torch.Tensor, K: int, out: torch.Tensor) -> None:
    """The kernel's arithmetic, vectorised over (rows, paths, elements): EXTEND builds the permutation
    weights of every path, UNWOUND_SUM removes each element in turn."""
    F, N = X.shape
    P = d["len"].shape[0]
    feat, zf, ln = d["feat"].long(), d["zf"], d["len"].long()
    e = torch.arange(G)
    real = (e[None, :] >= 1) & (e[None, :] < ln[:, None])           # [P, G]
    fidx = feat.clamp(min=0)
    dst = (d["cls"].long()[:, None] * (F + 1) + fidx).reshape(1, -1)
    rcp = torch.zeros(G + 2, dtype=torch.float64)
    rcp[1:] = 1.0 / torch.arange(1, G + 2, dtype=torch.float64)
    dl = (ln - 1)                                                       # index of the last element
    max_len = int(ln.max())
    step = max(1, (1 << 21) // max(1, P * G))
    o2 = out.view(N, K * (F + 1))
    for r0 in range(0, N, step):
        x = X[:, r0:r0 + step].T[:, fidx]                               # [n, P, G]
        n = x.shape[0]
        ok = _elements_ok(d, x)
        of = torch.where(real, ok, torch.ones_like(ok)).double()          # dummy and padding: 1
        pw = torch.zeros(n, P, G, dtype=torch.float64)
        pw[:, :, 0] = 1.0
        for dd in range(1, max_len):
            lft = torch.zeros_like(pw)
            lft[:, :, 1:] = pw[:, :, :-1]
            new = pw * zf[:, dd:dd + 1] * ((dd - e).double() * rcp[dd + 1]) + of[:, :, dd:dd + 1] * lft * (e.double() * rcp[dd + 1])
            pw = torch.where((dd < ln)[None, :, None], new, pw)
        nxt = torch.gather(pw, 2, dl[None, :, None].expand(n, P, 1)).expand(n, P, G).clone()
        tot = torch.zeros_like(pw)
        c1 = (dl + 1).double()[None, :, None]
        c2 = zf * rcp[dl + 1][:, None]
        c3 = c1 / zf
        hot = of != 0
        for i in range(max_len - 2, -1, -1):
            pi = pw[:, :, i:i + 1]
            act = (i < dl)[None, :, None]
            tmp = nxt * c1 * rcp[i + 1]
            k = (dl - i).clamp(min=0)
            cold = pi * c3 * rcp[k][None, :, None]
            tot = torch.where(act, tot + torch.where(hot, tmp, cold), tot)
            nxt = torch.where(act & hot, pi - tmp * c2 * k.double()[None, :, None], nxt)
        contrib = torch.where(real, tot * (of - zf) * d["value"][None, :, None], torch.zeros_like(tot))
        o2[r0:r0 + n].scatter_add_(1, dst.expand(n, -1), contrib.reshape(n, -1))


def path_shap_baseline(paths: PathTable, X: torch.Tensor, B: torch.Tensor, K: int, per_reference: bool = False,
                       out: torch.Tensor | None = None, rounds: int = 0) -> torch.Tensor:
    """Baseline SHAP of the rows X against the background rows B, both float32 ``[F, n]`` column-major model
    matrices on one device -> float64 on that device, margin space, per-tree sums, last column = bias:

    * ``per_reference=False``: ``[N, K, F+1]``, the SUM over the background rows (divide by their number for the mean);
    * ``per_reference=True``: ``[N * B, K, F+1]``, pair ``(i, j)`` at row ``i * B + j``.

    Per pair the feature cells sum to ``f(x) - f(b)`` and the bias cell is ``f(b)``. ``out``: a contiguous float64
    tensor of that shape (or with more rows) on X's device to accumulate into instead of a new one. ``rounds`` > 0
    fixes how many groups of paths one block of the kernel walks. CUDA tensors run ``k_shap_baseline``; CPU
    tensors, and forests whose longest path has more than :data:`MAX_PATH_LEN` elements, the PyTorch evaluation
    (for CUDA inputs on the host, the result moved to the device)."""
    F, N = X.shape
    if B.dim() != 2 or B.shape[0] != F or B.device != X.device:
        raise ValueError(f"the background must be a [{F}, n] tensor on {X.device}")
    nb = int(B.shape[1])
    rows = N * nb if per_reference else N
    out = _check_shap_args(paths, X, K, rows, out)
    if rows == 0 or nb == 0 or not paths.n_paths:
        return out
    Xc, Bc = X.contiguous().float(), B.contiguous().float()
    if X.is_cuda and paths.max_len <= MAX_PATH_LEN:
        d, T = paths.on(X.device), paths.baseline_weights(X.device)
        nat.call("h2o_tree_shap_baseline", Xc.data_ptr(), N, Bc.data_ptr(), nb, F, K, d["view"], T.data_ptr(),
                 int(rounds), int(bool(per_reference)), out.data_ptr(), nat.stream_ptr(X.device))
        return out
    cpu = torch.device("cpu")
    host = out[:rows] if not X.is_cuda else torch.zeros(rows, K, F + 1, dtype=torch.float64)
    _path_shap_baseline_torch(paths.on(cpu), paths.G, paths.baseline_weights(cpu), Xc.to(cpu), Bc.to(cpu), K,
                              bool(per_reference), host)
    if X.is_cuda:
        out[:rows] += host.to(X.device)
    return out


def _path_shap_baseline_torch(d: dict, G: int, T: torch.Tensor, X: torch.Tensor, Bg: torch.Tensor, K: int,
                              per_reference: bool, out: torch.Tensor) -> None:
    """The kernel's arithmetic, vectorised over (rows, background rows, paths, elements) in chunks of about 4M
    elements. Element 0 of a path (the dummy root) carries the bias cell, as lane 0 does in the kernel."""
    F, N = X.shape
    nb = Bg.shape[1]
    P = d["len"].shape[0]
    F1 = F + 1
    ln = d["len"].long()
    e = torch.arange(G)
    real = (e[None, :] >= 1) & (e[None, :] < ln[:, None])             # [P, G]
    fidx = d["feat"].long().clamp(min=0)
    cell = torch.where(e[None, :] == 0, torch.full_like(fidx, F), fidx)
    dst = (d["cls"].long()[:, None] * F1 + cell).reshape(1, -1)
    val = d["value"][None, None, :, None]
    cap = max(1, (1 << 22) // max(1, P * G))                         # pairs per chunk
    m_step = min(nb, cap)
    n_step = max(1, cap // m_step)
    o_sum = out.view(-1, K * F1)
    o_ref = out.view(N, nb, K * F1) if per_reference else None
    for r0 in range(0, N, n_step):
        mx = (_elements_ok(d, X[:, r0:r0 + n_step].T[:, fidx]) & real)[:, None]      # [n, 1, P, G]
        n = mx.shape[0]
        for c0 in range(0, nb, m_step):
            mb = (_elements_ok(d, Bg[:, c0:c0 + m_step].T[:, fidx]) & real)[None]    # [1, m, P, G]
            m = mb.shape[1]
            xo, bo = mx & ~mb, mb & ~mx
            alive = ~(real & ~mx & ~mb).any(-1)                        # no element refuses both rows
            a, c = xo.sum(-1), bo.sum(-1)                               # [n, m, P]
            w = xo * T[a, c][..., None] - bo * T[c, a][..., None]
            w[..., 0] = (a == 0).double()                               # b reaches the leaf
            w = w * alive[..., None] * val
            if per_reference:
                t = torch.zeros(n * m, K * F1, dtype=torch.float64)
                t.scatter_add_(1, dst.expand(n * m, -1), w.reshape(n * m, -1))
                o_ref[r0:r0 + n, c0:c0 + m] += t.view(n, m, -1)
            else:
                o_sum[r0:r0 + n].scatter_add_(1, dst.expand(n, -1), w.sum(1).reshape(n, -1))

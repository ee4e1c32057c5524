"""Compressed trees and forest scoring (reference: ``hex/tree/CompressedTree.java``,
``hex/genmodel/algos/tree/SharedTreeMojoModel.java`` scoreTree).

A :class:`Tree` is a flat node table (root = 0): ``feat`` (-1 = leaf), raw-value threshold ``thr``
(numeric: ``x < thr`` goes left), ``na_left``, categorical level bitsets, children, leaf ``value``,
``cover`` (weighted rows, used by TreeSHAP) and split ``gain`` (variable importance).
:class:`Forest` concatenates trees (with their class index) and scores raw features either with the
HIP kernel ``k_predict`` of ``csrc/predict_kernels.hip`` (CUDA tensors) or a vectorised PyTorch traversal (CPU).
:meth:`Forest.predict_raw_grid` scores the rows once per grid tuple of a feature set (partial dependence,
``explain.py``): ``k_predict_grid`` of ``csrc/pdp_kernels.hip`` on CUDA tensors, overwrite-and-rescore on CPU.
:meth:`Forest.predict_raw_permuted` scores them once per shuffled feature (permutation importance,
``rapids._permutation_varimp``): ``k_predict_permuted`` of ``csrc/permute_kernels.hip`` on CUDA tensors, clone,
overwrite and re-score on CPU.
:meth:`Forest.predict_stages` gives the per-tree and per-feature by-products of one walk (staged margins, leaf
assignments, feature frequencies): ``k_forest_stages`` of ``csrc/forest_stages_kernels.hip`` on CUDA tensors, a
per-tree PyTorch loop on CPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from .tree import NA_BIN, TreeLevels

FLAT_ARRAYS = ("feat", "thr", "left", "right", "na_left", "cat_off", "cat_bits", "cat_nbits", "value", "roots", "cls")


class ForestView(ctypes.Structure):
    """``ForestView`` of ``csrc/forest_view.h``: the device pointers of :meth:`Forest.flatten`'s arrays."""
    _fields_ = [(n, nat.c_void_p) for n in FLAT_ARRAYS] + [("n_trees", nat.c_int), ("n_nodes", nat.c_int)]


_view_p = ctypes.POINTER(ForestView)
nat.register_hip_signatures({
    # X, N, K, forest, out, leaf_out, stream
    "h2o_predict": [nat.c_void_p, nat.c_ll, nat.c_int, _view_p] + [nat.c_void_p] * 3,
    # X, N, K, forest, sel, V, G, masks, featx, ws_chunks, out, stream
    "h2o_predict_grid": [nat.c_void_p, nat.c_ll, nat.c_int, _view_p] + [nat.c_void_p] * 2 + [nat.c_ll]
                        + [nat.c_void_p] * 2 + [nat.c_int] + [nat.c_void_p] * 2,
    # X, N, K, F, forest, feats, src, J, fmask, chunk, max_chunks, out, stream
    "h2o_predict_permuted": [nat.c_void_p, nat.c_ll, nat.c_int, nat.c_int, _view_p] + [nat.c_void_p] * 2 + [nat.c_ll]
                            + [nat.c_void_p] + [nat.c_int] * 2 + [nat.c_void_p] * 2,
    # X, N, K, F, forest, freq_lds_bytes, stage, leaf, freq, stream
    "h2o_forest_stages": [nat.c_void_p, nat.c_ll, nat.c_int, nat.c_int, _view_p, nat.c_int] + [nat.c_void_p] * 4,
})

PD_CHUNK = 64               # grid tuples per chunk of k_predict_grid (PD_CHUNK in csrc/pdp_kernels.hip)
PD_MASK_BYTES = 64 << 20    # node masks of the chunks of one launch: 8 bytes per (chunk, node)
PV_CHUNK = 16               # variants per chunk of k_predict_permuted (1 ... 64; measured: profiles/permvi_gpu.md)
PV_LAUNCH_CHUNKS = 65535    # chunks per launch of k_predict_permuted (grid y); further chunks go in further launches
STAGES_FREQ_LDS_BYTES = 16 << 10    # k_forest_stages counts feature frequencies in LDS while F * 256 bytes fit under
                                    # this (F <= 64: at least 10 waves per CU), in the output array itself past it


@dataclass
class Tree:
    feat: np.ndarray
    thr: np.ndarray
    bin: np.ndarray
    na_left: np.ndarray
    is_cat: np.ndarray
    cat_bits: list          # per node: None or np.uint32 array over LEVELS
    cat_nbits: np.ndarray
    left: np.ndarray
    right: np.ndarray
    value: np.ndarray
    cover: np.ndarray
    gain: np.ndarray

    @property
    def n_nodes(self):
        return len(self.feat)

    def depth(self) -> int:
        d = np.zeros(self.n_nodes, dtype=np.int64)
        for i in range(self.n_nodes):
            if self.feat[i] >= 0:
                d[self.left[i]] = d[i] + 1
                d[self.right[i]] = d[i] + 1
        return int(d.max()) if self.n_nodes else 0

    def n_leaves(self) -> int:
        return int((self.feat < 0).sum())

    def to_state(self):
        return {k: (v.tolist() if isinstance(v, np.ndarray) else [None if b is None else b.tolist() for b in v])
                for k, v in self.__dict__.items()}

    @staticmethod
    def from_state(s):
        kw = {}
        for k, v in s.items():
            if k == "cat_bits":
                kw[k] = [None if b is None else np.asarray(b, dtype=np.uint32) for b in v]
            else:
                kw[k] = np.asarray(v)
        kw["thr"] = kw["thr"].astype(np.float32)
        kw["value"] = kw["value"].astype(np.float32)
        return Tree(**kw)


def levels_to_tree(tl: TreeLevels, binning, leaf_values=None) -> Tree:
    """Flatten level-wise decisions into a node array (root 0, children appended in visit order).
    Hot on the host during training (one call per tree, overlapped with GPU work): per-level columns
    are pulled out of the structured records once, the node loop touches only Python scalars."""
    vals = (tl.leaf_values if leaf_values is None else leaf_values)
    vals = [] if vals is None else np.asarray(vals, dtype=np.float64).tolist()
    nv = len(vals)
    feat, thr, bins, nal, iscat, bits, nbits, left, right, value, cover, gain = ([] for _ in range(12))

    def new(c):
        feat.append(-1); thr.append(0.0); bins.append(0); nal.append(0); iscat.append(0); bits.append(None)
        nbits.append(0); left.append(-1); right.append(-1); value.append(0.0); cover.append(c); gain.append(0.0)
        return len(feat) - 1

    ids = [new(tl.root_weight)]
    for d, decs in enumerate(tl.decs):
        fz, bz, nz, cz = decs["feat"].tolist(), decs["bin"].tolist(), decs["na_left"].tolist(), decs["is_cat"].tolist()
        gz, wlz, wrz = decs["gain"].tolist(), decs["wl"].tolist(), decs["wr"].tolist()
        clz, crz = np.asarray(tl.child_l[d]).tolist(), np.asarray(tl.child_r[d]).tolist()
        nxt = {}
        for i in range(len(fz)):
            g = ids[i]
            f, cl, cr = fz[i], clz[i], crz[i]
            if f < 0:
                value[g] = vals[-1 - cl] if cl < 0 and -1 - cl < nv else 0.0
                continue
            # engine column -> original feature (wide numeric features span several engine columns)
            feat[g], bins[g], nal[g], iscat[g], gain[g] = binning.orig(f), bz[i], nz[i], cz[i], gz[i]
            if cz[i]:
                nl = int(binning.nlevels[f])
                bits_b = decs["bits"][i]
                lv = np.arange(nl)
                if cz[i] == 2:
                    # wide-categorical group split: the bitset is over the group's global bins 254k + b (level_to_bin
                    # of real column k names the levels it holds; the others' bytes say 'elsewhere' = nbins - 1)
                    bl = np.full(nl, -1, dtype=np.int64)
                    for k in range(4):
                        if f + k >= binning.F or binning.orig(f + k) != binning.orig(f) or \
                                (binning.pad is not None and binning.pad[f + k]):
                            break
                        mk = np.asarray(binning.level_to_bin[f + k], dtype=np.int64)
                        hold = mk[lv] < int(binning.nbins[f + k]) - 1
                        bl[hold] = 254 * k + mk[lv][hold]
                    inleft = np.zeros(nl, dtype=bool)
                    ok = bl >= 0
                    inleft[ok] = ((bits_b[bl[ok] >> 5] >> (bl[ok] & 31).astype(np.uint32)) & 1).astype(bool)
                    iscat[g] = 1
                else:
                    m = binning.level_to_bin[f] if binning.level_to_bin else None
                    bl = lv if m is None else m[lv]
                    inleft = ((bits_b[bl >> 5] >> (bl & 31).astype(np.uint32)) & 1).astype(bool)
                words = np.zeros((nl + 31) // 32, dtype=np.uint32)
                lvl = np.nonzero(inleft)[0]
                np.bitwise_or.at(words, lvl >> 5, (np.uint32(1) << (lvl & 31).astype(np.uint32)))
                bits[g], nbits[g], thr[g] = words, nl, 0.0
            else:
                b = bz[i]
                e = binning.edges[f]
                thr[g] = float("inf") if b >= NA_BIN or b - 1 >= len(e) else float(e[b - 1])
            for c, w, arr in ((cl, wlz[i], left), (cr, wrz[i], right)):
                k = new(w)
                arr[g] = k
                if c >= 0:
                    nxt[c] = k
                else:
                    value[k] = vals[-1 - c] if -1 - c < nv else 0.0
        ids = [nxt[c] for c in sorted(nxt)]
    return Tree(feat=np.asarray(feat, dtype=np.int32), thr=np.asarray(thr, dtype=np.float32),
                bin=np.asarray(bins, dtype=np.int32), na_left=np.asarray(nal, dtype=np.int8),
                is_cat=np.asarray(iscat, dtype=np.int8), cat_bits=bits,
                cat_nbits=np.asarray(nbits, dtype=np.int32), left=np.asarray(left, dtype=np.int32),
                right=np.asarray(right, dtype=np.int32), value=np.asarray(value, dtype=np.float32),
                cover=np.asarray(cover, dtype=np.float64), gain=np.asarray(gain, dtype=np.float64))


class Forest:
    """Trees + class assignment, with cached flat device arrays for scoring."""

    def __init__(self, trees=None, tree_class=None, n_classes_out: int = 1):
        self._trees = list(trees or [])
        self._pending = []          # (TreeLevels, binning) decoded on first access of ``trees``
        self.tree_class = list(tree_class or [0] * len(self._trees))
        self.K = n_classes_out
        self._flat = {}
        self._paths = {}            # TreeSHAP path table (ops/shap.py), dropped together with ``_flat``

    def invalidate(self):
        """Drop everything derived from the node tables (flat device arrays, TreeSHAP path table)."""
        self._flat.clear()
        self.__dict__.setdefault("_paths", {}).clear()

    @property
    def trees(self):
        """Node tables of every tree. Trees added with :meth:`add_levels` are decoded from their level
        records here, on first use (scoring, MOJO, summaries), so the training loop never waits on the
        host-side flattening of the last trees it built."""
        if self._pending:
            pend, self._pending = self._pending, []
            self._trees.extend(levels_to_tree(tl, b) for tl, b in pend)
        return self._trees

    @trees.setter
    def trees(self, v):
        self._trees = list(v)
        self._pending = []

    def add(self, tree: Tree, cls: int = 0):
        if self._pending:
            self.trees    # keep insertion order
        self._trees.append(tree)
        self.tree_class.append(cls)
        self.invalidate()

    def add_levels(self, tl, binning, cls: int = 0):
        self._pending.append((tl, binning))
        self.tree_class.append(cls)
        self.invalidate()

    def depth_leaves(self) -> list:
        """(depth, leaf count) of every tree; trees still pending as level records are read from those records
        (no host-side flattening: the model summary of a 100-tree GBM spent ~21 ms decoding every tree)."""
        out = [(t.depth(), t.n_leaves()) for t in self._trees]
        for tl, _ in self._pending:
            d = 0
            for i, dec in enumerate(tl.decs):
                if len(dec) and bool((np.asarray(dec["feat"]) >= 0).any()):
                    d = i + 1
            out.append((d, int(tl.n_leaves)))
        return out

    def __len__(self):
        return len(self._trees) + len(self._pending)

    def flatten(self, t0=0, t1=None):
        t1 = len(self.trees) if t1 is None else t1
        feat, thr, left, right, nal, coff, cnb, val, roots, cls = [], [], [], [], [], [], [], [], [], []
        bits = []
        base = 0
        for ti in range(t0, t1):
            t = self.trees[ti]
            n = t.n_nodes
            feat.append(t.feat); thr.append(t.thr)
            left.append(np.where(t.left >= 0, t.left + base, -1)); right.append(np.where(t.right >= 0, t.right + base, -1))
            nal.append(t.na_left.astype(np.int32)); val.append(t.value)
            co = np.full(n, -1, dtype=np.int32)
            for i in range(n):
                if t.feat[i] >= 0 and t.is_cat[i]:
                    co[i] = sum(len(b) for b in bits)
                    bits.append(t.cat_bits[i])
            coff.append(co); cnb.append(t.cat_nbits)
            roots.append(base); cls.append(self.tree_class[ti])
            base += n
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return dict(feat=cat(feat, np.int32), thr=cat(thr, np.float32), left=cat(left, np.int32),
                    right=cat(right, np.int32), na_left=cat(nal, np.int32), cat_off=cat(coff, np.int32),
                    cat_bits=(np.concatenate(bits).astype(np.uint32) if bits else np.zeros(1, np.uint32)),
                    cat_nbits=cat(cnb, np.int32), value=cat(val, np.float32),
                    roots=np.asarray(roots, dtype=np.int32), cls=np.asarray(cls, dtype=np.int32))

    def _device_flat(self, device, t0, t1):
        key = (str(device), t0, t1)
        if key not in self._flat:
            fl = self.flatten(t0, t1)
            d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in fl.items()}
            # the launchers' view of these tensors: cached with them, so one dict keeps both alive
            d["n_features"] = int(fl["feat"].max(initial=-1)) + 1
            d["view"] = ForestView(*(d[k].data_ptr() for k in FLAT_ARRAYS), n_trees=t1 - t0, n_nodes=d["feat"].numel())
            self._flat[key] = d
        return self._flat[key]

    def predict_raw(self, X: torch.Tensor, t0: int = 0, t1: int | None = None, out: torch.Tensor | None = None,
                    return_leaves: bool = False):
        """X: float32 [F, N] column-major. Returns [N, K] sums of leaf values (no link, no init_f)."""
        t1 = len(self.trees) if t1 is None else t1
        F, N = X.shape
        if out is None:
            out = torch.zeros(N, self.K, dtype=torch.float32, device=X.device)
        nt = t1 - t0
        leaves = torch.empty(N, max(nt, 1), dtype=torch.int32, device=X.device) if return_leaves else None
        if nt <= 0 or N == 0:
            return (out, leaves) if return_leaves else out
        fl = self._device_flat(X.device, t0, t1)
        Xc = X.contiguous().float()
        if X.is_cuda:
            nat.call("h2o_predict", Xc.data_ptr(), N, self.K, fl["view"], out.data_ptr(), nat.ptr(leaves),
                     nat.stream_ptr(X.device))
        else:
            self._predict_torch(Xc, fl, nt, out, leaves)
        return (out, leaves) if return_leaves else out

    def predict_raw_grid(self, X: torch.Tensor, feats, V, t0: int = 0, t1: int | None = None,
                         out: torch.Tensor | None = None) -> torch.Tensor:
        """:meth:`predict_raw` of X once per grid tuple: tuple ``g`` replaces row ``feats[s]`` of X by ``V[s][g]``
        for every ``s``. X: float32 [F, N]; ``feats``: distinct feature indices (a feature no tree splits on, or
        every feature, is fine); V: float32 [len(feats), G]. Returns [G, N, K] float32 on X's device, cell
        ``(g, i, c)`` bit-equal to ``predict_raw`` of the overwritten matrix. CUDA tensors run the forking walk of
        ``csrc/pdp_kernels.hip`` (no copy of X, one walk per distinct leaf); CPU tensors overwrite and re-score.
        ``out``: a contiguous float32 tensor on X's device with at least ``G * N * K`` elements; the result is then
        a view of its first ``G * N * K`` (every one of them is written, nothing after them)."""
        t1 = len(self.trees) if t1 is None else t1
        F, N = X.shape
        feats = [int(f) for f in feats]
        V = torch.as_tensor(V, dtype=torch.float32, device=X.device).reshape(len(feats), -1)
        G = int(V.shape[1])
        if len(set(feats)) != len(feats) or any(f < 0 or f >= F for f in feats):
            raise ValueError(f"feats must be distinct indices in [0, {F}), got {feats}")
        if out is None:
            out = torch.empty(G, N, self.K, dtype=torch.float32, device=X.device)
        elif (out.dtype != torch.float32 or out.device != X.device or not out.is_contiguous()
              or out.numel() < G * N * self.K):
            raise ValueError(f"out must be a contiguous float32 tensor of >= {G * N * self.K} elements on {X.device}")
        else:
            out = out.view(-1)[:G * N * self.K].view(G, N, self.K)
        nt = t1 - t0
        if nt <= 0 or N == 0 or G == 0:
            return out.zero_()
        if not X.is_cuda:
            Xg = X.float().clone()
            for g in range(G):
                for s, f in enumerate(feats):
                    Xg[f] = V[s, g]
                out[g] = self.predict_raw(Xg, t0, t1)
            return out
        fl = self._device_flat(X.device, t0, t1)
        if fl["n_features"] > F:
            raise ValueError(f"the forest splits on feature {fl['n_features'] - 1}, X has {F} rows")
        n_nodes = int(fl["feat"].numel())
        Xc, Vc = X.contiguous().float(), V.contiguous()
        sel = torch.full((F,), -1, dtype=torch.int32)
        sel[feats] = torch.arange(len(feats), dtype=torch.int32)
        sel = sel.to(X.device)
        n_chunks = (G + PD_CHUNK - 1) // PD_CHUNK
        ws_chunks = max(1, min(n_chunks, PD_MASK_BYTES // (8 * n_nodes)))
        masks = torch.empty(ws_chunks * n_nodes, dtype=torch.int64, device=X.device)
        featx = torch.empty(n_nodes, dtype=torch.int32, device=X.device)
        nat.call("h2o_predict_grid", Xc.data_ptr(), N, self.K, fl["view"], sel.data_ptr(), Vc.data_ptr(), G,
                 masks.data_ptr(), featx.data_ptr(), ws_chunks, out.data_ptr(), nat.stream_ptr(X.device))
        return out

    def predict_raw_permuted(self, X: torch.Tensor, feats, src, t0: int = 0, t1: int | None = None,
                             out: torch.Tensor | None = None) -> torch.Tensor:
        """:meth:`predict_raw` of X once per variant: variant ``j`` sees ``X[feats[j]][src[j, i]]`` in place of
        ``X[feats[j]][i]`` (permutation importance, ``rapids._permutation_varimp``). X: float32 [F, N]; ``feats``: J
        feature indices in [0, F), repeats allowed; ``src``: integer [J, N] on X's device or the host, every entry in
        [0, N) (a row need not be a permutation; it is converted to int32). Returns [J, N, K] float32 on X's
        device, cell ``(j, i, c)`` bit-equal to ``predict_raw`` of a clone of X whose row ``feats[j]`` is
        ``X[feats[j]][src[j]]``. CUDA tensors run the forking walk of ``csrc/permute_kernels.hip`` (no copy of X, one
        extra sub-walk per variant that leaves the row's own path); CPU tensors clone, overwrite and re-score.
        ``out``: as in :meth:`predict_raw_grid`, at least ``J * N * K`` elements."""
        t1 = len(self.trees) if t1 is None else t1
        F, N = X.shape
        feats = [int(f) for f in feats]
        J = len(feats)
        if any(f < 0 or f >= F for f in feats):
            raise ValueError(f"feats must be indices in [0, {F}), got {feats}")
        src = torch.as_tensor(src)
        if src.dtype.is_floating_point or src.dtype.is_complex or src.dtype == torch.bool:
            raise ValueError(f"src must be an integer tensor, got {src.dtype}")
        if tuple(src.shape) != (J, N):
            raise ValueError(f"src must have shape {(J, N)}, got {tuple(src.shape)}")
        src = src.to(X.device)
        if src.numel():         # one reduction, one host read: the kernel reads X[feats[j]][src[j, i]] unguarded
            lo, hi = torch.stack(torch.aminmax(src)).tolist()
            if lo < 0 or hi >= N:
                raise ValueError(f"src must hold row indices in [0, {N}), got [{lo}, {hi}]")
        if out is None:
            out = torch.empty(J, N, self.K, dtype=torch.float32, device=X.device)
        elif (out.dtype != torch.float32 or out.device != X.device or not out.is_contiguous()
              or out.numel() < J * N * self.K):
            raise ValueError(f"out must be a contiguous float32 tensor of >= {J * N * self.K} elements on {X.device}")
        else:
            out = out.view(-1)[:J * N * self.K].view(J, N, self.K)
        nt = t1 - t0
        if nt <= 0 or N == 0 or J == 0:
            return out.zero_()
        if not X.is_cuda:
            Xp = X.float().clone()
            for j, f in enumerate(feats):
                Xp[f] = X[f][src[j].long()]
                out[j] = self.predict_raw(Xp, t0, t1)
                Xp[f] = X[f]
            return out
        fl = self._device_flat(X.device, t0, t1)
        if fl["n_features"] > F:
            raise ValueError(f"the forest splits on feature {fl['n_features'] - 1}, X has {F} rows")
        if N >= 1 << 31:
            raise ValueError(f"int32 row indices: N = {N} must be below 2^31")
        Xc, srcc = X.contiguous().float(), src.to(torch.int32).contiguous()
        chunk = max(1, min(int(PV_CHUNK), 64))
        fmask = np.zeros(((J + chunk - 1) // chunk, F), dtype=np.uint64)    # bit b of [c][f]: variant c * chunk + b shuffles f
        for j, f in enumerate(feats):
            fmask[j // chunk, f] |= np.uint64(1) << np.uint64(j % chunk)
        fmask = torch.from_numpy(fmask.view(np.int64)).to(X.device)
        fe = torch.tensor(feats, dtype=torch.int32).to(X.device)
        nat.call("h2o_predict_permuted", Xc.data_ptr(), N, self.K, F, fl["view"], fe.data_ptr(), srcc.data_ptr(), J,
                 fmask.data_ptr(), chunk, int(PV_LAUNCH_CHUNKS), out.data_ptr(), nat.stream_ptr(X.device))
        return out

    def predict_stages(self, X: torch.Tensor, t0: int = 0, t1: int | None = None, *, stage: bool = True,
                       leaves: bool = False, freq: bool = False, out: torch.Tensor | None = None):
        """The per-tree and per-feature by-products of ONE walk of the trees ``[t0, t1)`` over X (float32 [F, N]),
        tree-major so that a column of a result frame is one contiguous row. ``stage``: float32 [T, N], cell
        ``(t, i)`` = the fp32 sum in forest order of the leaf values of the trees ``t' <= t`` of tree ``t``'s class,
        bit-equal to ``predict_raw(X, t0, t0 + t + 1)[i, cls[t]]``; ``leaves``: int32 [T, N], what
        ``predict_raw(..., return_leaves=True)`` gives, transposed; ``freq``: int32 [F, N], the number of split nodes
        on row i's T paths that split on feature f. Returns the requested tensors on X's device in that order (one
        tensor when one is asked for, else a tuple). CUDA tensors run ``k_forest_stages``
        (``csrc/forest_stages_kernels.hip``); CPU tensors a per-tree loop over :meth:`_predict_torch`.
        ``out`` (for ``stage``): as in :meth:`predict_raw_grid`, at least ``T * N`` elements."""
        t1 = len(self.trees) if t1 is None else t1
        F, N = X.shape
        T = max(t1 - t0, 0)
        if not (stage or leaves or freq):
            raise ValueError("predict_stages: ask for at least one of stage, leaves, freq")
        if out is not None and not stage:
            raise ValueError("out= is the buffer of stage")
        st = lv = fq = None
        if stage:
            if out is None:
                st = torch.empty(T, N, dtype=torch.float32, device=X.device)
            elif (out.dtype != torch.float32 or out.device != X.device or not out.is_contiguous()
                  or out.numel() < T * N):
                raise ValueError(f"out must be a contiguous float32 tensor of >= {T * N} elements on {X.device}")
            else:
                st = out.view(-1)[:T * N].view(T, N)
        if leaves:
            lv = torch.empty(T, N, dtype=torch.int32, device=X.device)
        if freq:
            fq = torch.empty(F, N, dtype=torch.int32, device=X.device)
        res = [r for r in (st, lv, fq) if r is not None]
        ret = res[0] if len(res) == 1 else tuple(res)
        if T <= 0 or N == 0:
            for r in res:
                r.zero_()
            return ret
        fl = self._device_flat(X.device, t0, t1)
        if fl["n_features"] > F:
            raise ValueError(f"the forest splits on feature {fl['n_features'] - 1}, X has {F} rows")
        Xc = X.contiguous().float()
        if X.is_cuda:
            nat.call("h2o_forest_stages", Xc.data_ptr(), N, self.K, F, fl["view"], int(STAGES_FREQ_LDS_BYTES),
                     nat.ptr(st), nat.ptr(lv), nat.ptr(fq), nat.stream_ptr(X.device))
            return ret
        acc = torch.zeros(N, self.K, dtype=torch.float32)
        leaf_all = torch.empty(N, T, dtype=torch.int32)
        self._predict_torch(Xc, fl, T, acc, leaf_all, stages=st)
        if lv is not None:
            lv.copy_(leaf_all.T)
        if fq is not None:
            # the features on the way to a leaf are fixed by the tree: one table row per node, gathered per tree
            tab = self._path_feature_counts(fl, F)
            fq.zero_()
            for t in range(T):
                fq += tab[leaf_all[:, t].long()].T
        return ret

    def leaf_tables(self, device):
        """Per flat node of the whole forest, for leaf node assignment: ``node_id`` int32 [n_nodes] on ``device``, the
        node's breadth-first position in its tree (root 0, a split's left child then its right child appended in
        visiting order: the ids of ``tree_json`` / ``h2o.tree.H2OTree``); ``path_rank`` int32 [n_nodes] on
        ``device``, for a leaf the rank of its root-to-leaf ``L`` / ``R`` string among its tree's sorted leaf paths
        (-1 for a split); ``paths``: per tree, that sorted list. Built once on the host, cached with the flat arrays."""
        key = (str(device), "leaf_tables")
        if key not in self._flat:
            ids, ranks, paths = [], [], []
            for t in self.trees:
                n = t.n_nodes
                nid = np.zeros(n, dtype=np.int32)
                order, i = [0], 0
                while i < len(order):
                    k = order[i]
                    nid[k] = i
                    if t.feat[k] >= 0:
                        order += [int(t.left[k]), int(t.right[k])]
                    i += 1
                path = [""] * n
                for k in order:                     # parents come before their children in breadth-first order
                    if t.feat[k] >= 0:
                        path[int(t.left[k])] = path[k] + "L"
                        path[int(t.right[k])] = path[k] + "R"
                leaf_paths = sorted(path[k] for k in range(n) if t.feat[k] < 0)
                pos = {p: r for r, p in enumerate(leaf_paths)}
                ranks.append(np.asarray([pos[path[k]] if t.feat[k] < 0 else -1 for k in range(n)], dtype=np.int32))
                ids.append(nid)
                paths.append(leaf_paths)
            cat = lambda xs: torch.from_numpy(np.concatenate(xs) if xs else np.zeros(0, np.int32)).to(device)
            self._flat[key] = dict(node_id=cat(ids), path_rank=cat(ranks), paths=paths)
        return self._flat[key]

    @staticmethod
    def _path_feature_counts(fl, F):
        """int32 [n_nodes, F]: per node, how many of its proper ancestors split on each feature."""
        feat, left, right, roots = (fl[k].cpu().numpy() for k in ("feat", "left", "right", "roots"))
        cnt = np.zeros((len(feat), F), dtype=np.int32)
        todo = [int(r) for r in roots]
        while todo:
            n = todo.pop()
            if feat[n] >= 0:
                for c in (int(left[n]), int(right[n])):
                    cnt[c] = cnt[n]
                    cnt[c, feat[n]] += 1
                    todo.append(c)
        return torch.from_numpy(cnt)

    @staticmethod
    def _predict_torch(X, fl, nt, out, leaves, stages=None):
        N = X.shape[1]
        ar = torch.arange(N)
        feat, thr, left, right = fl["feat"].long(), fl["thr"], fl["left"].long(), fl["right"].long()
        nal, coff, cnb, bits, val = fl["na_left"].bool(), fl["cat_off"].long(), fl["cat_nbits"].long(), fl["cat_bits"].long(), fl["value"]
        for t in range(nt):
            node = torch.full((N,), int(fl["roots"][t]), dtype=torch.long)
            for _ in range(10_000):
                f = feat[node]
                act = f >= 0
                if not bool(act.any()):
                    break
                fi = f.clamp(min=0)
                x = X[fi, ar]
                isnan = torch.isnan(x)
                co = coff[node]
                iscat = co >= 0
                code = torch.nan_to_num(x, nan=-1).long()
                inrange = (code >= 0) & (code < cnb[node])
                word = bits[(co.clamp(min=0) + (code.clamp(min=0) >> 5)).clamp(max=bits.numel() - 1)]
                catleft = ((word >> (code.clamp(min=0) & 31)) & 1).bool()
                catgo = torch.where(inrange, catleft, nal[node])
                numgo = x < thr[node]
                go = torch.where(isnan, nal[node], torch.where(iscat, catgo, numgo))
                nxt = torch.where(go, left[node], right[node])
                node = torch.where(act, nxt, node)
            out[:, int(fl["cls"][t])] += val[node]
            if stages is not None:
                stages[t] = out[:, int(fl["cls"][t])]
            if leaves is not None:
                leaves[:, t] = node.int()

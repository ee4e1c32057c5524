"""Extended Isolation Forest scoring (reference: ``hex/genmodel/algos/isoforextended/ExtendedIsolationForestMojoModel.java``
scoreTree0): the packed forest of hyperplane splits and the path-length sums of a frame over it.

:func:`pack` flattens either tree format (the trainer's dicts of ``models/isoforest.py``, ``mojo.algos.load_eif``'s
dicts) into host arrays with absolute node indices and sparse normals (``EifView`` of ``csrc/eif_view.h``);
:func:`path_length_sums` walks them: ``k_eif_path`` of ``csrc/eif_kernels.hip`` on CUDA float32 tensors (a lane per
row, no temporary that grows with rows x nodes), one fp64 GEMM per tree and a level-wise gather walk in PyTorch on
everything else.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _native as nat

EIF_ARRAYS = ("left", "right", "off", "value", "nz_begin", "nz_feat", "nz_val", "roots")
_DTYPES = dict(left=np.int32, right=np.int32, off=np.float64, value=np.float64, nz_begin=np.int32, nz_feat=np.int32,
               nz_val=np.float64, roots=np.int32)


class EifView(ctypes.Structure):
    """``EifView`` of ``csrc/eif_view.h``: the device pointers of :func:`pack`'s arrays."""
    _fields_ = [(n, nat.c_void_p) for n in EIF_ARRAYS] + [("n_trees", nat.c_int), ("n_nodes", nat.c_int)]


nat.register_hip_signatures({
    # X, N, F, forest, nan_to_zero, row_lds_bytes, out, stream
    "h2o_eif_path": [nat.c_void_p, nat.c_ll, nat.c_int, ctypes.POINTER(EifView), nat.c_int, nat.c_int]
                    + [nat.c_void_p] * 2,
})

EIF_ROW_LDS_BYTES = 64 << 10    # k_eif_path stages a block's 256 rows in LDS while F * 1024 bytes fit under this
                                # (F <= 64: at least 8 waves per CU), reads X itself past it


def hip_enabled() -> bool:
    """``H2O_EIF_HIP=0`` restores the PyTorch scoring (one fp64 GEMM per tree) on every device."""
    return os.environ.get("H2O_EIF_HIP", "1") != "0"


def _tree_arrays(tr):
    """(normal [M, F], off [M], left [M], right [M], leaf value [M] or None, leaf rows [M] or None) of one tree in
    either input format."""
    left, right = np.asarray(tr["left"], dtype=np.int64), np.asarray(tr["right"], dtype=np.int64)
    if "offset" in tr:              # the trainer's dicts
        return (np.asarray(tr["normal"], dtype=np.float64), np.asarray(tr["offset"], dtype=np.float64), left, right,
                np.asarray(tr["value"], dtype=np.float64), None)
    nrm, pt = torch.as_tensor(tr["normal"]).cpu(), torch.as_tensor(tr["point"]).cpu()
    off = (nrm * pt).sum(1)                             # (row - p) . n per node
    return nrm.numpy().astype(np.float64), off.numpy().astype(np.float64), left, right, None, np.asarray(tr["rows"])


def pack(trees, keep_zeros: bool) -> dict:
    """Host arrays of the whole forest, ``EIF_ARRAYS``: per node ``left`` / ``right`` (absolute indices, -1 = leaf),
    ``off``, ``value`` (a leaf's path length, depth + c(rows)) and ``nz_begin`` [n_nodes + 1]; per listed normal
    component ``nz_feat`` (ascending within a node) and ``nz_val``; per tree ``roots``. ``keep_zeros`` lists all F
    components of every split (imported MOJOs: a NaN or an infinity in a feature outside the hyperplane must still
    poison the projection), else only the non-zero ones (native models: their inputs are made finite first, so
    ``x * 0`` adds exactly nothing). Also ``n_features``, ``n_trees``, ``n_nodes`` and ``depth`` (int [n_trees], for
    the PyTorch walk). The device copies are cached in the dict (:func:`device_arrays`)."""
    from ..models.isoforest import c_factor
    cols = {k: [] for k in EIF_ARRAYS if k != "nz_begin"}
    counts, depths = [], []
    base, F = 0, 0
    for tr in trees:
        nrm, off, left, right, value, rows = _tree_arrays(tr)
        M, F = nrm.shape
        split = left >= 0
        d = np.zeros(M, dtype=np.int64)
        todo = [0]
        while todo:                 # children need not follow their parent in the node order
            i = todo.pop()
            if split[i]:
                d[left[i]] = d[right[i]] = d[i] + 1
                todo += [int(left[i]), int(right[i])]
        if value is None:           # load_eif's dicts: a leaf holds the rows it isolated
            value = np.array([float(k) + float(c_factor(int(r))) for k, r in zip(d.tolist(), rows.tolist())])
        listed = (np.ones_like(nrm, dtype=bool) if keep_zeros else nrm != 0) & split[:, None]
        cols["left"].append(np.where(split, left + base, -1)); cols["right"].append(np.where(split, right + base, -1))
        cols["off"].append(np.where(split, off, 0.0)); cols["value"].append(np.where(split, 0.0, value))
        cols["nz_feat"].append(np.nonzero(listed)[1]); cols["nz_val"].append(nrm[listed])
        cols["roots"].append(np.array([base]))
        counts.append(listed.sum(1))
        depths.append(int(d.max()))
        base += M
    cat = lambda k: np.concatenate(cols[k]).astype(_DTYPES[k]) if cols[k] else np.zeros(0, _DTYPES[k])
    out = {k: cat(k) for k in cols}
    nzb = np.concatenate([[0], np.cumsum(np.concatenate(counts))]) if counts else np.zeros(1)
    if base >= 1 << 31 or nzb[-1] >= 1 << 31:
        raise ValueError("int32 node and component indices: the forest is too large to pack")
    out["nz_begin"] = nzb.astype(np.int32)
    out.update(n_features=int(F), n_trees=len(cols["roots"]), n_nodes=int(base),
               depth=np.asarray(depths, dtype=np.int64), _device={}, _dense=None)
    return out


def packed_nbytes(packed) -> int:
    return sum(int(packed[k].nbytes) for k in EIF_ARRAYS)


def device_arrays(packed, device):
    """The arrays of ``packed`` on ``device`` with the launcher's view of them, cached per device."""
    key = str(device)
    if key not in packed["_device"]:
        d = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(device) for k in EIF_ARRAYS}
        # the launcher's view of these tensors: cached with them, so one dict keeps both alive
        d["view"] = EifView(*(d[k].data_ptr() for k in EIF_ARRAYS), n_trees=packed["n_trees"], n_nodes=packed["n_nodes"])
        packed["_device"][key] = d
    return packed["_device"][key]


def _dense_trees(packed):
    """Per tree (normal [M, F], off, left, right, value) with tree-local children, for the PyTorch walk."""
    if packed["_dense"] is None:
        F = packed["n_features"]
        bounds = np.append(packed["roots"], packed["n_nodes"]).astype(np.int64)
        nzb = packed["nz_begin"].astype(np.int64)
        node_of = np.repeat(np.arange(packed["n_nodes"]), np.diff(nzb))
        out = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            nrm = np.zeros((b - a, F))
            k0, k1 = nzb[a], nzb[b]
            nrm[node_of[k0:k1] - a, packed["nz_feat"][k0:k1]] = packed["nz_val"][k0:k1]
            loc = lambda c: np.where(c >= 0, c.astype(np.int64) - a, -1)
            out.append(tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in (
                nrm, packed["off"][a:b], loc(packed["left"][a:b]), loc(packed["right"][a:b]), packed["value"][a:b])))
        packed["_dense"] = out
    return packed["_dense"]


def _path_length_sums_torch(X, packed, nan_to_zero):
    Xr = X.T.double()
    if nan_to_zero:
        Xr = torch.nan_to_num(Xr, nan=0.0)
    N = Xr.shape[0]
    tot = torch.zeros(N, dtype=torch.float64, device=Xr.device)
    for (nrm, off, left, right, leafv), depth in zip(_dense_trees(packed), packed["depth"].tolist()):
        nrm, off, leafv = nrm.to(Xr.device), off.to(Xr.device), leafv.to(Xr.device)
        left, right = left.to(Xr.device), right.to(Xr.device)
        proj = Xr @ nrm.T - off                                         # one GEMM per tree
        node = torch.zeros(N, dtype=torch.long, device=Xr.device)
        for _ in range(int(depth) + 1):
            isleaf = left[node] < 0
            go_left = proj.gather(1, node[:, None]).squeeze(1) <= 0     # NaN -> right, as in scoreTree0
            nxt = torch.where(go_left, left[node], right[node])
            node = torch.where(isleaf, node, nxt)
        tot += leafv[node]
    return tot


def path_length_sums(X: torch.Tensor, packed: dict, *, nan_to_zero: bool) -> torch.Tensor:
    """float64 [N] on X's device: per row of X ([F, N]) the sum over the trees, in forest order, of the value of the
    leaf the row reaches. ``nan_to_zero``: NaN -> 0 and +-inf -> +-DBL_MAX first (the native model), else the values
    pass through and a NaN projection goes right (the MOJO scorer). CUDA float32 tensors run ``k_eif_path``
    (``csrc/eif_kernels.hip``: an ordered fp64 dot product per visited node, rows staged in LDS while
    ``F * 1024 <= EIF_ROW_LDS_BYTES``); everything else, and every tensor under ``H2O_EIF_HIP=0``, the PyTorch walk
    over one dense fp64 projection per tree (the same decisions unless a row lies within rounding of a hyperplane)."""
    F, N = X.shape
    if packed["n_trees"] and F != packed["n_features"]:
        raise ValueError(f"the forest has {packed['n_features']} features, X has {F} rows")
    if packed["n_trees"] == 0 or N == 0:
        return torch.zeros(N, dtype=torch.float64, device=X.device)
    if not (X.is_cuda and X.dtype == torch.float32 and hip_enabled()):
        return _path_length_sums_torch(X, packed, nan_to_zero)
    dv = device_arrays(packed, X.device)
    Xc = X.contiguous()
    out = torch.empty(N, dtype=torch.float64, device=X.device)
    nat.call("h2o_eif_path", Xc.data_ptr(), N, F, dv["view"], int(bool(nan_to_zero)), int(EIF_ROW_LDS_BYTES),
             out.data_ptr(), nat.stream_ptr(X.device))
    return out

"""Uplift DRF level passes on device (``csrc/uplift_kernels.hip``): the integer histogram of a node window, the node
totals of a level and the one-pass row routing.

The four statistics of a histogram cell are integers (``n_treat, y_treat, n_ctrl, y_ctrl`` with 0/1 ``y`` and
``treat`` and no weights), so the kernels add integers and the result does not depend on the order of the atomics:
:func:`level_hist` equals ``np.add.at`` into int64 exactly. ``models/uplift.py`` converts it to fp64 and runs the
divergence search on it in PyTorch (``log2`` and FMA contraction in a kernel would put the bit-equality of the forest
with the PyTorch reference at risk).

Every function here takes CUDA tensors only and raises on anything else: the PyTorch reference of these passes is
``UpliftDRFTrainer._grow`` itself, which the trainer runs on the CPU and under ``H2O_UPLIFT_HIP=0``.
"""
from __future__ import annotations

import os

import torch

from . import _native as nat

nat.register_hip_signatures({
    # bins, N, stride, F, node, treat, y, n0, W, variant, fgroup, P, stream
    "h2o_uplift_hist": [nat.c_void_p, nat.c_ll, nat.c_int, nat.c_int] + [nat.c_void_p] * 3 + [nat.c_int] * 4
                       + [nat.c_void_p] * 2,
    # N, node, treat, y, A, T, stream
    "h2o_uplift_totals": [nat.c_ll] + [nat.c_void_p] * 3 + [nat.c_int] + [nat.c_void_p] * 2,
    # bins, N, stride, F, node, A, split_feat, split_bin, child, out, stream
    "h2o_uplift_route": [nat.c_void_p, nat.c_ll, nat.c_int, nat.c_int, nat.c_void_p, nat.c_int] + [nat.c_void_p] * 5,
})

LDS_GROUPS = 32         # (node, feature) pairs of 2 KiB a block of k_uplift_hist_lds may hold: 64 KiB of LDS
LDS_MAX_WINDOW = 32     # windows of up to this many nodes take the LDS variant (one feature per block at the limit),
                        # wider ones the direct global atomics. Measured at 1M x 28 (profiles/uplift_gpu.md): the LDS
                        # variant wins at every width it holds, 0.08 against 2.85 ms at one node and 0.46 against
                        # 0.82 ms at 32; the 64 KiB of a block, not the timing, end it
# Bound on everything that grows with nodes x features x bins: a level wider than search_window(F) nodes is
# evaluated window by window, each with its own histogram launch and split search, so the packed histogram (16 B per
# cell pair), its int64 and fp64 unpackings (32 B per cell each) and every fp64 temporary of the search (8 B per
# cell) stay below WINDOW_CELLS cells = 8 MiB per fp64 temporary whatever the level's width.
WINDOW_CELLS = 1 << 20


def hip_enabled() -> bool:
    """``H2O_UPLIFT_HIP=0`` restores the PyTorch level loop of ``UpliftDRFTrainer`` on every device."""
    return os.environ.get("H2O_UPLIFT_HIP", "1") != "0"


def search_window(F: int) -> int:
    """Nodes per histogram launch and split search: ``WINDOW_CELLS`` cells of ``F * 256`` per node."""
    return max(1, WINDOW_CELLS // (int(F) * 256))


def _need_cuda(name, **tensors):
    for k, t in tensors.items():
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"{name}: {k} must be a CUDA tensor (the PyTorch reference of this pass is "
                             "UpliftDRFTrainer._grow)")


def _check_rows(name, bins, F, node, treat, y):
    _need_cuda(name, bins=bins, node=node, treat=treat, y=y)
    N = node.numel()
    if bins.dtype != torch.uint8 or bins.dim() != 2 or bins.shape[0] != N or not bins.is_contiguous():
        raise ValueError(f"{name}: bins must be contiguous uint8 [N, stride]")
    if not 1 <= F <= bins.shape[1]:
        raise ValueError(f"{name}: F = {F} is outside [1, stride = {bins.shape[1]}]")
    if node.dtype != torch.int32 or not node.is_contiguous():
        raise ValueError(f"{name}: node must be contiguous int32 [N]")
    for k, t in (("treat", treat), ("y", y)):
        if t.dtype != torch.uint8 or t.numel() != N or not t.is_contiguous():
            raise ValueError(f"{name}: {k} must be contiguous uint8 [N]")
    if N >= 1 << 31:
        raise ValueError(f"{name}: packed 32-bit counts hold fewer than 2^31 rows")
    return N


def lds_feature_group(W: int, F: int) -> int:
    """Features per block of the LDS variant for a window of ``W`` nodes (0: the window is too wide for it)."""
    return min(int(F), LDS_GROUPS // int(W)) if 1 <= W <= LDS_MAX_WINDOW else 0


def level_hist(bins, node, treat, y, n0: int, W: int, F: int, variant: str | None = None) -> torch.Tensor:
    """int64 ``[W, F, 256, 4]``: per node slot ``n0 + w``, feature and bin (255 = NA included) the rows' ``(n_treat,
    y_treat, n_ctrl, y_ctrl)``. ``bins`` uint8 ``[N, stride >= F]``, ``node`` int32 ``[N]`` (-1 or a slot outside the
    window: the row is skipped), ``treat`` / ``y`` uint8 0/1. ``variant``: ``"lds"`` (block-private LDS histogram,
    ``W <= LDS_MAX_WINDOW``), ``"direct"`` (global 64-bit atomics) or None = by the window's width."""
    N = _check_rows("level_hist", bins, F, node, treat, y)
    n0, W, F = int(n0), int(W), int(F)
    if n0 < 0 or W < 1:
        raise ValueError(f"level_hist: window [{n0}, {n0} + {W}) is empty or negative")
    if variant is None:
        variant = "lds" if W <= LDS_MAX_WINDOW else "direct"
    if variant not in ("lds", "direct"):
        raise ValueError(f"level_hist: variant must be 'lds' or 'direct', got {variant!r}")
    fg = lds_feature_group(W, F)
    if variant == "lds" and fg == 0:
        raise ValueError(f"level_hist: the LDS variant holds windows of at most {LDS_MAX_WINDOW} nodes, got {W}")
    P = torch.zeros(W, F, 256, 2, dtype=torch.int64, device=bins.device)
    nat.call("h2o_uplift_hist", bins.data_ptr(), N, bins.shape[1], F, node.data_ptr(), treat.data_ptr(), y.data_ptr(),
             n0, W, 0 if variant == "lds" else 1, fg, P.data_ptr(), nat.stream_ptr(bins.device))
    return torch.stack([P >> 32, P & 0xFFFFFFFF], -1).view(W, F, 256, 4)


def node_totals(node, treat, y, A: int) -> torch.Tensor:
    """int64 ``[A, 4]``: ``(n_treat, y_treat, n_ctrl, y_ctrl)`` of the rows of every node slot ``< A``."""
    _need_cuda("node_totals", node=node, treat=treat, y=y)
    N = node.numel()
    if node.dtype != torch.int32 or treat.dtype != torch.uint8 or y.dtype != torch.uint8 or \
            treat.numel() != N or y.numel() != N or N >= 1 << 31:
        raise ValueError("node_totals: node int32 [N], treat / y uint8 [N], N < 2^31")
    T = torch.zeros(int(A), 2, dtype=torch.int64, device=node.device)
    nat.call("h2o_uplift_totals", N, node.contiguous().data_ptr(), treat.contiguous().data_ptr(),
             y.contiguous().data_ptr(), int(A), T.data_ptr(), nat.stream_ptr(node.device))
    return torch.stack([T >> 32, T & 0xFFFFFFFF], -1).view(int(A), 4)


def route(bins, node, split_feat, split_bin, child, F: int) -> torch.Tensor:
    """int32 ``[N]``, the rows' slots in the next level: ``child[n] + (bins[r, split_feat[n]] < split_bin[n] ? 0 : 1)``
    for ``n = node[r]``, and -1 for a row that is not in the level or whose node became a leaf (``child[n] < 0``).
    A NA bin (255) goes right. ``split_feat`` / ``split_bin`` / ``child``: int32 ``[A]`` on the device."""
    _need_cuda("route", bins=bins, node=node, split_feat=split_feat, split_bin=split_bin, child=child)
    N, A = node.numel(), child.numel()
    if bins.dtype != torch.uint8 or bins.dim() != 2 or bins.shape[0] != N or not bins.is_contiguous() or \
            not 1 <= int(F) <= bins.shape[1]:
        raise ValueError("route: bins must be contiguous uint8 [N, stride >= F]")
    tabs = [split_feat, split_bin, child]
    if node.dtype != torch.int32 or any(t.dtype != torch.int32 or t.numel() != A for t in tabs):
        raise ValueError("route: node and the route table are int32, the table [A] each")
    node, tabs = node.contiguous(), [t.contiguous() for t in tabs]
    out = torch.empty_like(node)
    nat.call("h2o_uplift_route", bins.data_ptr(), N, bins.shape[1], int(F), node.data_ptr(), A,
             *(t.data_ptr() for t in tabs), out.data_ptr(), nat.stream_ptr(bins.device))
    return out

"""Shared helpers of the K-Means Lloyd kernel tests (test_kmeans_lloyd_paths.py on the CPU, test_kmeans_lloyd_gpu.py on
the device): exact-arithmetic inputs, the case table, fp64 references, the Python twin of the MFMA kernel's dispatch
table (csrc/kmeans_mfma.hip), the rounding bounds and ``raw_lloyd``, a thin call of the C entry ``h2o_kmeans_mfma``
with buffers of its own. Only ``raw_lloyd`` and what calls it need a GPU.

Exact inputs. X and C hold integers in [-8, 8] ([-3, 3] at P = 4 and in the zero-weight-cluster cases), weights are
absent or integers in {0, 1, 2, 3}. With P <= 64 every one of ||x||^2, ||c||^2, c.x, ||c||^2 - 2 c.x and their sum is
an integer of magnitude below 2 * 64 * 64 + 2 * 4096 < 2^24, so the MFMA kernel's expanded form, the scalar kernels'
(x - c)^2 form and fp64 give the same number; |w x| <= 24, so every partial sum of a centroid stays an integer below
2^24 while 24 N < 2^24. Every comparison on these inputs is an equality.

Ties. A center index is c = 16 t + 4 q + r: t the center tile, q the lane quarter (lane >> 4) and r the accumulator
register that hold its score in the 16x16 MFMA result. The kernel resolves ties in its in-lane scan over (t, r), in
the ``xor 16`` butterfly step (q ^ 1) and in the ``xor 32`` step (q ^ 2). ``COPIES`` duplicates centers so that each
of them meets exact ties; the copy with the higher index must get no row:

    C[1] = C[0]   same lane, next register        C[5] = C[0]    xor 16        C[12] = C[0]   xor 32
    C[16] = C[0], C[35] = C[2], C[50] = C[34]   same lane, another center tile
    C[20] = C[2]   another tile and xor 16

Zero-weight cluster (``zero=True``): one center (``zc``) has every entry 8, far from the [-3, 3] data; three rows lie
exactly on it and have weight 0. The cluster has rows and count 0.

Rounding bounds (u = 2^-24, in fp64 from absolute values; row x, center c, n_c rows assigned to c):

    distance, MFMA path      B = (P + 4) u (sum x^2 + 2 sum |x||c| + sum c^2)
        (||x||^2: P / 4 fma + 2 adds; ||c||^2: P fma; c.x: P fma; ||c||^2 - 2 c.x and the final add: 1 each)
    distance, scalar kernels (P + 3) u D          (x - c rounded once, squared: 2 u; the fma chain: P u)
    assignment               D[chosen] <= D[best] + B[chosen] + B[best]   (each score is within its own B)
    a sum entry              (n_c + 4) u sum_{rows of c} |w x_d|   (one fma per row, 3 adds across the waves; the
        scalar step kernel: the products' roundings add up to u sum |w x_d|, each of at most n_c - 1 inexact adds
        to u |partial sum|, the block partials are summed in fp64)
    a count                  (n_c + 4) u sum_{rows of c} |w|
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

U24 = 2.0 ** -24
KM_ROWS = 64                      # rows per wave tile (csrc: KM_ROWS)
ASSIGN_SENTINEL = -77
MIND_SENTINEL = -12345.0          # a real distance is never negative
PAD = 64                          # sentinel elements behind assign / mind

# ---------------------------------------------------------------- the dispatch table of csrc/kmeans_mfma.hip
PS_PT = ((4, 1), (4, 2), (6, 2), (8, 2), (8, 3), (16, 3), (16, 4), (16, 5))
CLASSES = tuple((kt, ps, pt) for kt in (1, 2, 4) for ps, pt in PS_PT)          # the 24 L(KT, PS, PT) lines


def mfma_shape(K, P):
    """(KT, PS, PT) of h2o_kmeans_mfma_shape, None where the MFMA kernel does not apply."""
    if K < 1 or P < 1 or K > 64 or P > 64:
        return None
    KT = 1 if K <= 16 else (2 if K <= 32 else 4)
    PS = 4 if P <= 16 else (6 if P <= 24 else (8 if P <= 32 else 16))
    return KT, PS, (P + 1 + 15) // 16


def occ4(KT, PS, PT):
    """Shapes that run the 4-waves-per-SIMD variant k_lloyd_mfma4 (km_occ4) unless H2O_KM_OCC4=0."""
    return KT == 1 and PS <= 6 and PT <= 2


def stride_branch(P, o4=False):
    """Which return of km_stride a shape takes: 'pad' (17 mod 32) or 'plain' (P + 1). At P = 16 and 48 the two
    strides coincide; the branch taken is 'pad'."""
    pp = P + 1
    return "pad" if pp + ((17 - pp % 32) + 32) % 32 <= (38 if o4 else 52) else "plain"


def km_stride(P, o4=False):
    pp = P + 1
    return pp + ((17 - pp % 32) + 32) % 32 if stride_branch(P, o4) == "pad" else pp


def variant(K, P, occ4_enabled=True):
    """(kernel variant, km_stride branch) a shape reaches."""
    sh = mfma_shape(K, P)
    o4 = occ4(*sh) and occ4_enabled
    return ("occ4" if o4 else "occ3"), stride_branch(P, o4)


# ---------------------------------------------------------------- ties
COPIES = ((1, 0), (5, 0), (12, 0), (16, 0), (35, 2), (50, 34), (20, 2))        # (copy, source), applied in order
_SPECIAL = {i for pair in COPIES for i in pair}


def route(a, b):
    """Where the kernel meets a tie of centers a != b: a set out of lane | xor16 | xor32 (which step) and tile."""
    ta, qa, tb, qb = a >> 4, (a >> 2) & 3, b >> 4, (b >> 2) & 3
    out = set()
    if (qa >> 1) != (qb >> 1):
        out.add("xor32")
    elif qa != qb:
        out.add("xor16")
    elif ta == tb:
        out.add("lane")
    if ta != tb:
        out.add("tile")
    return out


def intended_routes(c):
    out = set()
    for cp, src in COPIES:
        if cp < c.K:
            out |= route(src, cp)
    if c.natural:
        out.add("natural")
    return out


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    K: int
    P: int
    N: int
    grid: int = 1
    wt: str = "int"            # int ({0, 1, 2, 3}) | none
    zero: bool = False         # far center with zero-weight rows on it
    ties: bool = True          # the case must have a row tied through every intended route
    natural: bool = False      # ... and a tie between centers that differ
    seed: int = 0

    @property
    def lim(self):
        return 3 if (self.P == 4 or self.zero) else 8


def _name(K, P, N, grid, extra=""):
    return f"K{K}P{P}-N{N}-g{grid}{extra}"


N_TAIL37 = 64 * 4 * 3 + 37     # 805: at grid 1 three full rounds, then a 37-row tile for wave 0 only
N_TAIL1 = 641                  # at grid 1: third round with two full tiles, a 1-row tile and an idle wave
N_G3 = 64 * 12 * 2 + 5         # 1541: at grid 3 two full rounds and a 5-row tile
MULTI = ((N_TAIL37, 1), (N_TAIL37, 2), (N_TAIL37, 3), (N_TAIL1, 1), (N_TAIL1, 2), (N_TAIL1, 3), (N_G3, 3))
MULTI_SHAPES = ((10, 20), (16, 16), (32, 32), (64, 64))      # occ4 plain, occ4 pad, KT 2, KT 4
OCC4_OFF_SHAPES = ((10, 20), (16, 24), (3, 12))
EDGE_N = (1, 15, 16, 17, 63, 64, 65)
EDGE_SHAPES = ((10, 20), (33, 44))


def _cases():
    c = []
    seen = set()

    def add(K, P, N, grid, extra="", **kw):
        nm = _name(K, P, N, grid, extra)
        if nm in seen:
            return
        seen.add(nm)
        kw.setdefault("ties", N >= 600)
        c.append(Case(nm, K, P, N, grid, seed=len(c) + 1, **kw))

    # every instantiation: P in {12 .. 64} x three K, one per KT; K in {1, 3} at P = 4
    for i, P in enumerate((12, 16, 24, 28, 32, 44, 60, 64)):
        for K in (16, (17, 32)[i & 1], (33, 64)[i & 1]):
            add(K, P, N_TAIL1, 2, wt=("int", "none")[(i + K) & 1])
    add(1, 4, N_TAIL1, 2, ties=False)
    add(3, 4, N_TAIL37, 1, natural=True)
    add(17, 4, N_TAIL37, 2, natural=True)
    add(64, 4, N_TAIL37, 1, natural=True)
    # multi-tile waves
    for K, P in MULTI_SHAPES + OCC4_OFF_SHAPES:
        for j, (N, grid) in enumerate(MULTI):
            add(K, P, N, grid, wt=("int", "none")[j % 3 == 2])
    # sub-tile edges, more blocks than tiles
    for K, P in EDGE_SHAPES:
        for N in EDGE_N:
            add(K, P, N, 1)
        add(K, P, 100, 4)
    # zero-weight cluster
    add(10, 20, N_TAIL37, 1, "-zero", zero=True)
    add(32, 28, N_TAIL1, 2, "-zero", zero=True)
    add(64, 64, N_TAIL37, 3, "-zero", zero=True)
    return tuple(c)


CASES = _cases()
_BY_NAME = {c.name: c for c in CASES}


def case(name):
    return _BY_NAME[name]


def occ4_off_cases():
    return [c for c in CASES if (c.K, c.P) in OCC4_OFF_SHAPES and (c.N, c.grid) in MULTI and not c.zero]


@dataclasses.dataclass(frozen=True)
class Inputs:
    X: np.ndarray              # [N, P] float32, integer valued
    C: np.ndarray              # [K, P] float32
    w: np.ndarray | None       # [N] float32 or None
    zc: int                    # index of the zero-weight cluster, -1 without one
    zrows: tuple


def exact_inputs(K, P, N, wt="int", zero=False, seed=0, lim=None):
    if lim is None:
        lim = 3 if (P == 4 or zero) else 8
    rng = np.random.default_rng(1000 + seed)
    X = rng.integers(-lim, lim + 1, (N, P)).astype(np.float32)
    C = rng.integers(-lim, lim + 1, (K, P)).astype(np.float32)
    for cp, src in COPIES:
        if cp < K:
            C[cp] = C[src]
    w = None if wt == "none" else rng.integers(0, 4, N).astype(np.float32)
    zc, zrows = -1, ()
    if zero:
        zc = max(i for i in range(K) if i not in _SPECIAL)
        C[zc] = 8.0
        zrows = tuple(sorted({0, N // 2, N - 1}))
        X[list(zrows)] = 8.0
        w[list(zrows)] = 0.0
    return Inputs(X, C, w, zc, zrows)


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    return exact_inputs(c.K, c.P, c.N, c.wt, c.zero, c.seed, c.lim)


# ---------------------------------------------------------------- references
@dataclasses.dataclass(frozen=True)
class Ref:
    assign: np.ndarray         # [N] int64, first minimum
    mind: np.ndarray           # [N] float64
    sums: np.ndarray           # [K, P] float64
    cnt: np.ndarray            # [K] float64


def distances(X, C):
    """fp64 D[N, K] = sum_d (x_d - c_d)^2, in row chunks."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty((X.shape[0], C.shape[0]))
    step = max(1, (1 << 22) // max(1, C.size))
    for i in range(0, X.shape[0], step):
        out[i:i + step] = ((X[i:i + step, None, :] - C[None]) ** 2).sum(-1)
    return out


def segment_sums(X, w, assign, K):
    """fp64 per-center weighted sums [K, P] and counts [K] of an assignment."""
    X = np.asarray(X, np.float64)
    wd = np.ones(X.shape[0]) if w is None else np.asarray(w, np.float64)
    sums = np.zeros((K, X.shape[1]))
    np.add.at(sums, assign, X * wd[:, None])
    return sums, np.bincount(assign, weights=wd, minlength=K).astype(np.float64)


def reference(X, C, w):
    D = distances(X, C)
    a = D.argmin(1)
    sums, cnt = segment_sums(X, w, a, C.shape[0])
    return Ref(a.astype(np.int64), D.min(1), sums, cnt)


@functools.lru_cache(maxsize=None)
def case_reference(c):
    inp = make_inputs(c)
    return reference(inp.X, inp.C, inp.w)


def emulate_expanded(X, C):
    """The MFMA kernel's distance arithmetic in fp32, operation by operation: ||c||^2 and c.x as chains over the
    dimensions, score = ||c||^2 - 2 c.x, strict '<' scan in center order, max(||x||^2 + score, 0)."""
    X, C = np.asarray(X, np.float32), np.asarray(C, np.float32)
    N, P = X.shape
    K = C.shape[0]
    csq = np.zeros(K, np.float32)
    xq = np.zeros(N, np.float32)
    dot = np.zeros((N, K), np.float32)
    for d in range(P):
        csq = (C[:, d] * C[:, d] + csq).astype(np.float32)
        xq = (X[:, d] * X[:, d] + xq).astype(np.float32)
        dot = (X[:, d, None] * C[None, :, d] + dot).astype(np.float32)
    sc = (csq[None] - np.float32(2) * dot).astype(np.float32)
    best = np.full(N, np.finfo(np.float32).max, np.float32)
    bidx = np.full(N, -1, np.int64)
    for k in range(K):
        m = sc[:, k] < best
        best[m], bidx[m] = sc[m, k], k
    return bidx, np.maximum((xq + best).astype(np.float32), np.float32(0))


def tie_routes(c, inp=None):
    """Routes through which at least one row of the case has an exact tie for its minimum."""
    inp = inp or make_inputs(c)
    D = distances(inp.X, inp.C)
    mn = D.min(1)
    got = set()
    for r in np.nonzero((D == mn[:, None]).sum(1) > 1)[0]:
        t = np.nonzero(D[r] == mn[r])[0]
        for b in t[1:]:
            if np.array_equal(inp.C[t[0]], inp.C[b]):
                got |= route(int(t[0]), int(b))
            else:
                got.add("natural")
    return got


def block_of_rows(N, grid):
    """Block whose slab a row's contribution lands in: tile j belongs to wave j mod (4 grid)."""
    tile = np.arange(N) // KM_ROWS
    return (tile % (4 * grid)) // 4


# ---------------------------------------------------------------- the device side
@dataclasses.dataclass
class Raw:
    assign: np.ndarray | None  # [N + PAD] int32 (None: launched with a null assign)
    mind: np.ndarray           # [N + PAD] float32
    slabs: np.ndarray          # [grid, KT*16, PT*16] float32


def raw_lloyd(X, C, w, grid, need_assign=True):
    """h2o_kmeans_mfma on buffers of its own: assign / mind PAD elements longer than N and pre-filled with a sentinel,
    the slabs pre-filled with NaN. X [N, P], C [K, P], w [N] or None: contiguous float32 CUDA tensors."""
    import torch

    from llama_github_io_amd.ops import _native as nat
    N, P = X.shape
    K = C.shape[0]
    sh = mfma_shape(K, P)
    assert sh is not None and P % 4 == 0 and N > 0 and grid > 0
    for t in (X, C) + (() if w is None else (w,)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert C.shape[1] == P and (w is None or w.shape == (N,))
    KT, PS, PT = sh
    dev = X.device
    a = torch.full((N + PAD,), ASSIGN_SENTINEL, dtype=torch.int32, device=dev) if need_assign else None
    d = torch.full((N + PAD,), MIND_SENTINEL, dtype=torch.float32, device=dev)
    slabs = torch.full((grid, KT * 16, PT * 16), float("nan"), dtype=torch.float32, device=dev)
    nat.call("h2o_kmeans_mfma", X.data_ptr(), N, P, C.data_ptr(), K, 0 if w is None else w.data_ptr(),
             0 if a is None else a.data_ptr(), d.data_ptr(), slabs.data_ptr(), int(grid), nat.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return Raw(None if a is None else a.cpu().numpy(), d.cpu().numpy(), slabs.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_exact(c, inp, ref, out, what=""):
    """Every equality an exact case owes (module docstring of test_kmeans_lloyd_gpu.py); returns the violations."""
    N, K, P = c.N, c.K, c.P
    KT, PS, PT = mfma_shape(K, P)
    bad = []

    def say(s):
        bad.append(f"{c.name}{what}: {s}")

    if out.assign is not None:
        a = out.assign[:N]
        m = np.nonzero(a != ref.assign)[0]
        if m.size:
            say(f"assign differs in {m.size} rows, first row {m[0]}: got {a[m[0]]} ref {ref.assign[m[0]]}")
        if not (out.assign[N:] == ASSIGN_SENTINEL).all():
            say("assign written past N")
    m = np.nonzero(_bits(out.mind[:N]) != _bits(ref.mind))[0]
    if m.size:
        say(f"mind differs in {m.size} rows, first row {m[0]}: got {out.mind[m[0]]!r} ref {ref.mind[m[0]]!r}")
    if not (out.mind[N:] == np.float32(MIND_SENTINEL)).all():
        say("mind written past N")
    s = out.slabs
    if s.shape != (c.grid, KT * 16, PT * 16):
        say(f"slab shape {s.shape}")
        return bad
    if np.isnan(s).any():
        say(f"{int(np.isnan(s).sum())} slab elements never written")
        return bad
    if (s[:, K:, :] != 0).any():
        say("padding center rows of a slab are not 0")
    if (s[:, :, P + 1:] != 0).any():
        say("padding dim columns of a slab are not 0")
    blk = block_of_rows(N, c.grid)
    for b in range(c.grid):
        rows = np.nonzero(blk == b)[0]
        sb, cb = segment_sums(inp.X[rows], None if inp.w is None else inp.w[rows], ref.assign[rows], K)
        if not np.array_equal(s[b, :K, :P].astype(np.float64), sb):
            say(f"block {b} sums differ ({rows.size} rows)")
        if not np.array_equal(s[b, :K, P].astype(np.float64), cb):
            say(f"block {b} counts differ ({rows.size} rows)")
        if rows.size == 0 and (s[b] != 0).any():
            say(f"block {b} has no rows and a non-zero slab")
    tot = s.astype(np.float64).sum(0)
    if not np.array_equal(tot[:K, :P], ref.sums):
        say("sums differ")
    if not np.array_equal(tot[:K, P], ref.cnt):
        say("counts differ")
    return bad


def run_exact_case(c, dev):
    """Both launches of an exact case (with and without assign) and their checks; returns the violations."""
    import torch
    inp, ref = make_inputs(c), case_reference(c)
    X = torch.from_numpy(inp.X).to(dev)
    C = torch.from_numpy(inp.C).to(dev)
    w = None if inp.w is None else torch.from_numpy(inp.w).to(dev)
    out = raw_lloyd(X, C, w, c.grid)
    bad = check_exact(c, inp, ref, out)
    out0 = raw_lloyd(X, C, w, c.grid, need_assign=False)
    bad += check_exact(c, inp, ref, out0, " (null assign)")
    if not np.array_equal(_bits(out.mind), _bits(out0.mind)) or not np.array_equal(_bits(out.slabs), _bits(out0.slabs)):
        bad.append(f"{c.name}: the launch with a null assign gives other mind / slabs")
    return bad


# ---------------------------------------------------------------- rounding cases
ROUND_SHAPES = ((10, 20), (32, 32), (64, 64))          # one per KT


def round_inputs(K, P, N=N_TAIL37, seed=0):
    """randn + 100 in every column (||x||^2 + (||c||^2 - 2 c.x) cancels five digits), weights in [0.25, 2.25)."""
    rng = np.random.default_rng(7000 + seed + 64 * K + P)
    X = (rng.standard_normal((N, P)) + 100.0).astype(np.float32)
    C = (rng.standard_normal((K, P)) + 100.0).astype(np.float32)
    w = (rng.random(N) * 2.0 + 0.25).astype(np.float32)
    return X, C, w


def mfma_dist_bound(X, C):
    """B[N, K] of the module docstring."""
    X, C = np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(C, np.float64))
    P = X.shape[1]
    return (P + 4) * U24 * ((X * X).sum(1)[:, None] + 2.0 * X @ C.T + (C * C).sum(1)[None])


def sum_bounds(X, w, assign, K):
    """(bound of every sum entry [K, P], bound of every count [K]) for an assignment."""
    n = np.bincount(assign, minlength=K).astype(np.float64)
    sa, ca = segment_sums(np.abs(np.asarray(X, np.float64)), np.abs(np.asarray(w, np.float64)), assign, K)
    return (n + 4)[:, None] * U24 * sa, (n + 4) * U24 * ca


def worst_ratio(err, bound):
    """max err / bound; an error where the bound is 0 is infinite."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------- the H2O_KM_OCC4=0 child
def _occ4_child():
    """Run in a fresh process with H2O_KM_OCC4=0 (the switch is read once per process): the exact multi-tile cases of
    the shapes whose default kernel is the 4-waves-per-SIMD variant, on k_lloyd_mfma<1, PS <= 6, PT <= 2>."""
    import os
    import torch
    assert os.environ.get("H2O_KM_OCC4") == "0"
    dev = torch.device("cuda", 0)
    bad = []
    cases = occ4_off_cases()
    for c in cases:
        assert occ4(*mfma_shape(c.K, c.P))
        bad += run_exact_case(c, dev)
    for s in bad:
        print("OCC4OFF", s)
    print(f"OCC4OFF {len(cases)} cases, {len(bad)} violations")
    return 1 if bad else 0


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert sys.argv[1:] == ["occ4-child"], sys.argv
    sys.exit(_occ4_child())

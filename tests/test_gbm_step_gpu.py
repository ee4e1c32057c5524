"""The fused GBM row step (csrc/gbm_kernels.hip k_gbm_step, k_add_leaf) and the scale kernels it feeds
(csrc/tree_kernels.hip k_amax, k_qscale) against fp64 references of the same operations.

The launchers are called directly (ops/_native.call), the way GBMTrainer._prepare calls them. The reference is the
project's own ``Distribution`` classes evaluated in fp64 on the same fp32 inputs, with the exponent argument clamped
at 80 as in the kernel; the row sample is a NumPy uint64 transcription of the kernel's splitmix64 hash. CPU-only
tests (not marked ``gpu``) anchor that reference: it agrees with what the trainer's eager path writes into ``aux``
(the same classes in fp32), and the hash reproduces the published splitmix64 vector.

Tolerances (derived, not tuned):

* planes without ``exp`` (gaussian, laplace, quantile, huber, modified_huber): ``k`` fp32 roundings,
  ``|got - ref| <= gamma_k |ref|`` with ``gamma_k = k u / (1 - k u)``, ``u = 2^-24``; ``k`` per plane in ``_EXACT_K``.
* planes through ``expc``: ``|got - ref| <= 2 * 2^-23 * (|a| + 4) * M + 2^-126``, ``a`` the row's largest |exp
  argument|, ``M`` the sum of the absolute values of the expression's terms (``_terms`` states each).

Two reference planes are not evaluated literally as the class writes them, because the class's own fp64 expression
cancels far below the kernel's error bound: bernoulli ``den = w ff (1 - ff)`` with ``ff = y - (y - p)`` and poisson
``den = w (y - (y - mu))`` lose ``2^-53 |y|`` absolutely, more than the whole bound once ``p`` or ``mu`` is below
~1e-9 (f < -25). The reference uses the algebraically equal ``w p (1 - p)`` / ``w mu`` from the same class's
``linkinv``; ``test_reference_cancel_free_forms_cpu`` checks that both agree to the class expression's own fp64 error.

Worst measured ``error / (2^-23 (|a| + 4) M)`` on an MI355X (bound: 2), over every shape and weight setting below:

    bernoulli 0.530   quasibinomial 0.492   poisson 0.513   gamma 0.506   tweedie 0.743   xgb_logistic 0.500

(the same figures as a CPU emulation of the kernel's arithmetic: fp32 operations and exp2 of the fp32-rounded product;
the hardware exp2 adds nothing visible). No plane of any distribution came near its bound.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from llama_github_io_amd.models import distributions as D

gpu = pytest.mark.gpu

CODE = {"gaussian": 0, "bernoulli": 1, "quasibinomial": 2, "poisson": 3, "gamma": 4, "tweedie": 5, "laplace": 6,
        "quantile": 7, "huber": 8, "modified_huber": 9, "xgb_logistic": 10}
EXP_DISTS = ("bernoulli", "quasibinomial", "poisson", "gamma", "tweedie", "xgb_logistic")
# fp32 roundings of the kernel's expression per plane (w z, num, den); den == w is stored as is.
#   gaussian   z = y - f (1), w z (2)
#   laplace    z = +-0.5 exact, w z (1)
#   quantile   z = 0.5 (p1 - 1): p1 - 1 (1), the halving is exact, w z (2)
#   huber      as gaussian, plus one where the fp32 and fp64 differences fall on either side of delta (3)
#   modified_huber  s = 2y - 1 = +-1 and yf = s f are exact; w z (1); num = w 2 s (1 - yf): 1 - yf, product (2);
#              den = w (1 - yf) (1 - yf): 1 - yf counted twice, two products (4); -w 4 yf of the other region (1)
_EXACT_K = {"gaussian": (2, 2, 0), "laplace": (1, 1, 0), "quantile": (2, 2, 0), "huber": (3, 3, 0),
            "modified_huber": (1, 2, 4)}
P1 = {"tweedie": 1.5, "quantile": 0.5, "huber": 1.5}
U = 2.0 ** -24
FTZ = 2.0 ** -126
SENTINEL = -12345.678
SEED2 = (12345 * 0x9E3779B1 + 3 * 7919) % (1 << 64)
SHARDS = 64
STEP_GRID, LEAF_GRID = 2048, 4096   # block caps of h2o_gbm_step / h2o_add_leaf (256 threads per block)


# ---------------------------------------------------------------------------------------------------------------
# reference


def _smix(x):
    """splitmix64 finaliser of gbm_kernels.hip on a uint64 array (uint64 array arithmetic wraps)."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def keep_mask(seed, row0, n, rate):
    """Rows the kernel keeps: u = float32(smix(seed ^ (row0 + i)) >> 40) * 2^-24 < rate, compared in fp32."""
    if rate >= 1.0:
        return np.ones(n, bool)
    idx = np.uint64(row0) + np.arange(n, dtype=np.uint64)
    h = _smix(np.uint64(seed) ^ idx) >> np.uint64(40)
    u = h.astype(np.float32) * np.float32(2.0 ** -24)   # 24 bits: exact
    return u < np.float32(rate)


@contextlib.contextmanager
def _exp_clamped_at_80():
    old = D._exp
    D._exp = lambda x: torch.exp(torch.clamp(x, max=80.0))
    try:
        yield
    finally:
        D._exp = old


def _dist(name, p1):
    p1 = float(np.float32(p1))
    d = D.get_distribution("bernoulli" if name == "xgb_logistic" else name, tweedie_power=p1, quantile_alpha=p1)
    d.huber_delta = p1
    return d


def _terms(name, y, f, w, p1):
    """fp64 planes of one distribution from fp32 inputs: dict with z, num, den, the cancel-free den, and per plane the
    magnitude M of the bound (sum of the absolute values of the terms) plus the row's largest |exp argument| a."""
    y, f, w = y.double(), f.double(), w.double()
    d = _dist(name, p1)
    p1 = float(np.float32(p1))
    out = {}
    with _exp_clamped_at_80():
        if name in ("bernoulli", "quasibinomial", "xgb_logistic"):
            fc = f.clamp(min=-80.0)               # exp(-f), argument clamped at 80
            p = d.linkinv(fc)
            z = d.neg_half_gradient(y, fc)
            a = fc.abs()
            m_wz = w * (y.abs() + p)              # w (y - p)
            if name == "xgb_logistic":
                hmin = float(np.float32(1e-16))
                z = y - p
                num = w * z
                den = den_cf = w * torch.clamp(p * (1 - p), min=hmin)
                m_den = w * torch.clamp(p * (1 + p), min=hmin)
            elif name == "bernoulli":
                num, den = d.gamma_num(w, y, z, fc), d.gamma_denom(w, y, z, fc)
                den_cf = w * p * (1 - p)          # the kernel's w p (1 - p): terms w p, w p p
                m_den = w * p * (1 + p)
            else:
                num, den = d.gamma_num(w, y, z, fc), d.gamma_denom(w, y, z, fc)
                den_cf = den                      # the kernel's w ff (1 - ff), ff = y - z: terms |y|, |z| in each factor
                t = y.abs() + z.abs()
                m_den = w * t * (1 + t)
            m_num = m_wz
        elif name == "poisson":
            mu = d.linkinv(f)
            z = d.neg_half_gradient(y, f)
            num, den = d.gamma_num(w, y, z, f), d.gamma_denom(w, y, z, f)
            den_cf = w * mu
            a = f.clamp(max=80.0).abs()
            m_wz, m_num, m_den = w * (y.abs() + mu), w * y.abs(), w * mu
        elif name == "gamma":
            z = d.neg_half_gradient(y, f)
            num, den = d.gamma_num(w, y, z, f), d.gamma_denom(w, y, z, f)
            den_cf = den
            e = D._exp(-f)
            a = (-f).clamp(max=80.0).abs()
            # z = y e - 1; num = w ((y e - 1) + 1); den = w
            m_wz, m_num, m_den = w * (y.abs() * e + 1), w * (y.abs() * e + 2), w
        elif name == "tweedie":
            z = d.neg_half_gradient(y, f)
            num, den = d.gamma_num(w, y, z, f), d.gamma_denom(w, y, z, f)
            den_cf = den
            a1, a2 = (f * (1 - p1)).clamp(max=80.0), (f * (2 - p1)).clamp(max=80.0)
            ea, eb = torch.exp(a1), torch.exp(a2)
            a = torch.maximum(a1.abs(), a2.abs())
            m_wz, m_num, m_den = w * (y.abs() * ea + eb), w * y.abs() * ea, w * eb
        else:
            z = d.neg_half_gradient(y, f)
            num, den = d.gamma_num(w, y, z, f), d.gamma_denom(w, y, z, f)
            den = den_cf = den.expand_as(f) if isinstance(den, torch.Tensor) else den
            a = torch.zeros_like(f)
            m_wz = m_num = m_den = None
    out.update(z=z, wz=w * z, num=num, den=den, den_cf=den_cf, a=a, m=(m_wz, m_num, m_den))
    return out


def reference(name, y, f_new, w_eff, p1):
    """([4, N] fp64 reference planes, [4, N] fp64 tolerances, [4, N] ratio denominators or None)."""
    t = _terms(name, y, f_new, w_eff, p1)
    w = w_eff.double()
    planes = [w, t["wz"], t["num"], t["den_cf"]]
    if name == "xgb_logistic":
        planes[0] = t["den_cf"]                  # p0 = den = the hessian
    ref = torch.stack([p.expand_as(w) for p in planes])
    tol = torch.zeros_like(ref)
    unit = None
    if name in EXP_DISTS:
        unit = torch.zeros_like(ref)
        for c, m in zip((1, 2, 3), t["m"]):
            unit[c] = U * 2 * (t["a"] + 4) * m
        if name == "xgb_logistic":
            unit[0] = unit[3]
        if name == "gamma":
            unit[3] = 0                           # den == w, stored as is
        tol = 2 * unit + FTZ * (unit > 0)
    else:
        for c, k in zip((1, 2, 3), _EXACT_K[name]):
            tol[c] = k * U / (1 - k * U) * ref[c].abs()
    return ref, tol, unit


# ---------------------------------------------------------------------------------------------------------------
# inputs (seeded, CPU)

_PLANT_F = (100.0, -100.0, 80.0, -80.0, 30.0, -30.0, 0.0, 1.0, -1.0)   # +-1: (2y - 1) f == +-1 for y in {0, 1}


@functools.lru_cache(maxsize=None)
def make_inputs(name, N, weights, seed=0):
    """(y, f, w or None) fp32 CPU tensors; f = 8 randn with the edge rows planted at evenly spread positions."""
    g = torch.Generator().manual_seed(1000 * CODE[name] + seed + N % 997)
    f = 8 * torch.randn(N, generator=g)
    if name in ("bernoulli", "modified_huber", "xgb_logistic"):
        y = (torch.rand(N, generator=g) < 0.5).float()
    elif name == "quasibinomial":
        y = 2.4 * torch.rand(N, generator=g) - 0.7          # inside and outside [0, 1]
        y[::5] = (y[::5] > 0.5).float()                      # and exactly 0 / 1
    elif name in ("poisson", "tweedie"):
        y = torch.poisson(torch.full((N,), 1.5), generator=g)
    elif name == "gamma":
        y = torch.empty(N).exponential_(1.0, generator=g) + 0.01
    else:
        y = 3 * torch.randn(N, generator=g)
    plants = [("f", v) for v in _PLANT_F] + [("f==y", None)]
    if name in ("gaussian", "laplace", "quantile", "huber"):
        plants += [("dy", (2.25, 1.5)), ("dy", (-3.5, -1.5))]   # |y - f| == delta == 1.5 exactly (multiples of 0.25)
    stride = max(1, N // (len(plants) + 1))
    for j, (kind, v) in enumerate(plants):
        i = j * stride + (stride // 2 if N > len(plants) else 0)
        if i >= N:
            break
        if kind == "f":
            f[i] = v
        elif kind == "f==y":
            f[i] = y[i]
        else:
            f[i], y[i] = v[0], v[0] + v[1]
    w = None
    if weights:
        w = 3 * torch.rand(N, generator=g)
        w[::13] = 0
    return y, f, w


def _w_eff(w, N, rate=1.0, seed=0, row0=0):
    w = torch.ones(N) if w is None else w
    return w * torch.from_numpy(keep_mask(seed, row0, N, rate)).float()


# ---------------------------------------------------------------------------------------------------------------
# CPU-only checks of the reference


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("name,p1", [(n, P1.get(n, 0.0)) for n in CODE if n != "xgb_logistic"]
                         + [("tweedie", 1.2), ("tweedie", 1.9), ("quantile", 0.1), ("quantile", 0.9)])
def test_reference_matches_eager_path_cpu(name, p1, weights):
    """The fp64 reference == what GBMTrainer._prepare's eager path writes into aux (the same Distribution calls in
    fp32), to fp32 rounding: per plane 4 u (|a| + 4) M with M the terms of the EAGER expression (the class's
    den = w ff (1 - ff), ff = y - z and den = w (y - z) cancel in fp32), where the clamp at 80 is not reached."""
    y, f, w = make_inputs(name, 4099, weights)
    w = _w_eff(w, 4099)
    d = _dist(name, p1)
    z = d.neg_half_gradient(y, f)
    eager = torch.stack([w, w * z, d.gamma_num(w, y, z, f), d.gamma_denom(w, y, z, f).expand_as(f)]).double()
    ref, tol, _ = reference(name, y, f, w, p1)
    t = _terms(name, y, f, w, p1)
    ok = t["a"] < 80 if name in EXP_DISTS else torch.ones_like(f, dtype=torch.bool)
    assert ok.sum() >= 4099 - 4
    if name in EXP_DISTS:
        wd, yz = w.double(), y.double().abs() + t["z"].abs()
        m_den = {"bernoulli": wd * yz * (1 + yz), "quasibinomial": wd * yz * (1 + yz), "poisson": wd * yz}.get(name, t["m"][2])
        for c, m in zip((1, 2, 3), (t["m"][0], t["m"][1], m_den)):
            lim = 4 * U * (t["a"] + 4) * m + FTZ
            assert bool(((eager[c] - ref[c]).abs() <= lim)[ok].all()), (name, c)
    else:
        for c in (1, 2, 3):
            assert bool(((eager[c] - ref[c]).abs() <= tol[c] + 0.0).all()), (name, c)
    assert torch.equal(eager[0], ref[0])


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_reference_cancel_free_forms_cpu(name):
    """w p (1 - p) and w mu are the class's gamma_denom up to that expression's own fp64 cancellation."""
    y, f, w = make_inputs(name, 4099, True)
    t = _terms(name, y, f, w, 0.0)
    yz = y.double().abs() + t["z"].abs()
    lim = 4 * 2.0 ** -53 * w.double() * (yz * (1 + yz) if name == "bernoulli" else yz)
    assert bool(((t["den"] - t["den_cf"]).abs() <= lim).all())
    low = (f < -40) & (w > 0)                     # there the class's form is 0 for y >= 1; the kernel's is not
    assert bool(low.any()) and bool((t["den_cf"][low] > 0).all())


def test_sampling_hash_reference_cpu():
    """The NumPy hash is splitmix64 (first output of the generator seeded with 0), is keyed by the global row, and
    keeps a share within 2.5 binomial standard deviations of the rate for every seed, rate and row0 the GPU tests use."""
    assert int(_smix(np.zeros(1, np.uint64))[0]) == 0xE220A8397B1DCDAF

    def smix_int(x):                              # the same mixer on Python integers
        m = (1 << 64) - 1
        x = (x + 0x9E3779B97F4A7C15) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)
    for s, r0, i in [(0, 0, 5), (SEED2, 0, 77), (SEED2, 5 * 10 ** 9, 123456), ((1 << 64) - 1, 3, 9)]:
        want = np.float32(smix_int(s ^ (r0 + i)) >> 40) * np.float32(2.0 ** -24) < np.float32(0.3)
        assert keep_mask(s, r0, i + 1, 0.3)[i] == want
    n = 300001
    for seed in (0, SEED2):
        for row0 in (0, 5 * 10 ** 9):
            full = keep_mask(seed, row0, n, 0.8)
            assert np.array_equal(keep_mask(seed, row0 + 1000, 500, 0.8), full[1000:1500])
            for rate in (0.8, 0.3, 0.01):
                share = keep_mask(seed, row0, n, rate).mean()
                assert abs(share - rate) <= 2.5 * np.sqrt(rate * (1 - rate) / n), (seed, row0, rate, share)


# ---------------------------------------------------------------------------------------------------------------
# GPU


def _dev():
    return torch.device("cuda", 0)


def run_step(name, y, f, w=None, vals=None, leaf=None, rate=1.0, seed=0, p1=0.0, skip=0, row0=0, amax=None):
    """One h2o_gbm_step launch on sentinel-filled planes -> (aux [4, N], f, amax [64, 4] as fp32), all on the CPU."""
    from llama_github_io_amd.ops import _native as nat
    dev = _dev()
    N = y.numel()
    yd, fd = y.to(dev), f.clone().to(dev)
    wd = None if w is None else w.to(dev)
    vd = None if vals is None else vals.to(dev)
    ld = None if leaf is None else leaf.to(dev)
    aux = torch.full((4, N), SENTINEL, dtype=torch.float32, device=dev)
    am = torch.zeros(4 * SHARDS, dtype=torch.int32, device=dev) if amax is None else amax
    nat.call("h2o_gbm_step", N, row0, CODE[name], yd.data_ptr(), nat.ptr(wd), fd.data_ptr(), nat.ptr(vd), nat.ptr(ld),
             float(rate), int(seed), float(p1), aux.data_ptr(), am.data_ptr(), int(skip), nat.stream_ptr(dev))
    torch.cuda.synchronize()
    return aux.cpu(), fd.cpu(), am.cpu().view(torch.float32).view(SHARDS, 4).clone()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _shard_maxima(planes, grid_cap):
    """fp32 max |.| per (shard, plane) of [4, N] planes: row i belongs to block (i // 256) % grid, shard block & 63."""
    N = planes.shape[1]
    grid = max(1, min((N + 255) // 256, grid_cap))
    nb = (N + 255) // 256
    a = np.zeros((4, nb * 256), np.float32)
    a[:, :N] = planes.abs().numpy()
    chunk = a.reshape(4, nb, 256).max(2)          # max |.| of each 256-row chunk
    shard = (np.arange(nb) % grid) & (SHARDS - 1)
    out = np.zeros((SHARDS, 4), np.float32)
    for c in range(4):
        np.maximum.at(out[:, c], shard, chunk[c])
    return torch.from_numpy(out)


def check_planes(name, aux, ref, tol, unit, w_eff, label=""):
    err = (aux.double() - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        c, i = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{name} {label}: plane {c} row {i}: got {aux[c, i].item()!r} ref {ref[c, i].item()!r} "
                             f"err {err[c, i].item():.3e} tol {tol[c, i].item():.3e}; {int(bad.sum())} rows off")
    if unit is not None:
        sel = unit > 1e-30                       # ratios where the flush-to-zero allowance plays no part
        if bool(sel.any()):
            print(f"RATIO {name} {label} {float((err[sel] / unit[sel]).max()):.3f}")
    # rows the sample or a zero weight dropped: exact zeros (every num / den here is a multiple of w)
    zero = w_eff == 0
    assert bool((aux[:, zero] == 0).all()), (name, label)


def check_maxima(name, shards, stored, ref, tol):
    """stored: the [4, N] planes the launch wrote (skip = 0)."""
    want = _shard_maxima(stored, STEP_GRID)
    assert torch.equal(_bits(shards), _bits(want)), name          # every shard, so the block -> shard map too
    fold = shards.max(0).values
    assert torch.equal(_bits(fold), _bits(stored.abs().max(1).values)), name
    assert bool((fold[:, None] >= stored.abs()).all()), name      # what k_qscale relies on
    # within the plane tolerance of the reference maximum: with i = argmax |ref|, j = argmax |got|,
    # |ref_i| - tol_i <= |got_i| <= fold = |got_j| <= |ref_j| + tol_j <= |ref_i| + tol_j
    for c in range(4):
        i, j = int(ref[c].abs().argmax()), int(stored[c].abs().argmax())
        d = float(fold[c].double() - ref[c].abs().max())
        assert -float(tol[c, i]) <= d <= float(tol[c, j]), (name, c, d)


def _step_case(name, N, weights, p1, rate=1.0, seed=0, pending=False, label=""):
    y, f, w = make_inputs(name, N, weights)
    vals = leaf = None
    f_new = f
    if pending:
        g = torch.Generator().manual_seed(N + 7)
        vals = 0.3 * torch.randn(37, generator=g)
        leaf = torch.randint(0, 37, (N,), generator=g, dtype=torch.int32)
        f_new = f + vals[leaf.long()]            # the fp32 sum
    we = _w_eff(w, N, rate, seed)
    ref, tol, unit = reference(name, y, f_new, we, p1)
    aux, f_out, shards = run_step(name, y, f, w, vals, leaf, rate, seed, p1)
    assert torch.equal(_bits(f_out), _bits(f_new)), (name, label)
    check_planes(name, aux, ref, tol, unit, we, label or f"N={N} w={weights} p1={p1}")
    check_maxima(name, shards, aux, ref, tol)


_GRID = [(n, P1.get(n, 0.0)) for n in CODE] + [("tweedie", 1.2), ("tweedie", 1.9), ("quantile", 0.1), ("quantile", 0.9)]


@gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257])
def test_step_planes_partial_waves_and_blocks(N):
    for name, p1 in _GRID:
        for weights in (False, True):
            _step_case(name, N, weights, p1, rate=0.8 if weights else 1.0, seed=SEED2)


@gpu
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("name,p1", _GRID)
def test_step_planes_shards_wrap(name, p1, weights):
    """70 001 rows = 274 blocks: the shard index wraps past 64. Weighted runs are also sampled (w_eff = w * mask)."""
    _step_case(name, 70001, weights, p1, rate=0.7 if weights else 1.0, seed=SEED2)


@gpu
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("name", ["bernoulli", "tweedie"])
def test_step_planes_grid_stride_second_iteration(name, weights):
    """524 288 + 257 rows: 2048 blocks, the loop runs a second time for the first 257 threads only; with a pending
    tree (vals / leaf), so the f update is checked there too."""
    _step_case(name, 524288 + 257, weights, P1.get(name, 0.0), pending=True)


@gpu
@pytest.mark.parametrize("name", ["gaussian", "poisson", "modified_huber"])
def test_step_pending_update(name):
    N = 70001
    _step_case(name, N, True, 0.0, pending=True)
    y, f, w = make_inputs(name, N, True)
    leaf = torch.randint(0, 37, (N,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    _, f_out, _ = run_step(name, y, f, w, torch.zeros(37), leaf)
    assert torch.equal(_bits(f_out), _bits(f))
    _, f_out, _ = run_step(name, y, f, w)       # no pending tree: f is not written
    assert torch.equal(_bits(f_out), _bits(f))


@gpu
@pytest.mark.parametrize("name,weights", [("bernoulli", True), ("tweedie", False), ("xgb_logistic", False)])
def test_step_skip_bits(name, weights):
    """skip bit 0 / 2: planes 0 / 2 are not stored, everything else (the four maxima included: the histogram scale
    of a skipped plane is still used) is the skip = 0 run bit for bit."""
    N = 70001
    y, f, w = make_inputs(name, N, weights)
    kw = dict(rate=0.8, seed=SEED2, p1=P1.get(name, 0.0))
    full, _, shards0 = run_step(name, y, f, w, **kw)
    assert not bool((full == SENTINEL).any())
    for skip in (0, 1, 4, 5):
        aux, _, shards = run_step(name, y, f, w, skip=skip, **kw)
        for c in range(4):
            if (c == 0 and skip & 1) or (c == 2 and skip & 4):
                assert bool((aux[c] == SENTINEL).all()), (skip, c)
            else:
                assert torch.equal(_bits(aux[c]), _bits(full[c])), (skip, c)
        assert torch.equal(_bits(shards), _bits(shards0)), skip
        assert torch.equal(_bits(shards.max(0).values), _bits(full.abs().max(1).values)), skip


@gpu
def test_step_maxima_accumulate_and_single_row():
    """A second launch without zeroing accumulates the max of both launches; N = 1 publishes its one row."""
    dev = _dev()
    N = 70001
    y, f, w = make_inputs("gaussian", N, True)
    amax = torch.zeros(4 * SHARDS, dtype=torch.int32, device=dev)
    a1, _, s1 = run_step("gaussian", y, f, w, amax=amax)
    a2, _, s2 = run_step("gaussian", 5 * y, -f, 0.5 * w, amax=amax)
    m1, m2 = _shard_maxima(a1, STEP_GRID), _shard_maxima(a2, STEP_GRID)
    assert torch.equal(_bits(s1), _bits(m1))
    assert torch.equal(_bits(s2), _bits(torch.maximum(m1, m2)))
    assert bool((m2[:, 1] > m1[:, 1]).any()) and bool((m1[:, 0] > m2[:, 0]).any())   # both launches matter
    y1, f1 = torch.tensor([2.5]), torch.tensor([-0.75])
    aux, _, s = run_step("gaussian", y1, f1, torch.tensor([3.0]))
    assert aux[:, 0].tolist() == [3.0, 9.75, 9.75, 3.0]
    assert s[0].tolist() == [3.0, 9.75, 9.75, 3.0] and bool((s[1:] == 0).all())


@gpu
@pytest.mark.parametrize("seed", [0, SEED2])
@pytest.mark.parametrize("rate", [0.8, 0.3, 0.01])
def test_step_sampling_mask(rate, seed):
    N = 300001
    y, f, _ = make_inputs("gaussian", N, False)
    aux, _, _ = run_step("gaussian", y, f, rate=rate, seed=seed)
    keep = keep_mask(seed, 0, N, rate)
    assert np.array_equal((aux[0] != 0).numpy(), keep)
    assert bool((aux[0][torch.from_numpy(keep)] == 1).all())
    assert abs(keep.mean() - rate) <= 5 * np.sqrt(rate * (1 - rate) / N)


@gpu
def test_step_sample_rate_one_keeps_every_weight():
    y, f, w = make_inputs("gaussian", 70001, True)
    aux, _, _ = run_step("gaussian", y, f, w, rate=1.0, seed=SEED2)
    assert torch.equal(_bits(aux[0]), _bits(w))
    aux, _, _ = run_step("gaussian", y, f, None, rate=1.0, seed=SEED2)
    assert bool((aux[0] == 1).all())


@gpu
def test_step_row0_shard_contract():
    """A run on rows [r0, r0 + n) with row0 = r0 writes the slice of the full run (a row-sharded training samples
    the rows of the single-GPU one); row0 = 5e9 does not wrap at 32 bits."""
    N, n = 170005, 70001
    y, f, w = make_inputs("bernoulli", N, True)
    full, _, _ = run_step("bernoulli", y, f, w, rate=0.3, seed=SEED2)
    for r0 in (0, 100003):
        part, _, _ = run_step("bernoulli", y[r0:r0 + n].clone(), f[r0:r0 + n].clone(), w[r0:r0 + n].clone(), rate=0.3,
                              seed=SEED2, row0=r0)
        assert torch.equal(_bits(part), _bits(full[:, r0:r0 + n])), r0
    n = 70001
    r0 = 5 * 10 ** 9
    y, f, _ = make_inputs("gaussian", n, False)
    aux, _, _ = run_step("gaussian", y, f, rate=0.3, seed=SEED2, row0=r0)
    assert np.array_equal((aux[0] != 0).numpy(), keep_mask(SEED2, r0, n, 0.3))
    assert not np.array_equal(keep_mask(SEED2, r0, n, 0.3), keep_mask(SEED2, r0 % (1 << 32), n, 0.3))


@gpu
def test_add_leaf_stride():
    """h2o_add_leaf past its 4096-block cap: bit-equal to the fp32 sum; fstride = 3 touches column 0 only."""
    from llama_github_io_amd.ops import _native as nat
    dev = _dev()
    N = 1048576 + 257
    g = torch.Generator().manual_seed(11)
    f = 8 * torch.randn(N, generator=g)
    vals = torch.randn(37, generator=g)
    leaf = torch.randint(0, 37, (N,), generator=g, dtype=torch.int32)
    want = f + vals[leaf.long()]
    vd, ld = vals.to(dev), leaf.to(dev)
    fd = f.to(dev)
    nat.call("h2o_add_leaf", N, fd.data_ptr(), 1, vd.data_ptr(), ld.data_ptr(), nat.stream_ptr(dev))
    assert torch.equal(_bits(fd.cpu()), _bits(want))
    f3 = torch.randn(N, 3, generator=g)
    f3[:, 0] = f
    fd = f3.to(dev)
    nat.call("h2o_add_leaf", N, fd.data_ptr(), 3, vd.data_ptr(), ld.data_ptr(), nat.stream_ptr(dev))
    got = fd.cpu()
    assert torch.equal(_bits(got[:, 0]), _bits(want))
    assert torch.equal(_bits(got[:, 1:]), _bits(f3[:, 1:]))


@gpu
@pytest.mark.parametrize("N", [1, 257, 524545])
def test_amax_planes(N):
    """h2o_amax on arbitrary [4, N] planes: the folded bits are the fp32 max |.|; NaN is ignored, inf is kept."""
    from llama_github_io_amd.ops import _native as nat
    dev = _dev()
    g = torch.Generator().manual_seed(N)
    aux = torch.randn(4, N, generator=g) * torch.tensor([1.0, 300.0, 1.0, 1e-3])[:, None]
    aux[2] = 0
    aux[0, N // 2] = float("nan")
    aux[1, N // 3] = float("-inf")
    if N > 1:
        aux[3, N - 1] = -7.5                      # the largest |.| is negative and sits in the last, partial block
    ad = aux.to(dev)
    amax = torch.zeros(4 * SHARDS, dtype=torch.int32, device=dev)
    nat.call("h2o_amax", ad.data_ptr(), N, amax.data_ptr(), nat.stream_ptr(dev))
    fold = amax.cpu().view(torch.float32).view(SHARDS, 4).max(0).values
    a = aux.abs()
    want = torch.where(torch.isnan(a), torch.zeros_like(a), a).max(1).values
    assert torch.equal(_bits(fold), _bits(want)), (fold, want)
    assert want[1] == float("inf") and want[2] == 0 and (N == 1 or want[3] == 7.5)


def _qscale_reference(m, N, fpack):
    """The comment above k_qscale in fp64. PACK_MAX / PACK_SHIFT: the defines of csrc/tree_kernels.hip."""
    PACK_MAX, PACK_SHIFT = 63488.0, 48.0
    m = [float(v) for v in m]
    ok = [v > 0 and v == v and v != float("inf") for v in m]
    qs = np.zeros(13)
    for c in (0, 1):
        sc = 2.0 ** 40 / m[c] if ok[c] else 1.0
        qs[c], qs[2 + c] = sc, 1.0 / sc
    sp = 1.0 if not ok[1] else (0.99 * 2.0 ** 31 / (PACK_MAX * m[1]) if fpack else 2.0 ** 30 / m[1])
    qs[4], qs[5] = sp, 1.0 / sp
    lb = max(61 - int(N).bit_length(), 8)
    assert 2 ** lb * N < 2 ** 62
    for c in (2, 3):
        sc = 2.0 ** lb / m[c] if ok[c] else 1.0
        qs[6 + c - 2], qs[8 + c - 2] = sc, 1.0 / sc
    sw = 0.99 * 2.0 ** 32 / (PACK_MAX * m[0]) if (fpack and ok[0]) else 1.0
    qs[10], qs[11], qs[12] = sw, 1.0 / sw, 32.0 if fpack else PACK_SHIFT
    return qs


@gpu
@pytest.mark.parametrize("fpack", [0, 1])
@pytest.mark.parametrize("N", [1, 2 ** 20 - 1, 2 ** 20, 11000000])
def test_qscale_formulas_and_reset(N, fpack):
    from llama_github_io_amd.ops import _native as nat
    dev = _dev()
    good = np.array([3.5, 1234.5, 0.0078125 * 0.9, 9.9e20], np.float32)
    cases = [good] + [np.full(4, v, np.float32) for v in (0.0, np.nan, np.inf)] + [
        np.array([np.inf, 2.0, 0.0, 5.0], np.float32)]
    for m in cases:
        sh = np.zeros((SHARDS, 4), np.float32)
        sh[63] = m                                # the largest value sits in the last shard
        fin = np.isfinite(m)
        sh[0, fin], sh[17, fin] = 0.5 * m[fin], 0.25 * m[fin]
        amax = torch.from_numpy(sh.view(np.int32).reshape(-1).copy()).to(dev)
        qs = torch.full((16,), -1.0, dtype=torch.float64, device=dev)
        counters = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device=dev)
        nat.call("h2o_qscale", amax.data_ptr(), qs.data_ptr(), counters.data_ptr(), N, fpack, nat.stream_ptr(dev))
        got = qs.cpu().numpy()
        want = _qscale_reference(m, N, fpack)
        np.testing.assert_allclose(got[:13], want, rtol=4 * 2.0 ** -53, atol=0, err_msg=str((m, N, fpack)))
        assert np.all(got[13:] == -1.0)
        assert not bool(amax.cpu().any()) and not bool(counters.cpu().any())
        if not np.isfinite(m).all() or not m.all():
            bad = ~(np.isfinite(m) & (m > 0))
            for c in range(4):
                if bad[c]:
                    assert got[[0, 1, 6, 7][c]] == 1.0

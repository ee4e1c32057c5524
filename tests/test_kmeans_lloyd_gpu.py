"""The K-Means Lloyd kernels against fp64 references (csrc/kmeans_mfma.hip, csrc/kmeans_kernels.hip; inputs, case
table, references and bounds in kmeans_cases.py, which test_kmeans_lloyd_paths.py anchors on the CPU).

Exact cases (integer inputs on which fp32 is exact, so every check is an equality). ``h2o_kmeans_mfma`` is launched on
buffers of the test's own with an explicit grid, once with and once without ``assign``; each launch must give

* ``assign`` equal to the first minimum of the fp64 distances in every row (ties -> the smaller center index: the
  in-lane scan, the ``xor 16`` and ``xor 32`` butterfly steps and the scan across center tiles each meet ties made by
  duplicated centers), ``mind`` bit-equal to the fp64 minimum;
* every element of the ``[grid][KT*16][PT*16]`` slabs written (they are pre-filled with NaN), each block's slab equal
  to the fp64 sums / counts of that block's rows, padding centers and padding dims exactly 0, blocks without rows all 0;
* the 64 sentinel elements behind ``assign`` and ``mind`` untouched; the two launches bit-identical.

Which kernel a case family reaches (KT, PS, PT; variant = k_lloyd_mfma4 'occ4' or k_lloyd_mfma 'occ3'; km_stride):

    K{16,17|32,33|64} x P{12,16,24,28,32,44,60,64}, K{1,3,17,64}P4    all 24 instantiations, N = 641 / 805, grid 1 / 2
    K10P20 (1,6,2) occ4 plain 21     K16P16 (1,4,2) occ4 pad 17      K16P24 (1,6,2) occ4 plain 25
    K3P12  (1,4,1) occ4 pad 17       K32P32 (2,8,3) occ3 pad 49      K64P64 (4,16,5) occ3 plain 65
        each at N = 805, 641 with grid 1, 2, 3 and N = 1541 with grid 3: waves with 2 to 4 tiles, a 37-, 1- or 5-row
        last tile that one wave of a block gets, idle waves
    K10P20, K33P44 ((4,16,3) occ3 pad 49) at N = 1, 15, 16, 17, 63, 64, 65 (grid 1) and N = 100 at grid 4
    *-zero: a far center that holds three zero-weight rows (rows, but count 0 and sums 0)
    H2O_KM_OCC4=0 (one child process): K10P20, K16P24, K3P12 on k_lloyd_mfma<1, 6|4, 2|1>, strides 49, 49, 17

Scalar kernels on the same kind of inputs: k_kmeans_step and k_kmeans_assign called directly at P in {1, 3, 5, 13}
x K in {1, 6, 65, 100} x N in {1, 255, 256, 257, 700}; kmeans_step with H2O_KMEANS_MFMA=0 at P = 20; the sort-based
torch segment sums (K = 200, P = 50, 92224 B of dynamic LDS in k_kmeans_assign); the largest dynamic LDS the launchers'
guard admits at P = 120: k_kmeans_step at K = 60 (154752 B, the largest kmeans_step itself sends to the kernel) and
K = 78 (163392 B), k_kmeans_assign at K = 83 (163744 B, 96 bytes under the device's 163840 per block, which is read
from the device properties; the HIP runtime asks for no opt-in attribute above 64 KiB). k_kmeans_update and
kmeans_lloyd_step: bit-equal to the model's torch update.

Rounding cases (randn + 100, float weights, N = 805 at grid 1), worst err / bound on an MI355X, bounds as derived in
kmeans_cases.py (a ratio above 1 is a failure; the tests print ``KMRATIO <case> <quantity> <ratio>``):

    kernel (bound of the distance)          shape    dist   assign  sums   cnt
    k_lloyd_mfma4 / k_lloyd_mfma  (B)       K10P20   0.073  0.035   0.129  0.095
                                            K32P32   0.074  0.028   0.237  0.138
                                            K64P64   0.059  0.019   0.251  0.187
    k_kmeans_step  ((P + 3) u D)            K10P20   0.181  0       0.065  0.046
                                            K32P32   0.141  0       0.125  0.055
                                            K64P64   0.105  0       0.194  0.069
    k_kmeans_assign  ((P + 3) u D)          K10P20   0.181  0       -      -
                                            K32P32   0.141  0       -      -
                                            K64P64   0.105  0       -      -

(The sums and counts of k_kmeans_step are held to the same (n_c + 4) u bounds as the MFMA kernel's; the scalar kernels
chose the fp64 argmin in every row.) The whole file takes about 7 s, 2 s of them the child process.

Bugs these tests found: none. Launches with more than 64 KiB of dynamic LDS, up to 163744 B, succeed as they are.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_cases as kc

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


def _dev(inp):
    return (torch.from_numpy(inp.X).to(dev), torch.from_numpy(inp.C).to(dev),
            None if inp.w is None else torch.from_numpy(inp.w).to(dev))


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------- A / B: the MFMA kernel, exact
def test_native_shape_table_matches_python():
    from llama_github_io_amd.ops.dense import _mfma_shape
    for K in range(0, 67):
        for P in range(0, 67):
            assert _mfma_shape(K, P) == kc.mfma_shape(K, P), (K, P)
    assert {_mfma_shape(c.K, c.P) for c in kc.CASES} == set(kc.CLASSES)


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_mfma_exact(name):
    bad = kc.run_exact_case(kc.case(name), dev)
    assert not bad, "\n".join(bad)


def _check_step(out, ref, K, P, need_assign=True):
    a, d, sums, cnt = out
    if need_assign:
        assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy(), ref.assign)
    else:
        assert a is None
    assert d.dtype == torch.float32 and np.array_equal(_f64(d), ref.mind)
    assert sums.shape == (K, P) and sums.dtype == torch.float64 and np.array_equal(sums.cpu().numpy(), ref.sums)
    assert cnt.shape == (K,) and cnt.dtype == torch.float64 and np.array_equal(cnt.cpu().numpy(), ref.cnt)


def test_kmeans_step_noncontiguous_fp64_input(monkeypatch):
    from llama_github_io_amd.ops.dense import kmeans_step
    monkeypatch.setenv("H2O_KMEANS_MFMA", "1")
    c = kc.case("K10P20-N805-g1")
    inp, ref = kc.make_inputs(c), kc.case_reference(c)
    wide = torch.full((c.N, c.P + 7), 99.0, dtype=torch.float64, device=dev)
    wide[:, 3:3 + c.P] = torch.from_numpy(inp.X).to(dev)
    X = wide[:, 3:3 + c.P]
    assert not X.is_contiguous() and X.dtype == torch.float64
    Cd = torch.from_numpy(inp.C).to(dev).double()
    wd = torch.from_numpy(inp.w).to(dev).double()
    _check_step(kmeans_step(X, Cd, wd), ref, c.K, c.P)


@pytest.mark.parametrize("name", ["K10P20-N805-g1-zero", "K64P64-N1541-g3"])
def test_kmeans_step_without_assign(name, monkeypatch):
    from llama_github_io_amd.ops.dense import kmeans_step
    monkeypatch.setenv("H2O_KMEANS_MFMA", "1")
    c = kc.case(name)
    X, C, w = _dev(kc.make_inputs(c))
    _check_step(kmeans_step(X, C, w, need_assign=False), kc.case_reference(c), c.K, c.P, need_assign=False)
    _check_step(kmeans_step(X, C, w), kc.case_reference(c), c.K, c.P)


def test_occ4_off_variant_in_a_child():
    """H2O_KM_OCC4 is read once per process: one fresh child runs the exact multi-tile cases of the occ4 shapes on the
    3-waves-per-SIMD kernel and exits non-zero on any inequality."""
    env = dict(os.environ, H2O_KM_OCC4="0", H2O_KMEANS_MFMA="1")
    r = subprocess.run([sys.executable, os.path.abspath(kc.__file__), "occ4-child"], timeout=120, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"OCC4OFF {len(kc.occ4_off_cases())} cases, 0 violations" in r.stdout


# ---------------------------------------------------------------- C: scalar kernels and fallbacks, exact
def _raw_scalar(X, C, w, step):
    """h2o_kmeans_step / h2o_kmeans_assign on sentinel-padded buffers and NaN-filled slabs."""
    from llama_github_io_amd.ops import _native as nat
    N, P = X.shape
    K = C.shape[0]
    a = torch.full((N + kc.PAD,), kc.ASSIGN_SENTINEL, dtype=torch.int32, device=dev)
    d = torch.full((N + kc.PAD,), kc.MIND_SENTINEL, dtype=torch.float32, device=dev)
    if not step:
        nat.call("h2o_kmeans_assign", X.data_ptr(), N, P, C.data_ptr(), K, a.data_ptr(), d.data_ptr(),
                 nat.stream_ptr(dev))
        return a.cpu().numpy(), d.cpu().numpy(), None
    G = (N + 255) // 256
    slab = torch.full((G, K, P + 1), float("nan"), dtype=torch.float32, device=dev)
    nat.call("h2o_kmeans_step", X.data_ptr(), N, P, C.data_ptr(), K, 0 if w is None else w.data_ptr(), a.data_ptr(),
             d.data_ptr(), slab.data_ptr(), nat.stream_ptr(dev))
    return a.cpu().numpy(), d.cpu().numpy(), slab.cpu().numpy()


def _check_scalar(tag, inp, ref, a, d, slab):
    N, P = inp.X.shape
    K = inp.C.shape[0]
    assert np.array_equal(a[:N], ref.assign), tag
    assert np.array_equal(d[:N].view(np.uint32), ref.mind.astype(np.float32).view(np.uint32)), tag
    assert (a[N:] == kc.ASSIGN_SENTINEL).all() and (d[N:] == np.float32(kc.MIND_SENTINEL)).all(), tag
    if slab is None:
        return
    assert not np.isnan(slab).any(), tag
    for b in range(slab.shape[0]):
        r = slice(256 * b, min(N, 256 * b + 256))
        sb, cb = kc.segment_sums(inp.X[r], None if inp.w is None else inp.w[r], ref.assign[r], K)
        assert np.array_equal(slab[b, :, :P].astype(np.float64), sb), (tag, b)
        assert np.array_equal(slab[b, :, P].astype(np.float64), cb), (tag, b)


SCALAR_N = (1, 255, 256, 257, 700)


@pytest.mark.parametrize("K", [1, 6, 65, 100])
@pytest.mark.parametrize("P", [1, 3, 5, 13])
def test_scalar_step_kernel_exact(P, K):
    from llama_github_io_amd.ops.dense import kmeans_step
    for i, N in enumerate(SCALAR_N):
        inp = kc.exact_inputs(K, P, N, ("int", "none")[i & 1], seed=100 * K + 10 * P + i)
        ref = kc.reference(inp.X, inp.C, inp.w)
        X, C, w = _dev(inp)
        _check_scalar((K, P, N), inp, ref, *_raw_scalar(X, C, w, step=True))
        _check_step(kmeans_step(X, C, w), ref, K, P)            # P % 4 != 0: the scalar kernel behind the op


def test_scalar_assign_kernel_exact():
    from llama_github_io_amd.ops.dense import kmeans_assign
    K, P = 100, 13
    for i, N in enumerate(SCALAR_N):
        inp = kc.exact_inputs(K, P, N, "none", seed=7 + i)
        ref = kc.reference(inp.X, inp.C, None)
        X, C, _ = _dev(inp)
        _check_scalar((K, P, N), inp, ref, *_raw_scalar(X, C, None, step=False))
        a, d = kmeans_assign(X, C)
        assert np.array_equal(a.cpu().numpy(), ref.assign) and np.array_equal(_f64(d), ref.mind)


@pytest.mark.parametrize("name", ["K10P20-N805-g1", "K10P20-N805-g1-zero"])
def test_scalar_step_when_mfma_is_switched_off(name, monkeypatch):
    from llama_github_io_amd.ops.dense import kmeans_step
    monkeypatch.setenv("H2O_KMEANS_MFMA", "0")                   # read per call
    c = kc.case(name)
    inp, ref = kc.make_inputs(c), kc.case_reference(c)
    X, C, w = _dev(inp)
    _check_step(kmeans_step(X, C, w), ref, c.K, c.P)
    _check_scalar(name, inp, ref, *_raw_scalar(X, C, w, step=True))


def test_torch_segment_sum_fallback_exact():
    from llama_github_io_amd.ops import dense
    K, P, N = 200, 50, 700
    assert K * (P + 1) > 8192 and dense._mfma_shape(K, P) is None
    assert (K * P + 256 * (P + 1)) * 4 <= dense._KM_LDS_MAX      # k_kmeans_assign, then torch sums
    inp = kc.exact_inputs(K, P, N, "int", seed=5)
    ref = kc.reference(inp.X, inp.C, inp.w)
    X, C, w = _dev(inp)
    _check_step(dense.kmeans_step(X, C, w), ref, K, P)
    inp1 = kc.exact_inputs(K, P, N, "none", seed=6)
    X, C, _ = _dev(inp1)
    _check_step(dense.kmeans_step(X, C, None), kc.reference(inp1.X, inp1.C, None), K, P)


def test_lds_guard_and_largest_admitted_shape():
    from llama_github_io_amd.ops import _native as nat
    from llama_github_io_amd.ops import dense
    lib = nat.hip()
    limit = int(lib.h2o_kmeans_lds_limit())
    per_block = int(torch.cuda.get_device_properties(0).shared_memory_per_block)
    print("KMLDS guard", limit, "device per-block", per_block)
    assert limit == dense._KM_LDS_MAX and limit <= per_block
    # the launchers refuse (without launching) the first shape past the guard
    P, N = 120, 300
    step_bytes = lambda K: (K * P + 256 * (P + 1) + 512) * 4       # noqa: E731
    Ks = max(k for k in range(1, 200) if step_bytes(k) <= limit)
    Ka = max(k for k in range(1, 200) if lib.h2o_kmeans_lds_bytes(k, P) <= limit)
    assert lib.h2o_kmeans_lds_bytes(Ka, P) == (Ka * P + 256 * (P + 1)) * 4 and (Ks, Ka) == (78, 83)
    # (buffers of the full size of the refused shape: were the guard to admit it, nothing is touched out of bounds)
    s = nat.stream_ptr(dev)
    for K, step in ((Ks + 1, True), (Ka + 1, False)):
        X = torch.zeros(N, P, device=dev)
        C = torch.zeros(K, P, device=dev)
        a = torch.zeros(N, dtype=torch.int32, device=dev)
        d = torch.zeros(N, device=dev)
        slab = torch.zeros((N + 255) // 256, K, P + 1, device=dev)
        if step:
            rc = lib.h2o_kmeans_step(X.data_ptr(), N, P, C.data_ptr(), K, 0, a.data_ptr(), d.data_ptr(),
                                     slab.data_ptr(), s)
        else:
            rc = lib.h2o_kmeans_assign(X.data_ptr(), N, P, C.data_ptr(), K, a.data_ptr(), d.data_ptr(), s)
        torch.cuda.synchronize()
        assert rc != 0, (K, step)
    # the largest shapes the guard admits run and are exact (more than 64 KiB of dynamic LDS); P = 120: distances up
    # to 120 * 256 and sums far below 2^24, still exact. K = 60 is the largest kmeans_step itself sends to the kernel
    for K in (60, Ks):
        assert 64 * 1024 < step_bytes(K) <= limit
        inp = kc.exact_inputs(K, P, N, "int", seed=K)
        ref = kc.reference(inp.X, inp.C, inp.w)
        X, C, w = _dev(inp)
        _check_scalar(("step", K, P), inp, ref, *_raw_scalar(X, C, w, step=True))
        if K * (P + 1) <= 8192:
            assert step_bytes(K) == 154752
            _check_step(dense.kmeans_step(X, C, w), ref, K, P)
    inp = kc.exact_inputs(Ka, P, N, "none", seed=3)
    ref = kc.reference(inp.X, inp.C, None)
    X, C, _ = _dev(inp)
    _check_scalar(("assign", Ka, P), inp, ref, *_raw_scalar(X, C, None, step=False))
    a, d = dense.kmeans_assign(X, C)
    assert np.array_equal(a.cpu().numpy(), ref.assign) and np.array_equal(_f64(d), ref.mind)


# ---------------------------------------------------------------- D: k_kmeans_update, kmeans_lloyd_step
def _torch_update(sums, cnt, C):
    """The update of models/kmeans.py::KMeans._step, on the CPU."""
    newC = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1e-300)[:, None], C.double()).float()
    flags = torch.stack([(cnt == 0).sum().double(), (newC - C).abs().max().double()])
    return newC, flags


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("K,P", [(1, 4), (10, 20), (64, 64)])
def test_update_kernel_bit_equal(K, P, wide):
    from llama_github_io_amd.ops import _native as nat
    ldt = kc.mfma_shape(K, P)[2] * 16 if wide else P + 1
    g = torch.Generator().manual_seed(K * 100 + P + wide)
    tot = torch.full((K, ldt), float("nan"), dtype=torch.float64)             # columns past P + 1 are never read
    tot[:, :P] = torch.randn(K, P, generator=g, dtype=torch.float64) * 50
    tot[:, P] = torch.rand(K, generator=g, dtype=torch.float64) * 40 + 0.01
    C = torch.randn(K, P, generator=g)
    if K > 1:
        tot[K // 2, P] = 0.0                   # empty: keeps its center
        tot[K - 1, P] = 1e-310                 # subnormal count: divided by the clamp 1e-300
        tot[K - 1, :P] *= 1e-280               # ... sums small enough that the quotient is an ordinary float
        tot[K - 1, 0] = 0.0
    if K == 64:
        tot[3, P] = 1e-310                     # ... and one whose quotient overflows fp32: +-inf, shift inf
    refC, refF = _torch_update(tot[:, :P].contiguous(), tot[:, P].contiguous(), C)
    td, Cd = tot.to(dev), C.to(dev)
    newC = torch.full((K, P), float("nan"), dtype=torch.float32, device=dev)
    cnt = torch.full((K,), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    nat.call("h2o_kmeans_update", td.data_ptr(), ldt, K, P, Cd.data_ptr(), newC.data_ptr(), cnt.data_ptr(),
             flags.data_ptr(), nat.stream_ptr(dev))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(newC), _bits(refC))
    assert np.array_equal(_bits(cnt), _bits(tot[:, P].contiguous()))
    assert np.array_equal(_bits(flags), _bits(refF)), (flags, refF)
    assert float(refF[0]) == (1 if K > 1 else 0) and (K != 64 or np.isinf(float(refF[1])))


@pytest.mark.parametrize("name", ["K10P20-N805-g1-zero", "K32P28-N641-g2-zero", "K64P64-N805-g3-zero",
                                  "K17P4-N805-g2", "K16P16-N1541-g3"])
def test_lloyd_step_bit_equal(name, monkeypatch):
    from llama_github_io_amd.models.kmeans import KMeansTrainer
    from llama_github_io_amd.ops.dense import kmeans_lloyd_step, kmeans_step
    monkeypatch.setenv("H2O_KMEANS_MFMA", "1")
    c = kc.case(name)
    inp, ref = kc.make_inputs(c), kc.case_reference(c)
    X, C, w = _dev(inp)
    refC, refF = _torch_update(torch.from_numpy(ref.sums), torch.from_numpy(ref.cnt), torch.from_numpy(inp.C))
    n_empty = int((ref.cnt == 0).sum())
    assert float(refF[0]) == n_empty and n_empty >= (1 if c.K > 1 else 0) + int(c.zero)

    def same(out):
        d, newC, cnt, flags = out
        assert d.dtype == torch.float32 and np.array_equal(_f64(d), ref.mind)
        assert newC.dtype == torch.float32 and np.array_equal(_bits(newC), _bits(refC))
        assert cnt.dtype == torch.float64 and np.array_equal(cnt.cpu().numpy(), ref.cnt)
        assert flags.dtype == torch.float64 and np.array_equal(_bits(flags), _bits(refF))

    same(kmeans_lloyd_step(X, C, w))
    # kmeans_step plus the torch update of KMeans._step, on the device
    a, d, sums, cnt = kmeans_step(X, C, w, need_assign=False)
    newC = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1e-300)[:, None], C.double()).float()
    same((d, newC, cnt, torch.stack([(cnt == 0).sum().double(), (newC - C).abs().max().double()])))
    # the model's own step: the fused path, and its torch path behind the scalar kernel
    tr = KMeansTrainer({})
    a, *rest = tr._step(X, None if w is None else w.double(), C)
    assert a is None
    same(rest)
    monkeypatch.setenv("H2O_KMEANS_MFMA", "0")
    a, *rest = tr._step(X, None if w is None else w.double(), C)
    same(rest)


# ---------------------------------------------------------------- E: rounding
def _ratios(tag, X, C, w, a, d, sums, cnt, dist_bound):
    """KMRATIO lines and the worst ratio of: distance, assignment, sums, counts (sums / counts where given)."""
    N, K = X.shape[0], C.shape[0]
    D = kc.distances(X, C)
    B = dist_bound(D)
    rows = np.arange(N)
    dref, aref = D.min(1), D.argmin(1)
    out = {"dist": kc.worst_ratio(np.abs(d.astype(np.float64) - D[rows, a]), B[rows, a]),
           "assign": kc.worst_ratio(D[rows, a] - dref, B[rows, a] + B[rows, aref])}
    if sums is not None:
        rs, rc = kc.segment_sums(X, w, a, K)
        bs, bc = kc.sum_bounds(X, w, a, K)
        out["sums"] = kc.worst_ratio(np.abs(sums - rs), bs)
        out["cnt"] = kc.worst_ratio(np.abs(cnt - rc), bc)
    for k, v in out.items():
        print(f"KMRATIO {tag} {k} {v:.3f}")
    assert (a >= 0).all() and (a < K).all()
    return out


@pytest.mark.parametrize("K,P", kc.ROUND_SHAPES)
def test_rounding_mfma(K, P):
    Xn, Cn, wn = kc.round_inputs(K, P)
    N = Xn.shape[0]
    KT, PS, PT = kc.mfma_shape(K, P)
    out = kc.raw_lloyd(torch.from_numpy(Xn).to(dev), torch.from_numpy(Cn).to(dev), torch.from_numpy(wn).to(dev), 1)
    assert (out.assign[N:] == kc.ASSIGN_SENTINEL).all() and (out.mind[N:] == np.float32(kc.MIND_SENTINEL)).all()
    s = out.slabs
    assert not np.isnan(s).any() and (s[:, K:, :] == 0).all() and (s[:, :, P + 1:] == 0).all()
    tot = s.astype(np.float64).sum(0)
    Bfull = kc.mfma_dist_bound(Xn, Cn)
    r = _ratios(f"mfma-K{K}P{P}", Xn, Cn, wn, out.assign[:N].astype(np.int64), out.mind[:N], tot[:K, :P], tot[:K, P],
                lambda D: Bfull)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("K,P", kc.ROUND_SHAPES)
def test_rounding_scalar(K, P, monkeypatch):
    from llama_github_io_amd.ops.dense import kmeans_assign, kmeans_step
    monkeypatch.setenv("H2O_KMEANS_MFMA", "0")
    Xn, Cn, wn = kc.round_inputs(K, P)
    X, C, w = torch.from_numpy(Xn).to(dev), torch.from_numpy(Cn).to(dev), torch.from_numpy(wn).to(dev)
    bound = lambda D: (P + 3) * kc.U24 * D                      # noqa: E731
    a, d, sums, cnt = kmeans_step(X, C, w)
    # sums and counts against the same (n_c + 4) u bounds as the MFMA kernel's: a block adds a center's rows one by
    # one (the first add into 0 and the 0 added for another center's rows are exact), the blocks are summed in fp64
    r = _ratios(f"step-K{K}P{P}", Xn, Cn, wn, a.cpu().numpy(), d.cpu().numpy(), sums.cpu().numpy(),
                cnt.cpu().numpy(), bound)
    assert max(r.values()) <= 1.0, r
    a, d = kmeans_assign(X, C)
    r = _ratios(f"assign-K{K}P{P}", Xn, Cn, wn, a.cpu().numpy(), d.cpu().numpy(), None, None, bound)
    assert max(r.values()) <= 1.0, r

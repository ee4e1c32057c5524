"""CPU anchors of the K-Means Lloyd kernel tests (kmeans_cases.py): conditions on the INPUTS and on the helpers that
test_kmeans_lloyd_gpu.py holds the kernels to. Nothing here runs a kernel.

* The Python twin of the dispatch table equals the ``L(KT, PS, PT)`` lines of csrc/kmeans_mfma.hip, and the case
  table reaches all 24 classes and both ``km_stride`` branches of each kernel variant.
* Every exact case: integer values within the stated ranges, 24 N < 2^24, an fp32 emulation of the kernel's expanded
  distance form equal to the fp64 reference (so an inequality on the device is the kernel's), at least one row tied
  through every route the case is meant to exercise, no row on the higher-index copy of a duplicated center, and the
  intended empty and zero-weight clusters.
* ``check_exact`` accepts the reference itself and reports a row moved to the tied copy, a dropped row, a padding
  leak, an unwritten element and a write past N.
* The rounding cases: the bound of every sum entry is below half the smallest |w x_d| of a row in it, so a dropped
  or doubled row is a failure there too.
* ``kmeans_assign`` / ``kmeans_step`` on CPU tensors (the GEMM branch and the sort-based segment sums) are exact on
  these inputs.
"""
import os
import re

import numpy as np
import pytest
import torch

import kmeans_cases as kc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama_github_io_amd", "csrc")
NAMES = [c.name for c in kc.CASES]


def test_python_table_matches_source():
    src = open(os.path.join(CSRC, "kmeans_mfma.hip")).read()
    body = src[src.index("int h2o_kmeans_mfma(const float* X"):]
    lines = [tuple(int(v) for v in m) for m in re.findall(r"\bL\((\d+), (\d+), (\d+)\);", body)]
    assert len(lines) == 24 and set(lines) == set(kc.CLASSES) and len(set(kc.CLASSES)) == 24
    # every supported (K, P) lands on one of the lines, and its float4 groups / dim tiles hold the shape
    for K in range(1, 65):
        for P in range(4, 65, 4):
            KT, PS, PT = kc.mfma_shape(K, P)
            assert (KT, PS, PT) in kc.CLASSES and K <= 16 * KT and P <= 4 * PS and P + 1 <= 16 * PT
            for o4 in (False, True):
                st = kc.km_stride(P, o4)
                assert st >= P + 1 and 4 * kc.KM_ROWS * st >= KT * 16 * PT * 16      # the block slab fits the slices
    assert kc.mfma_shape(65, 4) is None and kc.mfma_shape(4, 65) is None and kc.mfma_shape(0, 4) is None
    assert kc.km_stride(20) == 49 and kc.km_stride(20, True) == 21 and kc.km_stride(16, True) == 17
    assert kc.km_stride(48) == 49 and kc.km_stride(52) == 53 and kc.km_stride(36, True) == 37


def test_case_table_covers_every_class_and_stride_branch():
    assert {kc.mfma_shape(c.K, c.P) for c in kc.CASES} == set(kc.CLASSES)
    # multi-tile waves (N > 256 grid) in one class per KT at least, one of them the 4-waves-per-SIMD variant
    multi = [c for c in kc.CASES if c.N > 256 * c.grid]
    assert {kc.mfma_shape(c.K, c.P)[0] for c in multi} == {1, 2, 4}
    assert {kc.variant(c.K, c.P) for c in multi} == {("occ4", "pad"), ("occ4", "plain"), ("occ3", "pad"),
                                                      ("occ3", "plain")}
    for K, P in kc.MULTI_SHAPES + kc.OCC4_OFF_SHAPES:
        assert {(c.N, c.grid) for c in kc.CASES if (c.K, c.P) == (K, P) and not c.zero} >= set(kc.MULTI)
    # H2O_KM_OCC4=0: shapes whose default is the occ4 variant, run on k_lloyd_mfma<1, PS <= 6, PT <= 2>
    off = kc.occ4_off_cases()
    assert {(c.K, c.P) for c in off} == set(kc.OCC4_OFF_SHAPES) and len(off) == 3 * len(kc.MULTI)
    assert all(kc.variant(c.K, c.P) [0] == "occ4" and kc.variant(c.K, c.P, False)[0] == "occ3" for c in off)
    assert {kc.mfma_shape(c.K, c.P) for c in off} == {(1, 6, 2), (1, 4, 1)}
    # the named edges
    for K, P in kc.EDGE_SHAPES:
        assert {c.N for c in kc.CASES if (c.K, c.P, c.grid) == (K, P, 1)} >= set(kc.EDGE_N)
        assert any((c.K, c.P, c.N, c.grid) == (K, P, 100, 4) for c in kc.CASES)
    assert sum(c.zero for c in kc.CASES) >= 3 and {kc.mfma_shape(c.K, c.P)[0] for c in kc.CASES if c.zero} == {1, 2, 4}
    assert len(set(NAMES)) == len(NAMES)


def test_routes():
    assert kc.route(0, 1) == {"lane"} and kc.route(0, 5) == {"xor16"} and kc.route(0, 12) == {"xor32"}
    assert kc.route(0, 16) == {"tile"} and kc.route(2, 35) == {"tile"} and kc.route(34, 50) == {"tile"}
    assert kc.route(2, 20) == {"tile", "xor16"} and kc.route(0, 8) == {"xor32"} and kc.route(4, 12) == {"xor32"}
    assert kc.intended_routes(kc.Case("x", 64, 64, 805)) == {"lane", "xor16", "xor32", "tile"}
    assert kc.intended_routes(kc.Case("x", 3, 4, 805, natural=True)) == {"lane", "natural"}
    assert kc.intended_routes(kc.Case("x", 1, 4, 805)) == set()


@pytest.mark.parametrize("name", NAMES)
def test_exact_case_inputs(name):
    c = kc.case(name)
    inp, ref = kc.make_inputs(c), kc.case_reference(c)
    assert inp.X.shape == (c.N, c.P) and inp.C.shape == (c.K, c.P) and c.P % 4 == 0
    for a in (inp.X, inp.C):
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
    far = np.zeros(c.K, bool)
    if c.zero:
        far[inp.zc] = True
    assert np.abs(inp.C[~far]).max(initial=0) <= c.lim and np.abs(inp.C).max() <= 8
    on_far = np.zeros(c.N, bool)
    on_far[list(inp.zrows)] = True
    assert np.abs(inp.X[~on_far]).max(initial=0) <= c.lim and np.abs(inp.X).max() <= 8
    if c.wt == "none":
        assert inp.w is None
    else:
        assert inp.w.dtype == np.float32 and set(np.unique(inp.w)) <= {0.0, 1.0, 2.0, 3.0}
    assert 24 * c.N < 2 ** 24 and ref.mind.max() < 2 ** 24
    # the kernel's expanded form in fp32 gives the fp64 numbers: an inequality on the device is the kernel's
    ea, ed = kc.emulate_expanded(inp.X, inp.C)
    assert np.array_equal(ea, ref.assign) and np.array_equal(ed.astype(np.float64), ref.mind)
    # duplicated centers: the higher index gets no row, so it is an empty cluster
    for cp, src in kc.COPIES:
        if cp < c.K:
            assert np.array_equal(inp.C[cp], inp.C[src]) and not (ref.assign == cp).any() and ref.cnt[cp] == 0
    if c.ties:
        got = kc.tie_routes(c)
        assert kc.intended_routes(c) <= got, (kc.intended_routes(c), got)
        assert c.K < 2 or (ref.cnt == 0).any()
    if c.zero:
        rows = np.nonzero(ref.assign == inp.zc)[0]
        assert set(rows) == set(inp.zrows) and len(rows) == 3 and (inp.w[rows] == 0).all()
        assert ref.cnt[inp.zc] == 0 and (ref.sums[inp.zc] == 0).all() and (ref.mind[rows] == 0).all()


def _fake_raw(c, inp, ref):
    """What a correct kernel returns, built from the reference."""
    KT, PS, PT = kc.mfma_shape(c.K, c.P)
    a = np.full(c.N + kc.PAD, kc.ASSIGN_SENTINEL, np.int32)
    a[:c.N] = ref.assign
    d = np.full(c.N + kc.PAD, kc.MIND_SENTINEL, np.float32)
    d[:c.N] = ref.mind
    s = np.zeros((c.grid, KT * 16, PT * 16), np.float32)
    blk = kc.block_of_rows(c.N, c.grid)
    for b in range(c.grid):
        rows = np.nonzero(blk == b)[0]
        sb, cb = kc.segment_sums(inp.X[rows], None if inp.w is None else inp.w[rows], ref.assign[rows], c.K)
        s[b, :c.K, :c.P], s[b, :c.K, c.P] = sb, cb
    return kc.Raw(a, d, s)


@pytest.mark.parametrize("name", ["K64P64-N805-g3", "K10P20-N805-g1", "K17P4-N805-g2", "K10P20-N100-g4"])
def test_check_exact_notices(name):
    c = kc.case(name)
    inp, ref = kc.make_inputs(c), kc.case_reference(c)
    assert kc.check_exact(c, inp, ref, _fake_raw(c, inp, ref)) == []
    w = np.ones(c.N) if inp.w is None else inp.w
    r = int(np.nonzero((ref.assign == 0) & (w > 0))[0][-1])        # a row of center 0, whose copy is center 1
    o = _fake_raw(c, inp, ref)
    o.assign[r] = 1
    assert any("assign differs in 1 rows" in s for s in kc.check_exact(c, inp, ref, o))
    o = _fake_raw(c, inp, ref)                                       # the row's sums land on the copy
    b = kc.block_of_rows(c.N, c.grid)[r]
    o.slabs[b, 1, :c.P] += w[r] * inp.X[r]
    o.slabs[b, 0, :c.P] -= w[r] * inp.X[r]
    o.slabs[b, 1, c.P] += w[r]
    o.slabs[b, 0, c.P] -= w[r]
    bad = kc.check_exact(c, inp, ref, o)
    assert any("sums differ" in s for s in bad) and any("counts differ" in s for s in bad)
    o = _fake_raw(c, inp, ref)
    o.mind[r] = np.nextafter(o.mind[r], np.float32(np.inf))
    assert any("mind differs in 1 rows" in s for s in kc.check_exact(c, inp, ref, o))
    KT, PS, PT = kc.mfma_shape(c.K, c.P)
    for idx, word in (((0, KT * 16 - 1, 0), "padding center"), ((0, 0, PT * 16 - 1), "padding dim")):
        if (word == "padding center" and KT * 16 > c.K) or (word == "padding dim" and PT * 16 > c.P + 1):
            o = _fake_raw(c, inp, ref)
            o.slabs[idx] = 1.0
            assert any(word in s for s in kc.check_exact(c, inp, ref, o)), word
    o = _fake_raw(c, inp, ref)
    o.slabs[c.grid - 1, 0, 0] = np.nan
    assert any("never written" in s for s in kc.check_exact(c, inp, ref, o))
    o = _fake_raw(c, inp, ref)
    o.assign[c.N] = 0
    o.mind[c.N + kc.PAD - 1] = 0.0
    bad = kc.check_exact(c, inp, ref, o)
    assert any("assign written past N" in s for s in bad) and any("mind written past N" in s for s in bad)
    if c.N <= 256 * (c.grid - 1):                                    # a block without rows
        o = _fake_raw(c, inp, ref)
        o.slabs[c.grid - 1, 0, c.P] = 1.0
        assert any("no rows" in s for s in kc.check_exact(c, inp, ref, o))


@pytest.mark.parametrize("K,P", kc.ROUND_SHAPES)
def test_rounding_bounds_notice_a_row(K, P):
    X, C, w = kc.round_inputs(K, P)
    assert X.dtype == C.dtype == w.dtype == np.float32 and X.shape == (kc.N_TAIL37, P)
    assert w.min() >= 0.25 and not np.array_equal(w, np.rint(w))
    D = kc.distances(X, C)
    a = D.argmin(1)
    bs, bc = kc.sum_bounds(X, w, a, K)
    wx = np.abs(X.astype(np.float64) * w.astype(np.float64)[:, None])
    for k in range(K):
        rows = a == k
        if rows.any():
            assert (bs[k] < 0.5 * wx[rows].min(0)).all() and bc[k] < 0.5 * w[rows].min()
        else:
            assert (bs[k] == 0).all() and bc[k] == 0
    # the distance bound is far below the distances' spread over the centers, and it is a bound of the emulation
    B = kc.mfma_dist_bound(X, C)
    ea, ed = kc.emulate_expanded(X, C)
    assert kc.worst_ratio(np.abs(ed.astype(np.float64) - D[np.arange(len(ea)), ea]), B[np.arange(len(ea)), ea]) <= 1
    assert kc.worst_ratio(np.array([1.0, 0.0]), np.array([0.0, 0.0])) == np.inf
    assert kc.worst_ratio(np.array([0.0, 1.0]), np.array([0.0, 4.0])) == 0.25


@pytest.mark.parametrize("K,P,N", [(64, 64, 805), (17, 4, 805), (200, 50, 700), (100, 13, 257)])
def test_cpu_tensor_paths_are_exact(K, P, N):
    """kmeans_assign's GEMM branch (||x||^2 - 2 x.c + ||c||^2 in fp64) and kmeans_step's sort-based segment sums."""
    from llama_github_io_amd.ops.dense import kmeans_assign, kmeans_step
    inp = kc.exact_inputs(K, P, N, "int", seed=K + P)
    ref = kc.reference(inp.X, inp.C, inp.w)
    X, C, w = torch.from_numpy(inp.X), torch.from_numpy(inp.C), torch.from_numpy(inp.w)
    a, d = kmeans_assign(X, C)
    assert np.array_equal(a.numpy(), ref.assign) and d.dtype == torch.float32
    assert np.array_equal(d.numpy().astype(np.float64), ref.mind)
    a, d, sums, cnt = kmeans_step(X, C, w)
    assert np.array_equal(a.numpy(), ref.assign) and np.array_equal(d.numpy().astype(np.float64), ref.mind)
    assert np.array_equal(sums.numpy(), ref.sums) and np.array_equal(cnt.numpy(), ref.cnt)
    a, d, sums, cnt = kmeans_step(X, C, None)
    s1, c1 = kc.segment_sums(inp.X, None, ref.assign, K)
    assert np.array_equal(sums.numpy(), s1) and np.array_equal(cnt.numpy(), c1)

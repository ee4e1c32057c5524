"""CPU anchors of the level-histogram tests (hist_cases.py): the helpers that test_hist_levels_gpu.py holds the
kernels to are themselves checked against RefTreeBuilder, and the case table is checked to give bounds that mean
something.

* ``node_rows`` reproduces the reference builder's own row sets (leaf_of_row, the wl / wr of every decision).
* ``ref_node_hist`` equals ``RefTreeBuilder._hist``.
* Non-vacuity (a condition on the INPUTS of the case table, not on any kernel): in every occupied (node, bin, feature)
  entry of every level the GPU test checks, the wY bound is below half the smallest non-zero |wY| of a row in the
  entry, so dropping, duplicating or mis-binning any single row of the entry is a failure. Every case but the two
  named quantisation stress cases (all-negative windows, dynamic range).

  FPACK (packed=2) cannot meet this in every entry, whatever the inputs: its conversion error is up to
  PACK_MAX M / (2 0.99 2^31) = 1.49e-5 M per row, so an entry of n rows has a bound of at least n 1.49e-5 M, and the
  constant column's entry holds every row of the node (20,000 resp. 200,000 at the root, the sizes the modes and the
  flush windows need): 0.28 resp. 1.5 against half of 0.05 resp. 0.5. There the test asserts what FPACK's precision
  does allow: the condition holds in every entry of the columns of >= 200 bins, so every row has entries that catch
  its loss, duplication or move.
* The same as a test: a deliberately wrong reference (``ref_node_hist(shift=...)``: one row counted in the
  neighbouring bin) is reported as a failure on the count or the wY plane by the very comparison the GPU test uses.
"""
import numpy as np
import pytest

from llama_github_io_amd.ops import tree as T

import hist_cases as hc


def _ref_tree(c, depth=None):
    inp = hc.make_inputs(c)
    ref = hc.ref_builder(c, inp, max(c.depths) if depth is None else depth)
    ref.build(inp.aux, None, 0, seed=5, leaf_fn=hc.leaf_fn)
    return inp, ref, ref.pop_levels()[0]


@pytest.mark.parametrize("name", ["mode-unpacked-na", "mode-fpack-nona", "ragged-minw1-count",
                                  "layout-planar3-unpacked", "small-7", "small-1"])
def test_node_rows_match_reference_builder(name):
    c = hc.case(name)
    inp, ref, tl = _ref_tree(c)
    levels, leaf = hc.node_rows(tl, inp.bins)
    assert np.array_equal(leaf, ref.leaf_of_row.numpy())
    assert (leaf >= 0).all() and leaf.max() + 1 == tl.n_leaves
    a = inp.aux.numpy().astype(np.float64)
    b = inp.bins.numpy()
    for d, rows_d in enumerate(levels):
        assert len(rows_d) == len(tl.decs[d])
        assert d > 0 or np.array_equal(rows_d[0], np.arange(c.N))
        for i, rows in enumerate(rows_d):
            dd = tl.decs[d][i]
            if dd["feat"] < 0:
                continue
            gl = T.dec_go_left_np(dd, b[rows, int(dd["feat"])].astype(np.int64))
            np.testing.assert_allclose(a[rows[gl], 0].sum(), dd["wl"], rtol=1e-12)
            np.testing.assert_allclose(a[rows[~gl], 0].sum(), dd["wr"], rtol=1e-12)
    # the plan (which child is histogrammed) is consistent: one built child per parent, siblings point at each other
    plan = hc.plan_nodes(tl)
    assert len(plan) == len(levels)
    for d in range(1, len(plan)):
        assert len(plan[d]) == len(levels[d])
        for i, pl in enumerate(plan[d]):
            if pl["sib"] >= 0:
                s = plan[d][pl["sib"]]
                assert s["sib"] == i and s["parent"] == pl["parent"] and s["build"] + pl["build"] == 1
            else:
                assert pl["build"] == 1


@pytest.mark.parametrize("name", ["mode-unpacked-na", "mode-count-na", "layout-planar3-unpacked", "root16-count"])
def test_ref_node_hist_matches_reference_builder(name):
    c = hc.case(name)
    inp, ref, tl = _ref_tree(c, depth=3 if c.kind != "root16" else 1)
    levels, _ = hc.node_rows(tl, inp.bins)
    a = inp.aux.numpy()
    for rows_d in levels:
        for rows in rows_d:
            h, nayy, wyy = hc.ref_node_hist(rows, inp.bins, inp.aux, inp.F)
            h0, nayy0, wyy0 = ref._hist(rows, a)
            # the same bincounts in the same row order: bit for bit
            assert np.array_equal(h, h0.transpose(1, 0, 2))
            np.testing.assert_allclose(nayy, nayy0, rtol=1e-12, atol=0)
            np.testing.assert_allclose(wyy, wyy0, rtol=1e-12, atol=0)
            n, sw, sy, nak, kpos = hc.ref_node_abs(rows, inp.bins, inp.aux, inp.F)
            assert np.array_equal(n.sum(0), np.full(inp.F, rows.size))
            assert (np.abs(h[:, :, 1]) <= sy * (1 + 1e-12)).all() and (np.abs(h[:, :, 0]) <= sw * (1 + 1e-12)).all()


def test_case_table_reaches_what_it_names():
    names = hc.CASE_IDS
    assert len(set(names)) == len(names)
    assert sorted(c.name for c in hc.CASES if c.stress) == sorted(
        ["win-count-g1-minus", "win-count-g3-minus", "win-fpack-g1-minus", "win-fpack-g3-minus", "range-unpacked",
         "range-unit"])
    # flush windows per block at 200,000 rows: four with one block, two with three
    assert hc.windows_per_block(200000, 1, True) == 4 and hc.windows_per_block(200000, 3, True) == 2
    assert hc.windows_per_block(200000, 4, True) == 1 and hc.windows_per_block(200000, 256, True) == 1
    for c in hc.CASES:
        if c.kind != "synthetic":
            continue
        inp = hc.make_inputs(c)
        b = inp.bins.numpy()
        assert b.shape == (c.N, c.stride) and (b[:, c.F:] == 0).all()
        assert bool((b[:, :c.F] == T.NA_BIN).any()) == (c.na and c.N >= 2)
        for f in range(c.F):
            col = b[:, f]
            assert col[col != T.NA_BIN].max(initial=0) < inp.nbins_f[f]
        assert (b[:, 6] == 0).all()
        a = inp.aux.numpy()
        if c.mode in ("count", "unit"):
            assert set(np.unique(a[:, 0])) <= {0.0, 1.0}
        if c.mode == "fpack":
            assert a[:, 0].min() > 0 and a[:, 0].max() <= 0.25


def _checked_nodes(c):
    """(level, node, rows, tol dict) of every node of every level that the GPU test of ``c`` compares."""
    inp, ref, tl = _ref_tree(c)
    levels, _ = hc.node_rows(tl, inp.bins)
    tr = hc.TreeRef(c, inp)
    tols = tr.level_tols(levels, hc.plan_nodes(tl))
    return inp, tr, [(d, i, rows, tols[d][i]) for d, rows_d in enumerate(levels) for i, rows in enumerate(rows_d)]


@pytest.mark.parametrize("name", [c.name for c in hc.ORDINARY])
def test_bound_is_not_vacuous(name):
    c = hc.case(name)
    inp, tr, nodes = _checked_nodes(c)
    wide = np.nonzero(np.asarray(inp.nbins_f) >= 200)[0]
    worst = 0.0
    assert max(d for d, _, _, _ in nodes) + 1 >= hc.min_levels(c)
    for d, i, rows, tl in nodes:
        m = hc.min_abs_wy(rows, inp.bins, inp.aux, inp.F)
        occ = np.isfinite(m)
        with np.errstate(invalid="ignore"):
            ratio = np.where(occ, tl["wy"] / np.where(occ, 0.5 * m, 1.0), 0.0)
        if c.mode == "fpack":
            assert wide.size >= 3
            ratio = ratio[:, wide]
        worst = max(worst, float(ratio.max()))
        t, f = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        assert ratio.max() < 1.0, (f"level {d} node {i} ({rows.size} rows) feature {f} bin {t}: wY bound "
                                   f"{tl['wy'][t, f if c.mode != 'fpack' else wide[f]]!r} is not below half the "
                                   f"smallest |wY| of the entry")
    print(f"{name}: worst tol / (min |wY| / 2) = {worst:.3g} over {len(nodes)} nodes")


@pytest.mark.parametrize("name", [c.name for c in hc.ORDINARY])
def test_wrong_reference_is_caught(name):
    """One row shifted to the neighbouring bin in the reference must fail the count or the wY plane."""
    c = hc.case(name)
    inp, tr, nodes = _checked_nodes(c)
    a = inp.aux.numpy()
    rng = np.random.default_rng(3)
    no_na = not bool((inp.bins.numpy()[:, :inp.F] == T.NA_BIN).any())
    feats = np.nonzero(np.asarray(inp.nbins_f) >= 200)[0] if c.mode == "fpack" else np.arange(inp.F)
    last = max(d for d, _, _, _ in nodes)
    small = min((n for n in nodes if n[0] == last), key=lambda n: n[2].size)
    picks = [(nodes[0], 2, feats[rng.choice(feats.size, min(3, feats.size), replace=False)])]
    if small is not nodes[0]:
        picks.append((small, 2, feats))
    tried = 0
    for (d, i, rows, tl), nrows, fs in picks:
        live = rows[a[rows, 1] != 0]
        assert live.size > 0
        ref = tr.node(rows)
        got = (ref["h"], ref["nayy"], ref["wyy"])
        ratios, bad = hc.compare_node(got, ref, tl, inp.nbins_f, no_na)
        assert not bad and max(ratios.values()) == 0.0          # the right reference passes
        for r in rng.choice(live, min(nrows, live.size), replace=False):
            for f in fs:
                h, nayy, wyy = hc.ref_node_hist(rows, inp.bins, inp.aux, inp.F, shift=(int(r), int(f)))
                ratios, bad = hc.compare_node(got, dict(h=h, nayy=nayy, wyy=wyy), tl, inp.nbins_f, no_na)
                assert ratios["w"] > 1.0 or ratios["wy"] > 1.0, (d, i, int(r), int(f), ratios)
                assert any(s.startswith("plane") for s in bad)
                tried += 1
    assert tried >= 3

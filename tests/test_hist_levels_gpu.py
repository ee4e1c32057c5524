"""The tree engine's intermediate results against fp64 references (csrc/tree_kernels.hip; helpers, inputs, the case
table and the bound in hist_cases.py, which test_hist_levels_paths.py anchors on the CPU).

Every case builds its tree with max_depth 1 .. 5 on a fresh GpuTreeBuilder and, from the state each build leaves on the
device, checks

* the node histograms of the two levels that survive in the ping-pong buffers (``gb.hist``): every entry of every
  active node, built (k_hist_build / k_hist_root16 -> k_hist_reduce) or derived (parent - sibling), within ``tol``;
  counts of the packed count modes exactly; bins at or past a column's bin count, and the NA bin when no row is NA,
  exactly 0; nayy / wyy within their (loose) fp32 bound;
* the node list against the plan derived from the decoded tree (parent, build, sib, dir) and, on even levels,
  ``Node.len`` against the size of the row set;
* ``nl``: for every even-level parent with a continuing child, the rows its decision sends left (counted by the
  ftile-0 blocks of the filtered odd-level pass, once per parent row); 0 for the other parents;
* the routed payload (k_route): rows [start, start + len) of a level-2 / level-4 node in its ping-pong buffer are, as
  a multiset, the node's rows of the master bins (every byte of the stride, every plane) with their wY (and w);
* ``leaf_of_row`` and the leaf sums (k_leaf_assign / k_leafsum_finish) within n M 2^-lb + 2 2^-24 S;
* ``qs``: bit for bit the scales of k_qscale's formulas (capped at 2^127 in the two scale-overflow cases only).

Which k_hist_build instantiation a case reaches (launch_hist): FILT = every odd level of any case with depth >= 2,
!FILT = the even levels; PACKED / UNIT = the case's mode; NONA = the cases without NA rows, with 4 bin replicas on
columns 1, 2, 5, 6 (3, 60, 7, 1 bins), 2 on column 3 (100 bins), 1 elsewhere (``mode-*-nona``), !NONA = ``mode-*-na``;
the ``acc`` branch of flush_partial = ``win-*`` and ``pf32-count`` (2 and 4 windows per block). BUF is on for every
power-of-two row size here and off for strides 12 and 48 (``layout-s12-*``, ``layout-s48-*``); the > 2^31-byte side of
BUF stays with the large-buffer test of test_tree_engine.py.

Worst err / tol on an MI355X, per mode and plane, over every case (a ratio above 1 is a failure; the test prints
the figures of each case as ``HISTRATIO <case> <mode> <plane> <ratio>``):

    mode       w      wY     nayy   wyy    leaf num  leaf den
    unpacked   0.825  0.998  0.187  0.015  0.340     0.468
    count      0      0.673  0.298  0.001  0.108     0.441
    unit       0      0.999  0.164  0.001  0.203     0.525
    fpack      0.996  0.999  0.097  0.001  0.125     0.463

The ratios next to 1 are entries of one or two rows, where the bound is the conversion error of a single row (one
truncation, in FPACK one rounding) and the kernel comes as close to it as a single row can: the dynamic-range cases
(0.998 / 0.999) and FPACK's sparse bins. With the library of the commit before the scale cap the two scale-overflow
cases fail as k_qscale's code predicts (inf scales: |wY| entries of 1.9e-30 against 1.1e-31, leaf sums of the wrong
sign), while an ordinary case run against that library (``mode-unit-nona``) passes with the same ``qs``, bit for bit.
Each case takes 0.01 - 1 s (five builds and their references; the 200,000-row cases about 0.9 s).
"""
import time

import numpy as np
import pytest
import torch

from llama_github_io_amd.ops import tree as T

import hist_cases as hc

gpu = pytest.mark.gpu


def _note(c, plane, ratio, case_worst):
    case_worst[plane] = max(case_worst.get(plane, 0.0), ratio)


def _expected_qs(c, inp):
    """k_qscale's scales from the planes' maxima, in the kernel's own fp64 expressions."""
    a = inp.aux.numpy()
    m = [float(np.abs(a[:, k]).max()) for k in range(4)]
    cap = hc.QS_CAP
    fp = c.mode == "fpack"
    qs = np.zeros(13)
    for k in range(2):
        sc = min(1099511627776.0 / m[k], cap) if m[k] > 0 else 1.0
        qs[k], qs[2 + k] = sc, 1.0 / sc
    sp = 1.0 if not m[1] > 0 else min((0.99 * 2147483648.0) / (float(hc.PACK_MAX) * m[1]) if fp else 1073741824.0 / m[1],
                                      cap)
    qs[4], qs[5] = sp, 1.0 / sp
    sw = min((0.99 * 4294967296.0) / (float(hc.PACK_MAX) * m[0]), cap) if (fp and m[0] > 0) else 1.0
    qs[10], qs[11], qs[12] = sw, 1.0 / sw, 32.0 if fp else 48.0
    lb = max(8, 61 - int(c.N).bit_length())
    for k in (2, 3):
        sc = min(2.0 ** lb / m[k], cap) if m[k] > 0 else 1.0
        qs[6 + k - 2], qs[8 + k - 2] = sc, 1.0 / sc
    return qs


def _void_sorted(mat):
    mat = np.ascontiguousarray(mat)
    v = mat.view(np.dtype((np.void, mat.shape[1] * mat.dtype.itemsize))).ravel().copy()
    v.sort()
    return v


def _check_hist(c, inp, tr, gb, D, levels, plan, tols, problems, case_worst):
    no_na = gb._no_na()
    for d in sorted({D - 1, D - 2}):
        if d < 0 or d >= len(levels):
            continue
        slots = hc.gpu_level_hist(gb, d)
        for i, rows in enumerate(levels[d]):
            got = hc.split_slot(slots[i], inp.F)
            ratios, bad = hc.compare_node(got, tr.node(rows), tols[d][i], inp.nbins_f, no_na)
            for plane, r in ratios.items():
                _note(c, plane, r, case_worst)
            kind = "built" if plan[d][i]["build"] else "derived"
            problems += [f"D={D} level {d} node {i} ({kind}, {rows.size} rows) {s}" for s in bad]


def _check_nodes_and_nl(c, inp, gb, D, tl, levels, plan, problems):
    b = inp.bins.numpy()
    for d in range(len(levels)):
        n = len(levels[d])
        nodes = gb.av[f"nodes{d}"].cpu().numpy().view(T.NODE_DT)[:n]
        for k in ("parent", "build", "sib", "dir"):
            if d > 0 and not np.array_equal(nodes[k], plan[d][k]):
                problems.append(f"D={D} level {d}: Node.{k} {nodes[k].tolist()} != plan {plan[d][k].tolist()}")
        if d % 2 == 0:
            want = np.array([r.size for r in levels[d]])
            if not np.array_equal(nodes["len"], want):
                problems.append(f"D={D} level {d}: Node.len {nodes['len'].tolist()} != row sets {want.tolist()}")
        if d % 2 == 0 and d + 1 < D:
            nl = gb.av[f"nl{d}"].cpu().numpy().view(np.int32)[:n]
            want = np.zeros(n, dtype=np.int64)
            for i, rows in enumerate(levels[d]):
                dd = tl.decs[d][i]
                if dd["feat"] >= 0 and (tl.child_l[d][i] >= 0 or tl.child_r[d][i] >= 0):
                    want[i] = int(T.dec_go_left_np(dd, b[rows, int(dd["feat"])].astype(np.int64)).sum())
            if not np.array_equal(nl, want):
                problems.append(f"D={D} nl{d} {nl.tolist()} != left-going rows {want.tolist()}")


def _check_route(c, inp, gb, D, levels, problems):
    b, a = inp.bins.numpy(), inp.aux.numpy()
    N, stride = b.shape
    for e in range(2, min(D, len(levels)), 2):
        buf = gb.bufs[(e // 2 - 1) % 2]
        raw = buf["bins"].cpu().numpy()
        if gb.planar:
            raw = raw.reshape(stride // 32, N, 32).transpose(1, 0, 2).reshape(N, stride)
        else:
            raw = raw.reshape(N, stride)
        y = buf["y"].cpu().numpy()
        w = None if c.unit else buf["w"].cpu().numpy()
        nodes = gb.av[f"nodes{e}"].cpu().numpy().view(T.NODE_DT)[:len(levels[e])]
        spans = sorted((int(nd["start"]), int(nd["start"] + nd["len"])) for nd in nodes)
        if any(s < 0 or t > N or s > t for s, t in spans) or any(spans[k][1] > spans[k + 1][0]
                                                                   for k in range(len(spans) - 1)):
            problems.append(f"D={D} level {e}: node ranges overlap or leave the buffer: {spans}")
            continue
        for i, rows in enumerate(levels[e]):
            s, n = int(nodes[i]["start"]), int(nodes[i]["len"])
            if n != rows.size:
                continue                                     # reported by the Node.len check
            cols = [raw[s:s + n], y[s:s + n].view(np.uint8).reshape(n, 4)]
            ref = [b[rows], a[rows, 1].copy().view(np.uint8).reshape(n, 4)]
            if w is not None:
                cols.append(w[s:s + n].view(np.uint8).reshape(n, 4))
                ref.append(a[rows, 0].copy().view(np.uint8).reshape(n, 4))
            if not np.array_equal(_void_sorted(np.concatenate(cols, 1)), _void_sorted(np.concatenate(ref, 1))):
                problems.append(f"D={D} level {e} node {i}: routed rows [{s}, {s + n}) are not the node's rows")


def _check_leaves(c, inp, gb, D, tl, leaf, problems, case_worst):
    a = inp.aux.numpy().astype(np.float64)
    got_leaf = gb.leaf_of_row.cpu().numpy()
    if not np.array_equal(got_leaf, leaf):
        problems.append(f"D={D}: leaf_of_row differs from the decoded tree's walk in {int((got_leaf != leaf).sum())} rows")
        return
    L = tl.n_leaves
    ls = gb.leafsum[:L].cpu().numpy()
    n = np.bincount(leaf, minlength=L)
    for k, plane in ((2, "leaf_num"), (3, "leaf_den")):
        want = np.bincount(leaf, weights=a[:, k], minlength=L)
        t = hc.leaf_tol(c.N, n, np.bincount(leaf, weights=np.abs(a[:, k]), minlength=L), float(np.abs(a[:, k]).max()))
        err = np.abs(ls[:, k - 2] - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, np.where(t > 0, err / t, np.inf))
        q = np.where(np.isnan(ls[:, k - 2]), np.inf, q)
        j = int(np.argmax(q))
        _note(c, plane, float(q[j]), case_worst)
        if not q[j] <= 1.0:
            problems.append(f"D={D} {plane} leaf {j} ({n[j]} rows): got {ls[j, k - 2]!r} want {want[j]!r} tol {t[j]!r}")


@gpu
@pytest.mark.parametrize("name", hc.CASE_IDS)
def test_level_histograms_routed_rows_and_leaf_sums(name, monkeypatch):
    t_start = time.perf_counter()
    c = hc.case(name)
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    inp = hc.make_inputs(c)
    dev = torch.device("cuda", 0)
    bins_dev, aux_dev = inp.builder_bins(dev), inp.aux.to(dev)
    tr = hc.TreeRef(c, inp)
    problems, case_worst = [], {}
    deepest = 0
    for D in c.depths:
        gb = T.GpuTreeBuilder(bins_dev, inp.F, inp.nbins_f, inp.iscat_f, None, D, inp.params, grid=c.grid)
        if inp.groups is not None:
            gb.set_feature_groups(*inp.groups)
        assert gb.pf32 == int(c.pf32)
        assert gb.planar == (inp.planar_input or (c.stride >= 64 and c.stride % 32 == 0
                                                  and dict(c.env).get("H2O_BINS_ROWMAJOR") != "1"))
        assert gb._no_na() == (not bool((inp.bins.numpy()[:, :inp.F] == T.NA_BIN).any()))
        gb.build(aux_dev, None, 0, seed=5, leaf_fn=hc.leaf_fn, packed=c.packed, unit=c.unit)
        torch.cuda.synchronize()
        if c.kind == "root16":
            assert bool(gb._plan.fine16)
        tl = gb.pop_levels()[0]
        levels, leaf = hc.node_rows(tl, inp.bins)
        plan = hc.plan_nodes(tl)
        tols = tr.level_tols(levels, plan)
        deepest = max(deepest, len(levels))
        qs = gb.qs.cpu().numpy()[:13]
        want_qs = _expected_qs(c, inp)
        if not np.array_equal(qs, want_qs):
            problems.append(f"D={D} qs {qs.tolist()} != {want_qs.tolist()}")
        _check_hist(c, inp, tr, gb, D, levels, plan, tols, problems, case_worst)
        _check_nodes_and_nl(c, inp, gb, D, tl, levels, plan, problems)
        _check_route(c, inp, gb, D, levels, problems)
        _check_leaves(c, inp, gb, D, tl, leaf, problems, case_worst)
        del gb
    for plane, r in sorted(case_worst.items()):
        print(f"HISTRATIO {name} {c.mode} {plane} {r:.4g}")
    print(f"HISTTIME {name} levels {deepest} seconds {time.perf_counter() - t_start:.2f}")
    # the case reaches what it is for: a tree below the root wherever the response allows a split
    assert deepest >= hc.min_levels(c), f"the tree stopped at {deepest} levels"
    assert not problems, f"{len(problems)} problems, the first:\n" + "\n".join(problems[:12])

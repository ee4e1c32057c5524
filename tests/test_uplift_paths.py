"""Uplift DRF on the host: the full uplift metrics against the NumPy formulas of uplift_cases.py, scoring a frame
(``model_performance``, validation metrics, the REST route), the spellings of ``uplift_metric``, and a 2-rank gloo run
against a single process."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import uplift_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NUM, ROWS, NBINS = 3, 4000, 40
SCALARS = ("AUUC", "qini", "lift", "gain", "auuc_normalized", "aecu", "ate", "att", "atc")
CURVES = ("qini", "lift", "gain")


@pytest.fixture(scope="module")
def trained():
    """(model, training frame, validation frame): 3000 / 1000 rows of one synthetic frame, on the CPU."""
    from llama_github_io_amd.models import builder
    fr = uc.frame(ROWS, N_NUM)
    tr, va = fr[:3000, :], fr[3000:, :]
    m = builder.train("upliftdrf", dict(ntrees=4, max_depth=5, treatment_column="trt", seed=7, auuc_nbins=NBINS,
                                        auuc_type="gain", mtries=2), x=uc.predictors(N_NUM), y="y",
                      training_frame=tr, validation_frame=va)
    return m, tr, va


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "thresholds_and_metric_scores":
            assert [list(r.values()) for r in a[k]] == [list(r.values()) for r in b[k]]
        else:
            assert a[k] == b[k], k


def test_model_performance_of_the_training_frame_is_the_training_metrics(trained):
    m, tr, va = trained
    tm = m.output["training_metrics"]
    assert tm["auuc_nbins"] == NBINS and tm["auuc_type"] == "gain"
    _same(m.model_performance(tr), tm)


def test_validation_metrics_are_those_of_the_validation_frame(trained):
    m, tr, va = trained
    vm = m.output["validation_metrics"]
    assert vm is not None and vm["model_category"] == "BinomialUplift"
    _same(m.model_performance(va), vm)
    assert m.model_performance(valid=True) is vm
    assert vm["AUUC"] != m.output["training_metrics"]["AUUC"]


def _columns(fr, m):
    df = fr.as_data_frame()
    u = m.predict(fr).as_data_frame()["uplift_predict"].to_numpy()
    return u, (df["y"] == "yes").to_numpy().astype(float), (df["trt"] == "treat").to_numpy().astype(float)


def test_every_key_equals_the_numpy_formulas(trained):
    from llama_github_io_amd.models import uplift
    m, tr, va = trained
    tm = m.output["training_metrics"]
    u, y, t = _columns(tr, m)
    ref = uc.uplift_metrics_reference(u, y, t, NBINS, "gain")
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=1e-12, atol=1e-12)
    tab = tm["auuc_table"]
    close(tab["thresholds"], ref["thresholds"])
    close(tab["n"], ref["n"])
    assert ref["n"][-1] == 3000 and len(tab["n"]) == NBINS
    for c in CURVES:
        close(tab[c], ref["curves"][c])
        close(tm[c], ref["auuc"][c])
        close(tm["auuc_normalized_table"][c], ref["auuc_normalized"][c])
        close(tm["auuc_random_table"][c], ref["auuc_random"][c])
        close(tm["aecu_table"][c], ref["aecu"][c])
    close(tab["uplift"], ref["curves"]["gain"])
    close(tab["uplift_normalized"], ref["normalized"]["gain"])
    close(tab["uplift_random"], ref["random"]["gain"])
    close(tm["AUUC"], ref["auuc"]["gain"])
    close(tm["auuc_normalized"], ref["auuc_normalized"]["gain"])
    close(tm["aecu"], ref["aecu"]["gain"])
    for k in ("ate", "att", "atc"):
        close(tm[k], ref[k])
    assert tm["att"] != tm["atc"]
    # a random line ends on its curve, a normalised qini / gain curve at +-1, lift is not rescaled
    rows = tm["thresholds_and_metric_scores"]
    for c in CURVES:
        close(rows[-1][c + "_random"], rows[-1][c])
    assert abs(rows[-1]["gain_normalized"]) == 1.0 and abs(rows[-1]["qini_normalized"]) == 1.0
    assert [r["lift_normalized"] for r in rows] == tab["lift"]
    # the keys of before are those of auuc() on the same scores
    again = uplift.auuc(*(torch.from_numpy(v).to(m.device) for v in (u, y, t)), NBINS, "gain")
    for k in ("qini", "lift", "gain", "AUUC", "auuc_type", "auuc_nbins"):
        assert again[k] == tm[k], k
    for c in CURVES:
        assert again["auuc_table"][c] == tab[c]


def test_accessors_honour_metric(trained):
    m, tr, va = trained
    tm = m.output["training_metrics"]
    rows = tm.thresholds_and_metric_scores()
    assert len(rows) == NBINS
    assert list(rows[0]) == ["threshold"] + [c + s for s in ("", "_normalized", "_random") for c in CURVES] + ["n"]
    assert [r["threshold"] for r in rows] == sorted((r["threshold"] for r in rows), reverse=True)
    for c in CURVES:
        assert tm.auuc(c) == tm[c]
        assert tm.auuc_normalized(c) == tm["auuc_normalized_table"][c]
        assert tm.aecu(c) == tm["aecu_table"][c]
        assert tm.uplift(c) == tm["auuc_table"][c] == [r[c] for r in rows]
        assert tm.uplift_normalized(c) == [r[c + "_normalized"] for r in rows]
        assert tm.uplift_random(c) == [r[c + "_random"] for r in rows]
    assert tm.auuc() == tm["AUUC"] == tm["gain"] and tm.auuc_normalized() == tm["auuc_normalized"]
    assert tm.uplift() == tm.uplift("AUTO") == tm["auuc_table"]["uplift"] == tm["auuc_table"]["gain"]
    assert tm.uplift_normalized() == tm["auuc_table"]["uplift_normalized"]
    assert tm.uplift_random() == tm["auuc_table"]["uplift_random"]
    assert tm.aecu("AUTO") == tm["aecu"] and tm.aecu() == tm["aecu_table"]["qini"]
    assert (tm.ate(), tm.att(), tm.atc()) == (tm["ate"], tm["att"], tm["atc"])
    assert tm.uplift("qini") != tm.uplift("gain")
    with pytest.raises(ValueError):
        tm.uplift("auc")


def test_a_frame_without_the_treatment_column_raises(trained):
    m, tr, va = trained
    with pytest.raises(ValueError, match="trt"):
        m.model_performance(va[:, [f"x{j}" for j in range(N_NUM)] + ["c", "y"]])


def test_rest_model_metrics_carry_the_uplift_fields(trained):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from llama_github_io_amd.api.server import create_app
    from llama_github_io_amd.core import dkv
    m, tr, va = trained
    dkv.put(m.key, m)
    r = TestClient(create_app()).post(f"/3/ModelMetrics/models/{m.key}/frames/{va.frame_id}").json()["model_metrics"][0]
    vm = m.output["validation_metrics"]
    assert r["model_category"] == "BinomialUplift"
    for k in SCALARS:
        assert abs(r[k] - vm[k]) <= 1e-12 * max(1.0, abs(vm[k])), k
    for k in ("auuc_table", "auuc_normalized_table", "auuc_random_table", "aecu_table"):
        assert set(r[k]) == set(vm[k])
    assert r["aecu_table"]["lift"] == vm["aecu_table"]["lift"] and r["auuc_table"]["n"] == vm["auuc_table"]["n"]
    assert r["thresholds_and_metric_scores"]["rowcount"] == NBINS


def _forest(m):
    return [(t.feat.tolist(), t.thr.tolist(), t.left.tolist(), t.right.tolist(), t.value.tolist())
            for f in (m.f_t, m.f_c) for t in f.trees]


def test_chi_squared_in_every_spelling():
    from llama_github_io_amd.models import builder
    fr = uc.frame(ROWS, N_NUM)
    grow = lambda metric: _forest(builder.train(
        "upliftdrf", dict(ntrees=3, max_depth=6, treatment_column="trt", seed=1, uplift_metric=metric),
        x=uc.predictors(N_NUM), y="y", training_frame=fr))
    chi = grow("chi_squared")
    assert chi == grow("ChiSquared") == grow("CHI_SQUARED")
    assert chi != grow("euclidean")             # the data tells the two divergences apart
    assert chi != grow("KL")


# ---- two ranks against one process
def _rank(rank, world, port, csv, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), H2O_AMD_DEVICE="cpu", OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    import h2o
    from llama_github_io_amd.models import builder
    import llama_github_io_amd.parallel.collectives as coll
    h2o.init(verbose=False)
    fr = h2o.import_file(csv)
    m = builder.train("upliftdrf", dict(ntrees=3, max_depth=4, treatment_column="trt", seed=3, auuc_nbins=30,
                                        auuc_type="lift"), x=uc.predictors(N_NUM), y="y", training_frame=fr)
    tm = m.output["training_metrics"]
    res = dict(cloud_size=h2o.cluster().cloud_size, scalars={k: tm[k] for k in SCALARS},
               tables={k: tm[k] for k in ("auuc_table", "auuc_normalized_table", "auuc_random_table", "aecu_table")})
    if coll.rank() == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def _launch(world, csv, out_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank, args=(r, world, port, csv, out_path)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    with open(out_path) as f:
        return json.load(f)


def test_two_ranks_give_the_metrics_of_one_process(tmp_path):
    import pandas as pd
    csv = str(tmp_path / "uplift.csv")
    pd.DataFrame(uc.frame_data(1200, N_NUM, 5)).to_csv(csv, index=False)
    one = _launch(1, csv, str(tmp_path / "one.json"))
    two = _launch(2, csv, str(tmp_path / "two.json"))
    assert one["cloud_size"] == 1 and two["cloud_size"] == 2
    # the forests are equal (test_distributed_api.py); sums merged over two shards differ from one sum by rounding
    for k, v in one["scalars"].items():
        assert abs(v - two["scalars"][k]) <= 1e-9 * max(1.0, abs(v)), (k, v, two["scalars"][k])
    for k, tab in one["tables"].items():
        for c, v in tab.items():
            np.testing.assert_allclose(two["tables"][k][c], v, rtol=1e-9, atol=1e-9, err_msg=f"{k}.{c}")

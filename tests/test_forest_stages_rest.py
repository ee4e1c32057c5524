"""The ``leaf_node_assignment`` / ``predict_staged_proba`` / ``feature_frequencies`` fields of the Predictions routes
(what the h2o-py client sends for predict_leaf_node_assignment, staged_predict_proba, feature_frequencies) against
the facade's frames."""
import time

import pytest

pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from llama_github_io_amd.api.server import create_app  # noqa: E402
from llama_github_io_amd.core import dkv  # noqa: E402

import forest_stages_cases as fs  # noqa: E402


@pytest.fixture(scope="module")
def served():
    client = TestClient(create_app())
    fr = fs.training_frame()
    est = fs.estimator("gbm", "y", fr)
    mid, fid = est._model.key, fr.frame_id
    assert dkv.get(mid) is est._model and dkv.get(fid) is fr
    return client, est, fr, f"models/{mid}/frames/{fid}"


CALLS = {
    "path": (dict(leaf_node_assignment=True, leaf_node_assignment_type="Path"),
             lambda est, fr: est.predict_leaf_node_assignment(fr, "Path")),
    "node_id": (dict(leaf_node_assignment=True, leaf_node_assignment_type="Node_ID"),
                lambda est, fr: est.predict_leaf_node_assignment(fr, "Node_ID")),
    "default_type": (dict(leaf_node_assignment="true"), lambda est, fr: est.predict_leaf_node_assignment(fr)),
    "staged": (dict(predict_staged_proba=True), lambda est, fr: est.staged_predict_proba(fr)),
    "frequencies": (dict(feature_frequencies=True), lambda est, fr: est.feature_frequencies(fr)),
}


@pytest.mark.parametrize("which", list(CALLS))
def test_v3_fields(served, which):
    client, est, fr, url = served
    fields, facade = CALLS[which]
    r = client.post(f"/3/Predictions/{url}", data=dict(fields, predictions_frame=f"stages_{which}"))
    assert r.status_code == 200, r.text
    j = r.json()
    assert j["predictions_frame"]["name"] == f"stages_{which}"
    assert j["leaf_node_assignment"] is ("leaf_node_assignment" in fields)
    fs.frames_equal(dkv.get(f"stages_{which}"), facade(est, fr))


def test_v4_leaf_node_assignment_job(served):
    client, est, fr, url = served
    r = client.post(f"/4/Predictions/{url}", data=dict(leaf_node_assignment=True, leaf_node_assignment_type="Node_ID",
                                                       predictions_frame="stages_v4"))
    assert r.status_code == 200, r.text
    key = r.json()["key"]["name"]
    for _ in range(2000):
        job = client.get(f"/3/Jobs/{key}").json()["jobs"][0]
        if job["status"] in ("DONE", "FAILED", "CANCELLED"):
            break
        time.sleep(0.01)
    assert job["status"] == "DONE", job
    fs.frames_equal(dkv.get("stages_v4"), est.predict_leaf_node_assignment(fr, "Node_ID"))


def test_no_field_is_the_prediction(served):
    client, est, fr, url = served
    asked = client.post(f"/3/Predictions/{url}", data=dict(leaf_node_assignment=True)).json()
    assert asked["leaf_node_assignment"] is True
    for fields in (dict(), dict(leaf_node_assignment=False, predict_staged_proba="false")):
        j = client.post(f"/3/Predictions/{url}", data=dict(fields, predictions_frame="stages_plain")).json()
        assert set(j) == set(asked)
        assert j["leaf_node_assignment"] is False and j["predictions_frame"]["name"] == "stages_plain"
        assert j["reconstruction_error"] is False and j["exemplar_index"] == -1
        assert j["deep_features_hidden_layer"] == -1 and len(j["model_metrics"]) == 1
        fs.frames_equal(dkv.get("stages_plain"), est.predict(fr))

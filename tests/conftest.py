import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


_saved_tmp = None


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP) device")
    config.addinivalue_line("markers", "slow: long-running test")
    # The REST server keeps notebooks, exported models and cloud scratch under fixed names in the system temp
    # directory (h2o_nps/, <model_id>.zip, ...). Give the session a temp directory of its own, also for the servers
    # and ranks it starts, so a run never meets such files left behind by another user or an earlier run.
    global _saved_tmp
    if _saved_tmp is None:
        _saved_tmp = (os.environ.get("TMPDIR"), tempfile.tempdir)
        d = tempfile.mkdtemp(prefix="h2o_amd_tests_")
        os.environ["TMPDIR"] = tempfile.tempdir = d


def pytest_unconfigure(config):
    global _saved_tmp
    if _saved_tmp is not None:
        d = tempfile.tempdir
        env, tempfile.tempdir = _saved_tmp
        if env is None:
            os.environ.pop("TMPDIR", None)
        else:
            os.environ["TMPDIR"] = env
        _saved_tmp = None
        shutil.rmtree(d, ignore_errors=True)


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)

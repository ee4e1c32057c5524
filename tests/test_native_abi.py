"""The ctypes side of the native ABI against the built ``lib/libh2o_hip.so``. Loading the library needs no device
(it links against the HIP runtime that torch ships)."""
import ctypes
import importlib
import pkgutil

import pytest

import llama_github_io_amd.ops as ops_pkg
from llama_github_io_amd.ops import _native as nat
from llama_github_io_amd.ops import tree as T


def test_native_abi_matches_the_library():
    """Every launcher signature registered in ``_HIP_SIGS`` names an exported symbol (``_bind`` refuses a stale
    one), and the Python mirror of ``TreePlan`` has the size the library was compiled with."""
    # every ops module, and the model module that registers signatures of its own
    for m in pkgutil.iter_modules(ops_pkg.__path__):
        importlib.import_module(f"{ops_pkg.__name__}.{m.name}")
    importlib.import_module("llama_github_io_amd.models.datainfo")
    lib = nat.hip()
    assert len(nat._HIP_SIGS) > 30
    missing = [name for name in nat._HIP_SIGS if not hasattr(lib, name)]
    assert not missing, missing
    for name, args in nat._HIP_SIGS.items():
        assert getattr(lib, name).argtypes == args, name
    with pytest.raises(RuntimeError, match="h2o_no_such_launcher"):
        nat._bind(lib, {"h2o_no_such_launcher": [nat.c_void_p]})
    assert lib.h2o_tree_plan_size() == ctypes.sizeof(T._TreePlan)

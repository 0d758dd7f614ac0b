"""Own-nodes batches on the all-feature kernel (simon_set_own_nodes_all_feature), host side: the C-ABI surface, the Python option on the
context and on the engine, and the build lists that carry the new translation unit.  No GPU."""
import ctypes
import inspect
import os

import __graft_entry__ as entry
from open_simulator_amd import capi, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALL = "simon_set_own_nodes_all_feature"


def _header():
    with open(os.path.join(ROOT, "include", "simon_hip.h")) as f:
        return f.read()


def test_the_header_declares_the_call_and_capi_exports_it():
    hdr = _header()
    assert f"int {CALL}(simon_ctx* ctx, int32_t on);" in hdr
    assert CALL in capi.EXPORTS and capi.EXPORTS.count(CALL) == 1


def test_the_abi_stays_7_and_the_call_has_no_group_twin():
    hdr = _header()
    assert "#define SIMON_HIP_ABI_VERSION 7 " in hdr and capi.ABI_VERSION == 7
    assert "simon_group_set_own_nodes_all_feature" not in hdr
    assert not [n for n in capi.EXPORTS if n.startswith("simon_group_") and "own_nodes" in n]


def test_the_library_exports_the_symbol():
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, CALL) and lib.simon_hip_version() == 7
    assert not hasattr(lib, "simon_group_set_own_nodes_all_feature")
    assert lib.simon_set_own_nodes_all_feature(None, 1) == capi.EINVAL        # no context: refused before anything is touched


def test_the_engine_carries_the_flag_off_by_default():
    assert sim.HipEngine.supports_own_nodes_all_feature is False
    assert sim.HipEngine().supports_own_nodes_all_feature is False
    assert sim.HipEngine(own_nodes_all_feature=True).supports_own_nodes_all_feature is True
    assert sim.HipEngine(1, own_nodes_all_feature=True).device_id == 1
    sig = inspect.signature(sim.HipEngine.__init__)
    assert list(sig.parameters) == ["self", "device_id", "own_nodes_all_feature"]
    assert sig.parameters["device_id"].default == 0 and sig.parameters["own_nodes_all_feature"].default is False
    assert inspect.signature(capi.Context.set_own_nodes_all_feature).parameters["on"].default is True


def test_the_engine_sets_the_option_on_every_context_it_makes(monkeypatch):
    made = []

    class FakeContext:
        def __init__(self, device_id):
            self.device_id, self.option = device_id, None
            made.append(self)

        def set_own_nodes_all_feature(self, on=True):
            self.option = on

    monkeypatch.setattr(capi, "Context", FakeContext)
    sim.HipEngine(3)._context()
    sim.HipEngine(2, own_nodes_all_feature=True)._context()
    assert [(c.device_id, c.option) for c in made] == [(3, None), (2, True)]


def test_the_build_carries_the_new_unit():
    assert "simon_wide_own.hip" in entry.HIP_SOURCES
    assert entry.EXTRA_DEPS["simon_wide_own.hip"] == ["simon_wide.hip"]
    with open(os.path.join(entry.CSRC, "simon_wide_own.hip")) as f:
        unit = f.read()
    assert "#define SIMON_WIDE_OWN_TU" in unit and '#include "simon_wide.hip"' in unit

"""Explain on own-nodes batches (simon_explain_own_batch), host side: the C-ABI surface, and the roads above it -- sweep_failures(reasons=True)
and sweep_mix(reasons=True) -- on oracle-backed engines that implement explain_own_batch (explain_own_util): the same unscheduled_pods as
the replay road, without a single replay.  No GPU."""
import ctypes
import os
import re

import pytest

import evict_util as EU
import explain_own_util as OU
import mix_util as MU
import subset_util as SU
from open_simulator_amd import capi, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = """
int simon_explain_own_batch(simon_ctx* ctx, const int32_t* scenarios, int32_t n_scen, int32_t max_failed, int32_t max_bins,
                            int32_t* n_failed, int32_t* failed_pods, int32_t* n_bins, simon_fail_bin* bins,
                            uint16_t* fail_codes, int32_t code_stride)
"""


def _squash(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)).replace(" ,", ",").replace(" )", ")").strip()


def test_header_binding_and_library_carry_the_entry():
    header = _squash(open(os.path.join(ROOT, "include", "simon_hip.h")).read())
    assert _squash(PROTOTYPE) in header
    assert re.search(r"#define SIMON_HIP_ABI_VERSION 7\b", header)
    assert "simon_explain_own_batch" in capi.EXPORTS and capi.ABI_VERSION == 7
    assert not any(n.startswith("simon_group_explain") for n in capi.EXPORTS)     # no group forward
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, "simon_explain_own_batch") and lib.simon_hip_version() == 7
    assert sim.HipEngine.supports_explain_own and callable(sim.HipEngine.explain_own_batch) and callable(capi.Context.explain_own_batch)


def _no_replay(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("_failure_replay called: the batched explain was to tell")
    monkeypatch.setattr(sim, "_failure_replay", boom)


@pytest.mark.parametrize("reschedule", [False, "owned", "all"])
def test_sweep_failures_reasons_without_a_replay_on_the_live_cluster(reschedule, monkeypatch):
    cluster, apps = EU.live_cluster()
    if not reschedule:                   # (without rescheduling, a node-bound pod with an owner is refused: the cluster's own pods only)
        cluster = dict(cluster, Pod=[p for p in cluster["Pod"] if not p["metadata"].get("ownerReferences") or not p["spec"].get("nodeName")])
    want = sim.sweep_failures(cluster, apps, "node", engine=EU.EvictOracleEngine(), reschedule=reschedule, reasons=True)     # the parent road
    assert want.batched and any(want.unscheduled)
    _no_replay(monkeypatch)
    OU.OwnSubsetOracleEngine.own_calls = 0
    got = sim.sweep_failures(cluster, apps, "node", engine=OU.OwnSubsetOracleEngine(), reschedule=reschedule, reasons=True)
    assert got.batched and OU.OwnSubsetOracleEngine.own_calls == 1
    assert got.unscheduled == want.unscheduled and got.placements == want.placements
    assert got.unscheduled_pods == want.unscheduled_pods
    assert [len(lst) for lst in got.unscheduled_pods] == got.unscheduled
    for d, lst in enumerate(got.unscheduled_pods):                              # the node count is the scenario's own
        n_s = len(cluster["Node"]) - len(got.domains[d])
        assert all(f"0/{n_s} nodes are available" in u["reason"] for u in lst), d


def test_sweep_failures_reasons_without_a_replay_on_the_simple_example(monkeypatch):
    cluster, apps, _ = MU.example_simple()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    want = sim.sweep_failures(cluster, apps, "node", engine=SU.SubsetOracleEngine(), reasons=True)
    assert want.batched and any(want.unscheduled)
    _no_replay(monkeypatch)
    got = sim.sweep_failures(cluster, apps, "node", engine=OU.OwnSubsetOracleEngine(), reasons=True)
    assert got.batched and got.unscheduled_pods == want.unscheduled_pods and got.unscheduled == want.unscheduled
    # several chunks: one explain call per chunk that fails somewhere
    OU.OwnSubsetOracleEngine.own_calls = 0
    chunked = sim.sweep_failures(cluster, apps, "node", engine=OU.OwnSubsetOracleEngine(), reasons=True, batch_scenarios=2)
    assert chunked.unscheduled_pods == want.unscheduled_pods and OU.OwnSubsetOracleEngine.own_calls >= 2


def test_an_engine_without_the_call_and_a_refusal_take_the_replay_road(monkeypatch):
    cluster, apps = EU.live_cluster()
    want = sim.sweep_failures(cluster, apps, "node", engine=EU.EvictOracleEngine(), reschedule="owned", reasons=True)

    class Refusing(OU.OwnSubsetOracleEngine):
        def explain_own_batch(self, *a, **kw):
            e = capi.SimonError("simon_explain_own_batch failed (-5): the all-feature kernel takes prefix scenarios only")
            e.code = capi.ESTATE
            raise e

    got = sim.sweep_failures(cluster, apps, "node", engine=Refusing(), reschedule="owned", reasons=True)
    assert got.unscheduled_pods == want.unscheduled_pods


def test_sweep_mix_reasons_equal_simulate_of_every_mix():
    """A 3 x 3 grid on the simple example, with its app's DaemonSet (most failing mixes have a pod stream of their own and are listed from
    their own simulate(), simulate._same_stream) and without it (every failing mix is explained in the batch's one call)."""
    cluster, apps, types = MU.example_simple()
    counts = [[0, 1, 2], [0, 1, 3]]
    bare = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    for ap, all_batched in ((apps, False), (bare, True)):
        listed = []

        class Recording(OU.OwnSegmentOracleEngine):
            def explain_own_batch(self, prob, scen, orders, node_ranks, ids, *a, **kw):
                listed.append([int(s) for s in ids])
                assert kw.get("segments") is not None and kw.get("present") is None
                return super().explain_own_batch(prob, scen, orders, node_ranks, ids, *a, **kw)

        plain = sim.sweep_mix(cluster, ap, types, counts, engine=Recording())
        assert plain.batched and plain.unscheduled_pods == [] and listed == []           # the default changes nothing
        got = sim.sweep_mix(cluster, ap, types, counts, engine=Recording(), reasons=True)
        assert got.batched and len(got.counts) == 9 and len(got.unscheduled_pods) == 9
        assert (got.unscheduled, got.best, got.cost) == (plain.unscheduled, plain.best, plain.cost)
        failing = [s for s in range(9) if got.unscheduled[s] > 0]
        assert failing, "no mix of the grid leaves a pod unscheduled: nothing to explain"
        assert len(listed) == 1 and listed[0] and set(listed[0]) <= set(failing) and (not all_batched or listed[0] == failing)
        for s, mix in enumerate(got.counts):
            res, _, _ = MU.mix_answer(cluster, ap, types, mix)
            assert len(res.unscheduled_pods) == got.unscheduled[s], mix
            assert got.unscheduled_pods[s] == res.unscheduled_pods, mix
        # an engine without explain_own_batch: every failing mix from its own simulate(), the same lists
        slow = sim.sweep_mix(cluster, ap, types, counts, engine=MU.SegmentOracleEngine(), reasons=True)
        assert slow.unscheduled_pods == got.unscheduled_pods

"""Node-subset batches (simon_set_scenario_nodes, simulate.sweep_failures) on the host: the C-ABI surface, sweep_failures' batched road on
an oracle-backed engine against simulate() of every reduced cluster, bound pods, the fallbacks and argument checks, and the validator's
rules restated in numpy.  No GPU."""
import copy
import ctypes
import os

import numpy as np
import pytest

import mix_util as MU
import subset_util as SU
from open_simulator_amd import capi, k8s, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLUSTERS = {"simple": MU.example_simple, "simple_no_ds": lambda: _simple_without_app_daemonset(), "gpushare": MU.example_gpushare, "zoned": lambda: MU.random_zoned(11, n_nodes=14)}


def test_abi_declares_and_exports_the_subset_calls():
    with open(os.path.join(ROOT, "include", "simon_hip.h")) as f:
        hdr = f.read()
    assert "int simon_set_scenario_nodes(simon_ctx* ctx, const uint32_t* present" in hdr
    assert "int simon_fetch_node_ranks(simon_ctx* ctx, int32_t* rank" in hdr
    assert "#define SIMON_MAX_ZONES 64" in hdr and capi.MAX_ZONES == 64
    assert "simon_set_scenario_nodes" in capi.EXPORTS and "simon_fetch_node_ranks" in capi.EXPORTS
    assert "#define SIMON_HIP_ABI_VERSION 7 " in hdr and capi.ABI_VERSION == 7
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, "simon_set_scenario_nodes") and hasattr(lib, "simon_fetch_node_ranks") and lib.simon_hip_version() == 7
    assert sim.HipEngine.supports_scenario_subsets


def test_presence_words_layout():
    m = np.zeros((2, 70), bool)
    m[0, [0, 31, 32, 69]] = True
    m[1] = True
    w = capi.presence_words(m)
    assert w.dtype == np.uint32 and w.shape == (2, 3)
    assert w[0].tolist() == [1 | 1 << 31, 1, 1 << 5] and w[1].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, (1 << 6) - 1]


def _simple_without_app_daemonset():
    """example_simple with its app's DaemonSet taken out: with it the loss of worker-1 reorders the app's pods (ScheduleApp's unstable
    sorts see a shorter list), so that example runs scenario by scenario; without it the sweep is one batch."""
    cluster, apps, types = MU.example_simple()
    return cluster, [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps], types


def _domains(cluster, form):
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    if form == "node":
        return "node", [[n] for n in names]
    if form == "label":
        by = {}
        for n in cluster["Node"]:
            v = (n["metadata"].get("labels") or {}).get(k8s.LABEL_ZONE)
            if v is not None:
                by.setdefault(v, []).append(n["metadata"]["name"])
        return k8s.LABEL_ZONE, list(by.values())
    # neighbouring pairs (explicit domains may overlap); a cluster of two nodes: its nodes alone, last first
    pairs = [names[i:i + 2] for i in range(len(names) - 1)] if len(names) > 2 else [[n] for n in reversed(names)]
    return pairs, pairs


def _zoned_without_daemonset_app(name):
    cluster, apps, _ = CLUSTERS[name]()
    if name != "zoned":                   # the examples' nodes carry no zone label: give them two zones so that a label sweep has domains
        cluster = dict(cluster, Node=copy.deepcopy(cluster["Node"]))
        for j, n in enumerate(cluster["Node"]):
            n["metadata"].setdefault("labels", {})[k8s.LABEL_ZONE] = "za" if j % 3 else "zb"
    return cluster, apps


@pytest.mark.parametrize("form", ["node", "label", "pairs"])
@pytest.mark.parametrize("name", sorted(CLUSTERS))
def test_sweep_failures_on_the_oracle_engine_equals_simulate_of_every_reduced_cluster(name, form):
    cluster, apps = _zoned_without_daemonset_app(name)
    arg, doms = _domains(cluster, form)
    assert len(doms) >= 2 and all(len(d) < len(cluster["Node"]) for d in doms)
    if name == "simple":                    # its app holds a DaemonSet and the stream without worker-1 is not the cluster's: one by one, visibly
        with pytest.warns(sim.FailureFallbackWarning, match="pod order"):
            sw = sim.sweep_failures(cluster, apps, arg, engine=SU.SubsetOracleEngine())
        assert not sw.batched and "DaemonSet" in sw.fallback and sw.domains == doms
    else:
        sw = sim.sweep_failures(cluster, apps, arg, engine=SU.SubsetOracleEngine())
        assert sw.batched and sw.fallback is None and sw.domains == doms
    ref = SU.reduced_answers(cluster, apps, doms)
    assert len(sw.placements) == len(doms) + 1
    for s, (where, uns) in enumerate(ref):
        assert sw.placements[s] == where, s
        assert (sw.baseline["unscheduled"] if s == 0 else sw.unscheduled[s - 1]) == uns, s
    assert sw.critical == sorted((d for d in range(len(doms)) if not sw.survives[d]), key=lambda d: (-sw.unscheduled[d], d))
    assert all(ok == (u == 0) for ok, u in zip(sw.survives, sw.unscheduled))       # (no caps: only unscheduled pods decide)
    # the road without node subsets gives the same rows
    with pytest.warns(sim.FailureFallbackWarning, match="no node subsets"):
        each = sim.sweep_failures(cluster, apps, arg, engine=MU.OracleEngine())
    assert not each.batched and each.placements == sw.placements
    assert (each.unscheduled, each.cpu_pct, each.mem_pct, each.vg_pct, each.baseline) == (sw.unscheduled, sw.cpu_pct, sw.mem_pct, sw.vg_pct, sw.baseline)


def _bound(cluster, node_name):
    pod = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "pinned-db", "namespace": "default", "labels": {"app": "db"}},
           "spec": {"nodeName": node_name, "containers": [{"name": "c", "image": "db", "resources": {"requests": {"cpu": "500m", "memory": "256Mi"}}}]}}
    return dict(cluster, Pod=list(cluster.get("Pod", [])) + [pod])


def test_a_bound_pod_is_lost_exactly_in_its_node_s_scenario():
    cluster, apps, _ = _simple_without_app_daemonset()
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    cluster = _bound(cluster, names[1])
    sw = sim.sweep_failures(cluster, apps, "node", engine=SU.SubsetOracleEngine())
    assert sw.batched
    key = ("default", "pinned-db")
    assert sw.placements[0][key] == names[1]
    for d, dom in enumerate(sw.domains):
        if dom == [names[1]]:
            assert key not in sw.placements[d + 1]
        else:
            assert sw.placements[d + 1][key] == names[1]
    ref = SU.reduced_answers(cluster, apps, sw.domains)
    assert [w for w, _ in ref] == sw.placements


def test_fallbacks_are_visible_and_match():
    cluster, apps, _ = _simple_without_app_daemonset()
    with pytest.warns(sim.FailureFallbackWarning, match="no node subsets"):
        a = sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine())
    assert not a.batched and a.fallback == "the engine has no node subsets"
    with pytest.warns(sim.FailureFallbackWarning, match="DaemonSet"):          # (the reference example's own DaemonSet app does it too)
        b = sim.sweep_failures(cluster, MU.example_simple()[1], "node", engine=SU.SubsetOracleEngine())
    with_ds = MU.example_simple()[1]
    assert not b.batched and "DaemonSet" in b.fallback
    ref = SU.reduced_answers(cluster, with_ds, b.domains)
    assert [w for w, _ in ref] == b.placements and [u for _, u in ref][1:] == b.unscheduled

    class Refusing(SU.SubsetOracleEngine):
        def run(self, prob, scen, orders, present=None, **kw):
            if present is not None:
                err = capi.SimonError("simon_run_loaded failed (-4): node-subset batch on a problem the score-table kernel does not take")
                err.code = capi.ESTATE
                raise err
            return super().run(prob, scen, orders, **kw)

    with pytest.warns(sim.FailureFallbackWarning, match="refused"):
        c = sim.sweep_failures(cluster, apps, "node", engine=Refusing())
    assert not c.batched and c.placements == a.placements


def test_arguments_are_checked_and_critical_is_ordered():
    cluster, apps, _ = _simple_without_app_daemonset()
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    eng = SU.SubsetOracleEngine()
    with pytest.raises(ValueError, match="every node"):
        sim.sweep_failures(cluster, apps, [names], engine=eng)
    with pytest.raises(ValueError, match="unknown node"):
        sim.sweep_failures(cluster, apps, [["no-such-node"]], engine=eng)
    with pytest.raises(ValueError, match="empty failure domain"):
        sim.sweep_failures(cluster, apps, [[]], engine=eng)
    with pytest.raises(ValueError, match="no node carries the label"):
        sim.sweep_failures(cluster, apps, "example.com/rack", engine=eng)
    with pytest.raises(ValueError, match="not both"):
        sim.HipEngine().run(None, None, None, segments=([0], [[1]]), present=(np.ones((1, 1), bool), None))
    # critical: the domains that do not survive, most unscheduled pods first, ties in domain order
    rows = [(0, 10, 10, 0, False), (2, 10, 10, 0, False), (0, 10, 10, 0, False), (5, 10, 10, 0, False), (2, 10, 10, 0, False), (0, 90, 10, 0, False)]
    r = sim._failure_result([["a"], ["b"], ["c"], ["d"], ["e"]], rows, (50, 100, 100), [None] * 6, [], True, None)
    assert r.critical == [2, 0, 3, 4] and r.survives == [False, True, False, False, False] and r.baseline["survives"]
    # caps decide `survives` on a real sweep too
    free = sim.sweep_failures(cluster, apps, "node", engine=eng)
    tight = sim.sweep_failures(cluster, apps, "node", engine=eng, max_cpu=0)
    assert tight.unscheduled == free.unscheduled
    assert tight.survives == [u == 0 and c == 0 for u, c in zip(free.unscheduled, free.cpu_pct)] and any(c > 0 for c in free.cpu_pct)
    with_reasons = sim.sweep_failures(cluster, apps, "node", engine=eng, reasons=True)
    for d, lst in enumerate(with_reasons.unscheduled_pods):
        assert len(lst) == with_reasons.unscheduled[d]
        assert all(u["reason"] for u in lst)


# ---- the validator's rules, restated --------------------------------------------------------------------------------------------------
def _case():
    import randprob
    prob = randprob.rand_problem(5, N=40, P=60, gates=True, presets=True, init_state=True)
    prob, _ = MU.segmentable(prob, fixed=0)
    rng = np.random.default_rng(2)
    mask = rng.random((5, 40)) < 0.7
    mask[0] = True
    scen = np.stack([mask.sum(1), np.zeros(5, np.int64)], 1).astype(np.int32)
    return prob, scen, mask


def test_the_validator_rules_restated_in_numpy_on_hand_made_inputs():
    import dataclasses
    prob, scen, mask = _case()
    words = capi.presence_words(mask)
    zone = np.arange(40) % 3
    assert SU.subset_errors(prob, scen, words) == [] and SU.subset_errors(prob, scen, words, zone) == []
    w = words.copy()
    w[2, 1] |= np.uint32(1 << 9)                                       # node 41 of a 40-node pool
    assert "bits beyond N" in SU.subset_errors(prob, scen, w)
    s2 = scen.copy()
    s2[3, 0] += 1
    assert SU.subset_errors(prob, s2, words) == ["n_nodes mismatch"]
    w = words.copy()
    w[4] = 0
    s2 = scen.copy()
    s2[4, 0] = 0
    assert SU.subset_errors(prob, s2, w) == ["empty scenario"]
    assert SU.subset_errors(prob, scen, words, zone, n_zones=2) == ["zone ids"]
    assert SU.subset_errors(prob, scen, words, zone - 1) == ["zone ids"]
    assert SU.subset_errors(prob, scen, words, zone, n_zones=65) == ["n_zones"] and SU.subset_errors(prob, scen, words, zone, n_zones=0) == ["n_zones"]
    assert SU.subset_errors(prob, scen, words, np.arange(40) % 64, n_zones=64) == []
    lost = int(np.flatnonzero(~mask.all(0))[0])
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    busy = np.zeros(40, np.int32)
    busy[lost] = 1
    assert SU.subset_errors(capi.Problem(**dict(kw, init_npods=busy)).normalise(), scen, words) == ["init state"]
    kept = int(np.flatnonzero(mask.all(0))[0])
    busy = np.zeros(40, np.int32)
    busy[kept] = 1
    assert SU.subset_errors(capi.Problem(**dict(kw, init_npods=busy)).normalise(), scen, words) == []
    pre, gate = np.full(60, -1, np.int32), np.full(60, -1, np.int32)
    pre[7] = lost
    assert SU.subset_errors(capi.Problem(**dict(kw, preset_node=pre, gate_node=gate)).normalise(), scen, words) == ["preset"]
    gate[7] = lost                                                       # gated on its own node: accepted (unlike segments)
    assert SU.subset_errors(capi.Problem(**dict(kw, preset_node=pre, gate_node=gate)).normalise(), scen, words) == []
    pre[7] = gate[7] = kept
    gate[7] = -1                                                         # a node every scenario holds needs no gate
    assert SU.subset_errors(capi.Problem(**dict(kw, preset_node=pre, gate_node=gate)).normalise(), scen, words) == []


def test_rank_yardsticks_agree():
    """simulate.mix_node_ranks (pool dicts), subset_util.zone_ranks (zone ids, plain loops) and k8s.canonical_node_order of each scenario's
    own node list give the same rows: the yardsticks of the device staging."""
    rng = np.random.default_rng(0)
    for N, Z in ((1, 1), (33, 3), (70, 64), (65, 5)):
        zone = rng.integers(0, Z, N)
        pool = [{"metadata": {"name": f"n{j}", "labels": {k8s.LABEL_ZONE: f"z{zone[j]}"}}} for j in range(N)]
        mask = SU.staging_masks(N, zone, seed=N)
        assert mask.shape == (12, N) and mask.any(1).all()
        a, b = sim.mix_node_ranks(pool, mask), SU.zone_ranks(mask, zone)
        assert (a == b).all()
        for s in range(len(mask)):
            own = np.flatnonzero(mask[s])
            order = k8s.canonical_node_order([pool[j] for j in own])
            want = np.full(N, -1)
            want[own[order]] = np.arange(len(own))
            assert a[s].tolist() == want.tolist()

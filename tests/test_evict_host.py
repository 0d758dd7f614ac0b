"""Pod eviction (simon_set_pod_eviction, simulate.cluster_evicted, sweep_failures(reschedule=...)) on the host: the C-ABI surface,
cluster_evicted on a hand-written cluster, the rescheduling sweep on an oracle-backed engine against simulate() of every evicted
cluster, reschedule=False against the sweep as it was, the fallbacks, and the promise that a pod's class does not depend on
spec.nodeName.  No GPU."""
import copy
import ctypes
import os
import warnings

import numpy as np
import pytest

import evict_util as EU
import mix_util as MU
import subset_util as SU
from open_simulator_amd import capi, flatten as fl, k8s, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_the_eviction_call():
    with open(os.path.join(ROOT, "include", "simon_hip.h")) as f:
        hdr = f.read()
    assert "int simon_set_pod_eviction(simon_ctx* ctx, const uint8_t* evict" in hdr
    assert "#define SIMON_HIP_ABI_VERSION 7 " in hdr and capi.ABI_VERSION == 7
    assert "simon_set_pod_eviction" in capi.EXPORTS
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, "simon_set_pod_eviction") and lib.simon_hip_version() == 7
    assert sim.HipEngine.supports_pod_eviction and callable(capi.Context.set_pod_eviction)
    assert MU.unclassified_fields() == ([], [], [])                    # the flags travel as an argument: capi.Problem gained no field
    with pytest.raises(ValueError, match="present"):
        sim.HipEngine().run(None, None, None, evict=np.ones(1, bool))


def _names(pods):
    return [p["metadata"]["name"] for p in pods]


def test_cluster_evicted_on_a_hand_written_cluster():
    nodes = [{"metadata": {"name": n}} for n in ("a", "b", "c")]
    gpu = {k8s.GPU_INDEX: "0-1", k8s.GPU_ASSUME_TIME: "123", "keep": "me"}
    pods = [EU._pod("first", None, "1", "1Gi"),
            EU._pod("rs-0", "a", "1", "1Gi", ("ReplicaSet", "rs"), annotations=gpu),
            EU._pod("bare", "a", "1", "1Gi"),
            EU._pod("ds-a", "a", "1", "1Gi", ("DaemonSet", "ds")),
            EU._pod("mirror", "a", "1", "1Gi", ("Node", "a")),
            EU._pod("rs-1", "b", "1", "1Gi", ("ReplicaSet", "rs")),
            EU._pod("sts-0", "a", "1", "1Gi", ("StatefulSet", "sts")),
            EU._pod("last", "c", "1", "1Gi")]
    uncontrolled = EU._pod("loose", "a", "1", "1Gi", ("ReplicaSet", "x"))
    uncontrolled["metadata"]["ownerReferences"][0]["controller"] = False
    app_pods = [EU._pod("app-rs", "a", "1", "1Gi", ("Job", "j")), uncontrolled, EU._pod("app-free", None, "1", "1Gi")]
    cluster = {"Node": nodes, "Pod": pods}
    apps = [sim.AppResource("app", {"Pod": app_pods}), sim.AppResource("other", {"Deployment": []})]
    before = copy.deepcopy((cluster, [a.resource for a in apps]))
    cl, ap = sim.cluster_evicted(cluster, apps, ["a"], "owned")
    assert _names(cl["Node"]) == ["b", "c"]
    assert _names(cl["Pod"]) == ["first", "rs-0", "rs-1", "sts-0", "last"]           # position kept; bare / DaemonSet / mirror pods die
    assert _names(ap[0].resource["Pod"]) == ["app-rs", "app-free"] and ap[1] is apps[1]
    moved = {p["metadata"]["name"]: p for p in cl["Pod"] + ap[0].resource["Pod"]}
    for name in ("rs-0", "sts-0", "app-rs"):
        assert "nodeName" not in moved[name]["spec"] and "status" not in moved[name]
    assert moved["rs-0"]["metadata"]["annotations"] == {"keep": "me"}               # what Reserve / Bind wrote is gone
    assert moved["rs-1"]["spec"]["nodeName"] == "b" and moved["last"]["spec"]["nodeName"] == "c"
    assert moved["rs-1"] is pods[5]                                                 # untouched pods are the caller's objects
    cl, ap = sim.cluster_evicted(cluster, apps, ["a"], "all")
    assert _names(cl["Pod"]) == _names(pods) and _names(ap[0].resource["Pod"]) == _names(app_pods)
    assert all("nodeName" not in p["spec"] for p in cl["Pod"] if p["metadata"]["name"] not in ("rs-1", "last"))
    cl, ap = sim.cluster_evicted(cluster, apps, ["a", "c"], "owned")
    assert _names(cl["Node"]) == ["b"] and _names(cl["Pod"]) == ["first", "rs-0", "rs-1", "sts-0"]
    assert (cluster, [a.resource for a in apps]) == before                           # the inputs are not edited
    without = sim.cluster_without(cluster, apps, ["a"])
    assert _names(without[0]["Pod"]) == ["first", "rs-1", "last"]
    with pytest.raises(ValueError, match="neither"):
        sim.cluster_evicted(cluster, apps, ["a"], "some")


def _pairs(cluster):
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    return [names[i:i + 2] for i in range(len(names) - 1)] if len(names) > 2 else [[n] for n in reversed(names)]


@pytest.mark.parametrize("form", ["node", "pairs"])
@pytest.mark.parametrize("which", ["owned", "all"])
def test_rescheduling_sweep_equals_simulate_of_every_evicted_cluster(which, form):
    cluster, apps = EU.live_cluster()
    doms = [[n["metadata"]["name"]] for n in cluster["Node"]] if form == "node" else _pairs(cluster)
    sw = sim.sweep_failures(cluster, apps, "node" if form == "node" else doms, engine=EU.EvictOracleEngine(), reschedule=which, reasons=True)
    assert sw.batched and sw.fallback is None and sw.domains == doms
    ref = EU.evicted_answers(cluster, apps, doms, which)
    for s, (where, uns) in enumerate(ref):
        assert sw.placements[s] == where, s
        assert (sw.baseline["unscheduled"] if s == 0 else sw.unscheduled[s - 1]) == uns, s
    # the counters, from the definition: the evictable pods listed on the domain's nodes, and those of them the yardstick left unscheduled
    for d, names in enumerate(doms):
        mine = [p for p in cluster["Pod"] if (p["spec"].get("nodeName") in names) and sim.evictable(p, which)]
        assert sw.evicted[d] == len(mine) > 0
        assert sw.evicted_unscheduled[d] == sum(ref[d + 1][0][sim._pod_ref(p)] is None for p in mine)
        assert len(sw.unscheduled_pods[d]) == sw.unscheduled[d]
    assert sum(sw.evicted_unscheduled) > 0 and sum(sw.evicted) > sum(sw.evicted_unscheduled)
    assert sw.removable == [d for d in range(len(doms)) if sw.survives[d]]
    assert sorted(sw.removable + sw.critical) == list(range(len(doms)))
    # the rescheduled pods make a difference: dropping them instead leaves fewer pods unscheduled somewhere
    assert sw.unscheduled != [u for _, u in SU.reduced_answers(cluster, apps, doms)][1:]
    # the roads without the batch give the same rows, visibly
    with pytest.warns(sim.FailureFallbackWarning, match="supports_pod_eviction"):
        each = sim.sweep_failures(cluster, apps, "node" if form == "node" else doms, engine=SU.SubsetOracleEngine(), reschedule=which)
    assert not each.batched and "supports_pod_eviction" in each.fallback
    with pytest.warns(sim.FailureFallbackWarning, match="no node subsets"):
        slow = sim.sweep_failures(cluster, apps, "node" if form == "node" else doms, engine=MU.OracleEngine(), reschedule=which)
    for other in (each, slow):
        assert other.placements == sw.placements
        assert (other.unscheduled, other.cpu_pct, other.mem_pct, other.vg_pct, other.baseline, other.critical, other.removable, other.evicted,
                other.evicted_unscheduled) == (sw.unscheduled, sw.cpu_pct, sw.mem_pct, sw.vg_pct, sw.baseline, sw.critical, sw.removable,
                                               sw.evicted, sw.evicted_unscheduled)


def test_reschedule_false_is_the_sweep_as_it_was():
    cluster, apps, _ = MU.example_simple()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    seen = []

    class Recording(SU.SubsetOracleEngine):
        def run(self, prob, scen, orders, **kw):
            seen.append(sorted(kw))
            return super().run(prob, scen, orders, **kw)

    a = sim.sweep_failures(cluster, apps, "node", engine=Recording())
    b = sim.sweep_failures(cluster, apps, "node", engine=Recording(), reschedule=False)
    assert a.batched and b.batched and all("evict" not in kw for kw in seen)        # an engine that predates the flag is called as before
    assert a.placements == b.placements == [w for w, _ in SU.reduced_answers(cluster, apps, a.domains)]
    assert (a.unscheduled, a.cpu_pct, a.mem_pct, a.vg_pct, a.survives, a.baseline, a.critical) == \
           (b.unscheduled, b.cpu_pct, b.mem_pct, b.vg_pct, b.survives, b.baseline, b.critical)
    assert b.evicted == b.evicted_unscheduled == [0] * len(b.domains) and b.removable == [d for d, ok in enumerate(b.survives) if ok]
    # a node-bound pod with an owner is still refused without reschedule, and a template that binds its pods is refused with it
    live, live_apps = EU.live_cluster()
    with pytest.raises(fl.Unsupported, match="bound to node"):
        sim.sweep_failures(live, live_apps, "node", engine=EU.EvictOracleEngine())
    node = live["Node"][0]["metadata"]["name"]
    dep = {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "stuck", "namespace": "default"},
           "spec": {"replicas": 2, "selector": {"matchLabels": {"app": "stuck"}}, "template": {"metadata": {"labels": {"app": "stuck"}},
                    "spec": {"nodeName": node, "containers": [{"name": "c", "image": "i", "resources": {"requests": {"cpu": "100m", "memory": "64Mi"}}}]}}}}
    with pytest.raises(fl.Unsupported, match="by its template"):
        sim.sweep_failures(dict(live, Deployment=[dep]), live_apps, "node", engine=EU.EvictOracleEngine(), reschedule="owned")
    with pytest.raises(ValueError, match="neither"):
        sim.sweep_failures(live, live_apps, "node", engine=EU.EvictOracleEngine(), reschedule="sometimes")


def test_a_gpu_index_annotation_on_an_evicted_pod_falls_back_with_the_same_rows():
    cluster, apps = EU.live_cluster(heavy=False)
    cluster = dict(cluster, Pod=copy.deepcopy(cluster["Pod"]))
    next(p for p in cluster["Pod"] if p["metadata"]["name"] == "web-0")["metadata"]["annotations"] = {k8s.GPU_INDEX: "0"}   # (no GPU request: the text alone)
    with pytest.warns(sim.FailureFallbackWarning, match="gpu-index"):
        sw = sim.sweep_failures(cluster, apps, "node", engine=EU.EvictOracleEngine(), reschedule="owned")
    assert not sw.batched
    ref = EU.evicted_answers(cluster, apps, sw.domains, "owned")
    assert [w for w, _ in ref] == sw.placements and [u for _, u in ref][1:] == sw.unscheduled


def test_a_pod_s_class_and_request_do_not_depend_on_its_node_name():
    """The batch keeps ONE row per flagged pod for both of its lives: flatten must intern the same class, request and descriptors for a pod
    with and without spec.nodeName."""
    cluster, apps = EU.live_cluster()
    pool = cluster["Node"]
    pods, gates = sim.build_stream(cluster, apps, pool, 0)
    freed = [sim._recreated(p) if p["spec"].get("nodeName") else p for p in pods]
    a = fl.flatten(pool, pods, cluster.get("Service", []), gates=[-1] * len(pods)).problem
    b = fl.flatten(pool, freed, cluster.get("Service", []), gates=[-1] * len(pods)).problem
    assert (np.asarray(a.preset_node) >= 0).sum() == sum(bool(p["spec"].get("nodeName")) for p in pods) > 0 and b.preset_node is None
    for name in MU.problem_fields():
        if name in ("preset_node",):
            continue
        va, vb = getattr(a, name), getattr(b, name)
        if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
            assert va is not None and vb is not None and va.shape == vb.shape and (va == vb).all(), name
        else:
            assert va == vb, name


def test_the_oracle_engine_s_scenarios_are_the_scenarios_own_problems():
    """evict_util's yardstick on a hand-checkable case: two nodes, one flagged pod bound to the node that scenario 1 loses."""
    GiB = 1 << 30
    prob = capi.Problem(alloc_cpu=np.array([4000, 4000]), alloc_mem=np.array([8 * GiB, 8 * GiB]), alloc_pods=np.array([10, 10]),
                        req_cpu=np.array([3000, 3000, 3000]), req_mem=np.array([GiB, GiB, GiB]), pod_class=np.zeros(3, np.int32), n_pod_classes=1,
                        n_node_classes=1, node_class=np.zeros(2, np.int32), simon_raw=np.zeros((1, 1), np.int64), const_score=np.zeros(1, np.int64),
                        preset_node=np.array([1, -1, -1], np.int32)).normalise()
    evict = np.array([True, False, False])
    mask = np.array([[True, True], [True, False]])
    res = EU.EvictOracleEngine().run(prob, [[2, 0], [1, 0]], np.arange(3, dtype=np.int32)[None], present=(mask, None), evict=evict)
    assert res.placement[0].tolist() == [1, 0, capi.UNSCHEDULED]                     # bound to node 1, the next takes node 0, the third finds none
    assert res.placement[1].tolist() == [0, capi.UNSCHEDULED, capi.UNSCHEDULED]      # evicted: scheduled first, onto the node that is left
    assert res.unscheduled.tolist() == [1, 2]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert EU.evicted_here(prob, evict, mask[1]).tolist() == [True, False, False] and not EU.evicted_here(prob, evict, mask[0]).any()

"""Shared pieces of the pod-eviction tests (test_evict_host.py, test_gpu_evict.py): problems with pods flagged for eviction
(simon_set_pod_eviction), the yardstick -- the unmodified oracle on every scenario's OWN problem, where the pods evicted there carry no
preset -- an oracle-backed engine that honours `evict`, and a hand-made "live" cluster of controller-owned Running pods."""
import copy
import dataclasses
import functools

import numpy as np

import mix_util as MU
import subset_util as SU
from open_simulator_amd import capi, simulate as sim


def replaced(prob, **changes):
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    return capi.Problem(**dict(kw, **changes)).normalise()


def evicted_here(prob, evict, present_row):
    """bool [P]: the flagged pods whose preset node the scenario lacks."""
    pre = np.asarray(prob.preset_node)
    return np.asarray(evict, bool) & (pre >= 0) & ~np.asarray(present_row, bool)[np.maximum(pre, 0)]


def scenario_problem(prob, evict, present_row):
    """The scenario's own problem: the pods evicted there are ordinary pods (no preset)."""
    gone = evicted_here(prob, evict, present_row)
    return replaced(prob, preset_node=np.where(gone, -1, np.asarray(prob.preset_node)).astype(np.int32)), gone


def oracle_rows(prob, evict, mask, scen, orders, ranks, restricted=()):
    """[(placement row, oracle result, evicted-here)] per scenario, from oracle_of_scenario on the scenario's own problem; the scenarios
    listed in `restricted` also through oracle_of_restricted (asserted equal here: the two roads are each other's second opinion)."""
    out = []
    for s in range(len(mask)):
        ps, gone = scenario_problem(prob, evict, mask[s])
        row, ref = MU.oracle_of_scenario(ps, mask[s], orders[scen[s, 1]], None if ranks is None else ranks[s])
        if s in restricted:
            other, _ = MU.oracle_of_restricted(ps, mask[s], orders[scen[s, 1]], None if ranks is None else ranks[s])
            assert other.tolist() == row.tolist(), s
        out.append((row, ref, gone))
    return out


def eligible(prob):
    """Pods that may be flagged: no gate, no pin, no ephemeral-storage / extended-resource request (a preset pod with one keeps the
    problem off the score table), no gpu-index list of their own."""
    P = prob.n_pods
    ok = np.ones(P, bool)
    for name in ("gate_node", "pin_node"):
        v = getattr(prob, name)
        if v is not None:
            ok &= np.asarray(v) < 0
    if prob.preset_node is not None:
        ok &= np.asarray(prob.preset_node) < 0
    if prob.req_eph is not None:
        ok &= np.asarray(prob.req_eph) == 0
    if prob.scalar_req is not None and len(prob.scalar_req):
        ok &= (np.asarray(prob.scalar_req) == 0).all(0)
    if prob.scalar_entries is not None:
        ok &= np.asarray(prob.scalar_entries) == 0
    if prob.gpu_index is not None:
        ok &= np.asarray(prob.gpu_index) == 0
    return np.flatnonzero(ok)


def flag(prob, where, huge=None):
    """prob with pod p preset to node where[p] (no gate) and flagged; `huge`: a flagged pod given a cpu request twice the largest node's
    (bound without a filter it over-commits its node; evicted it fits nowhere).  Returns (problem, evict bool [P])."""
    P = prob.n_pods
    pre = np.full(P, -1, np.int32) if prob.preset_node is None else np.array(prob.preset_node, np.int32)
    gate = np.full(P, -1, np.int32) if prob.gate_node is None else np.array(prob.gate_node, np.int32)
    evict = np.zeros(P, bool)
    for p, j in where.items():
        assert pre[p] < 0 and gate[p] < 0
        pre[p], evict[p] = j, True
    changes = dict(preset_node=pre, gate_node=gate)
    if huge is not None:
        assert evict[huge]
        big = 2 * int(np.asarray(prob.alloc_cpu).max())
        req = np.array(prob.req_cpu, np.int64)
        req[huge] = big
        changes["req_cpu"] = req
        if prob.nz_cpu is not None:
            nz = np.array(prob.nz_cpu, np.int64)
            nz[huge] = big
            changes["nz_cpu"] = nz
    return replaced(prob, **changes), evict


@functools.lru_cache(maxsize=None)
def route_problem(case):
    """The small problems of test_gpu_mix._route_case, subset-ready (no initial state, every preset turned into a plain gate), plus one
    with more than 64 request signatures."""
    import randprob
    from test_gpu_mix import _route_case
    if case == "many_sigs":
        prob = randprob.rand_problem(23, N=48, P=300, gates=True, n_pod_classes=90, n_node_classes=6)
        orders = np.stack([np.arange(300), np.random.default_rng(23).permutation(300)]).astype(np.int32)
    else:
        prob, _, orders = _route_case(case)
    prob, _ = MU.segmentable(prob, fixed=0)
    return prob, np.asarray(orders, np.int32)


@functools.lru_cache(maxsize=None)
def route_case(case, seed=0):
    """(problem, evict, mask [S][N], zone, scen, orders, ranks, oracle rows) of one route case: flagged pods on three nodes -- t0, the
    smallest node, over-committed by the flagged pods bound to it; t1 with a pod that fits nowhere once evicted; t2 -- taken from as
    many pod classes as the eligible pods offer, and eight scenarios: every node; without t0; without all three; three nodes that hold
    none of the flagged pods; four seeded random rows.  The oracle's rows are computed once and shared."""
    prob, orders = route_problem(case)
    N = prob.n_nodes
    rng = np.random.default_rng(1000 + seed + sum(map(ord, case)))
    ok = eligible(prob)
    cls = np.asarray(prob.pod_class)[ok] if prob.pod_class is not None else np.zeros(len(ok), np.int64)
    by_cls = [ok[cls == c] for c in np.unique(cls)]
    picked, k = [], 0
    while len(picked) < 14 and any(k < len(b) for b in by_cls):       # round-robin over the classes
        picked += [int(b[k]) for b in by_cls if k < len(b)]
        k += 1
    picked = picked[:14]
    assert len(picked) >= 6
    t0 = int(np.argmin(np.asarray(prob.alloc_cpu)))
    t1, t2 = [int(j) for j in rng.choice(np.setdiff1d(np.arange(N), [t0]), 2, replace=False)]
    where = {p: (t1 if i == 0 else t2 if i % 4 == 1 else t0) for i, p in enumerate(picked)}
    prob, evict = flag(prob, where, huge=picked[0])
    mask = np.stack([rng.random(N) < q for q in (1.0, 1.0, 1.0, 0.0, 0.5, 0.7, 0.85, 0.95)])
    mask[0] = True
    mask[1, t0] = False
    mask[2, [t0, t1, t2]] = False
    mask[3, rng.choice(np.setdiff1d(np.arange(N), [t0, t1, t2]), 3, replace=False)] = True
    for s in range(4, 8):
        if not mask[s].any():
            mask[s, 0] = True
    mask[4, t1] = False                                                # (the pod that fits nowhere is evicted in a random row too)
    zone = rng.integers(0, 3, N).astype(np.int32)
    scen = np.stack([mask.sum(1), rng.integers(0, len(orders), len(mask))], 1).astype(np.int32)
    ranks = SU.zone_ranks(mask, zone)
    rows = oracle_rows(prob, evict, mask, scen, orders, ranks, restricted=(2, 5))
    return prob, evict, mask, zone, scen, orders, ranks, rows


def evicted_counts(rows):
    """(evicted pods the oracle placed, evicted pods it left unscheduled) over a case's scenarios."""
    placed = sum(int((row[gone] >= 0).sum()) for row, _, gone in rows)
    failed = sum(int((row[gone] == capi.UNSCHEDULED).sum()) for row, _, gone in rows)
    return placed, failed


class EvictOracleEngine(SU.SubsetOracleEngine):
    """Test-only engine that honours `evict`: scenario s runs on the oracle with the pods evicted there stripped of their preset."""
    supports_pod_eviction = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, evict=None):
        if evict is None:
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices, present)
        assert present is not None
        mask, zone = present
        scen = capi.scenarios_array(scen)
        res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
        for s in range(len(scen)):
            ps, _ = scenario_problem(prob, evict, np.asarray(mask)[s])
            one = super().run(ps, scen[s:s + 1], orders, want_placement, None if node_ranks is None else node_ranks[s:s + 1], want_gpu_slices,
                              (np.asarray(mask)[s:s + 1], zone))
            res.placement[s], res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = one.placement[0], one.unscheduled[0], one.used_cpu[0], one.used_mem[0]
            if want_gpu_slices and one.gpu_slices is not None:
                res.gpu_slices[s] = one.gpu_slices[0]
            if res.used_vg is not None and one.used_vg is not None:
                res.used_vg[s] = one.used_vg[0]
            if one.preempt_risk is not None:
                if res.preempt_risk is None:
                    res.preempt_risk = np.zeros(len(scen), np.uint8)
                res.preempt_risk[s] = one.preempt_risk[0]
        return res


# ---- a hand-made live cluster ----------------------------------------------------------------------------------------------------------
def _pod(name, node, cpu, mem, owner=None, labels=None, annotations=None, namespace="default"):
    md = {"name": name, "namespace": namespace, "labels": dict(labels or {"app": name.rsplit("-", 1)[0]})}
    if annotations:
        md["annotations"] = dict(annotations)
    if owner:
        md["ownerReferences"] = [{"apiVersion": "apps/v1", "kind": owner[0], "name": owner[1], "controller": True}]
    spec = {"containers": [{"name": "c", "image": "img", "resources": {"requests": {"cpu": cpu, "memory": mem}}}]}
    if node:
        spec["nodeName"] = node
    return {"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": spec, "status": {"phase": "Running"}}


def live_cluster(heavy=True):
    """The reference's example cluster (tests/golden/example, cluster/demo_1) ingested the way a live one is: its app (without the
    DaemonSet, whose pods would reorder the app's stream per node set) plus Running pods bound to the nodes -- ReplicaSet- and
    StatefulSet-owned ones, a DaemonSet-owned one, a mirror pod (owner kind Node) and a bare pod.  heavy: the ReplicaSet pods of the
    first worker are large enough that not all of them find room elsewhere."""
    cluster, apps, _ = MU.example_simple()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    cluster = dict(cluster, Node=copy.deepcopy(cluster["Node"]))
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    pods = []
    for i, n in enumerate(names):
        pods.append(_pod(f"web-{i}", n, "500m", "256Mi", ("ReplicaSet", "web")))
        pods.append(_pod(f"agent-{i}", n, "100m", "64Mi", ("DaemonSet", "agent")))
    big = "6" if heavy else "1"
    for k in range(3):
        pods.append(_pod(f"batch-{k}", names[-1], big, "1Gi", ("ReplicaSet", "batch")))
    pods.append(_pod("db-0", names[0], "1", "1Gi", ("StatefulSet", "db")))
    pods.append(_pod("mirror-0", names[0], "200m", "64Mi", ("Node", names[0])))
    pods.append(_pod("bare-0", names[1 % len(names)], "200m", "64Mi"))
    pods.append(_pod("floating-0", None, "300m", "128Mi", ("ReplicaSet", "floating")))
    return dict(cluster, Pod=list(cluster.get("Pod", [])) + pods), apps


def evicted_answers(cluster, apps, doms, which, engine=None):
    """simulate() of the whole cluster and of cluster_evicted(...) for every domain, on the oracle: [(where, unscheduled count)]."""
    engine = engine or MU.OracleEngine()
    out = []
    for names in [[]] + list(doms):
        res = sim.simulate(*sim.cluster_evicted(cluster, apps, names, which), engine=engine)
        out.append((SU.names_of(res), len(res.unscheduled_pods)))
    return out

"""N-1 with rescheduling, end to end: simulate.sweep_failures(domains="node", reschedule="owned") over a synthetic LIVE cluster of config
3's size, next to simulate(*cluster_evicted(...)) of ten of its scenarios one by one, and the cost of a bound pod's cycle against a
scheduled pod's on the same batch (profiles/evictions/README.md).

    python profiles/evictions/n1_evict.py [n_nodes] [n_workloads]

The live cluster: profiles/subsets/n1_sweep.py's objects (seed 3) scheduled once as a whole; every pod that found a node becomes a
Running pod under "Pod" with spec.nodeName and its controller's ownerReference (ReplicaSet for the Deployments' pods, DaemonSet for the
agent's; these lose the per-node affinity the expansion gave them, see live_cluster), the workloads themselves are dropped, the
Services stay.  A sweep that falls back is an error here, not a record."""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "subsets"))

import numpy as np  # noqa: E402
from open_simulator_amd import capi, simulate as sim  # noqa: E402
from n1_sweep import cluster_objects  # noqa: E402


def live_cluster(n_nodes, n_workloads):
    cluster, apps = cluster_objects(n_nodes, n_workloads)
    res = sim.simulate(cluster, apps, engine=sim.HipEngine())
    pods = [p for st in res.node_status for p in st["pods"]]
    for p in pods:
        # a DaemonSet pod's affinity names its node (matchFields metadata.name): one pod class per node, 1 512 request signatures, beyond
        # what the score table holds -- such a cluster sweeps scenario by scenario.  The pod is bound by spec.nodeName and dies with its
        # node, so the affinity decides nothing here: dropped, and the agents share one class
        if any(o.get("kind") == "DaemonSet" for o in p["metadata"].get("ownerReferences") or []):
            p["spec"] = {k: v for k, v in p["spec"].items() if k != "affinity"}
    live = {k: v for k, v in cluster.items() if k not in ("DaemonSet", "Pod")}
    return dict(live, Pod=pods), len(res.unscheduled_pods)


class TimedEngine(sim.HipEngine):
    """HipEngine.run with a clock around every step of a node-subset batch; keeps the batch's problem and flags."""

    def __init__(self):
        super().__init__()
        self.t = {"load": 0.0, "staging": 0.0, "run": 0.0}
        self.launches = []

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, segments=None, present=None, evict=None):
        if present is None:
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices, segments)
        self.batch = (prob, scen, orders, present, evict)
        with capi.Context(self.device_id) as ctx:
            t0 = time.perf_counter()
            ctx.load_problem(prob)
            if evict is not None:
                ctx.set_pod_eviction(evict)
            ctx.load_scenarios(scen, orders)
            t1 = time.perf_counter()
            ctx.set_scenario_nodes(*present)
            t2 = time.perf_counter()
            ctx.run_loaded(want_placement, want_gpu_slices)
            res = ctx.fetch(want_placement, want_gpu_slices)
            t3 = time.perf_counter()
            self.last_stats = ctx.stats()
            self.t["load"] += t1 - t0
            self.t["staging"] += t2 - t1
            self.t["run"] += t3 - t2
            self.launches.append((len(scen), int(self.last_stats.n_launches), int(self.last_stats.kernel_generation), float(self.last_stats.kernel_ms)))
            return res


def kernel_ms(prob, scen, orders, present, evict, repeats=3):
    """kernel_ms of the batch run `repeats` times on one context (the first run of a context is left out)."""
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        if evict is not None:
            ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(*present)
        out = []
        for _ in range(repeats + 1):
            ctx.run_loaded(False)
            out.append(round(float(ctx.stats().kernel_ms), 3))
        return out[1:], int(ctx.stats().kernel_generation)


def main():
    import dataclasses
    n_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 1512
    n_workloads = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    warnings.simplefilter("error", sim.FailureFallbackWarning)
    live, left_out = live_cluster(n_nodes, n_workloads)
    eng = TimedEngine()
    t0 = time.perf_counter()
    sw = sim.sweep_failures(live, [], "node", engine=eng, reschedule="owned")
    total = time.perf_counter() - t0
    assert sw.batched
    names = [n["metadata"]["name"] for n in live["Node"]]
    rng = np.random.default_rng(0)
    one = []
    for d in rng.choice(len(names), 10, replace=False).tolist():
        t0 = time.perf_counter()
        res = sim.simulate(*sim.cluster_evicted(live, [], [names[d]], "owned"), engine=sim.HipEngine())
        one.append(round(time.perf_counter() - t0, 3))
        assert len(res.unscheduled_pods) == sw.unscheduled[d], (d, len(res.unscheduled_pods), sw.unscheduled[d])
    engine = sum(eng.t.values())
    prob, scen, orders, present, evict = eng.batch
    P, S = prob.n_pods, len(scen)
    # the bound cycle against the scheduled cycle: the same S scenarios with every node present -- every node-bound pod takes the bound
    # branch -- and the same batch with the presets taken away -- every pod is scheduled.  One wave per scenario and all of them resident,
    # so kernel time / P is the time of one cycle
    full = (np.ones_like(present[0]), present[1])
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    free = capi.Problem(**dict(kw, preset_node=None, gate_node=None)).normalise()
    scen_full = np.stack([np.full(S, prob.n_nodes), scen[:, 1]], 1).astype(np.int32)
    sweep_ms, gen = kernel_ms(prob, scen, orders, present, evict)
    bound_ms, _ = kernel_ms(prob, scen_full, orders, full, evict)
    free_ms, gen_free = kernel_ms(free, scen_full, orders, full, None)
    n_bound = int((np.asarray(prob.preset_node) >= 0).sum())
    print(json.dumps({"nodes": n_nodes, "pods": P, "bound_pods": n_bound, "flagged_pods": int(np.asarray(evict).sum()), "left_unscheduled_by_the_whole_cluster_run": left_out,
                      "scenarios": S, "batched": sw.batched, "total_s": round(total, 3), "flatten_s": round(total - engine, 3),
                      "load_s": round(eng.t["load"], 3), "staging_s": round(eng.t["staging"], 3), "run_s": round(eng.t["run"], 3),
                      "launches (scenarios, launches, generation, kernel ms)": eng.launches,
                      "kernel_us_per_scenario": round(1000 * eng.launches[0][3] / S, 2),
                      "evicted_total": int(sum(sw.evicted)), "evicted_unscheduled_total": int(sum(sw.evicted_unscheduled)),
                      "critical": len(sw.critical), "removable": len(sw.removable),
                      "simulate_s_each": one, "simulate_s_median": float(np.median(one)),
                      "kernel_ms sweep (generation %d)" % gen: sweep_ms, "kernel_ms all nodes present, every pod bound": bound_ms,
                      "kernel_ms all nodes present, presets removed (generation %d)" % gen_free: free_ms,
                      "us per bound cycle": round(1000 * float(np.median(bound_ms)) / P, 3),
                      "us per scheduled cycle": round(1000 * float(np.median(free_ms)) / P, 3)}))


if __name__ == "__main__":
    main()

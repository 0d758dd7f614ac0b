"""N-1 end to end: simulate.sweep_failures(domains="node") over a cluster of config 3's size, its wall time in three parts, next to
simulate() of ten of its scenarios one by one (profiles/subsets/README.md).

    python profiles/subsets/n1_sweep.py [n_nodes] [n_workloads]

The cluster is Kubernetes objects (seed 3): nodes in three shapes over three zones, Deployments behind Services (soft spread
constraints: generation 7 of the score-table kernel), one cluster DaemonSet.  flatten = everything outside the engine (domains, pod
stream, flatten, the result rows); staging = simon_set_scenario_nodes; run = run_loaded + fetch.  A sweep that falls back is an error
here, not a record."""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from open_simulator_amd import capi, k8s, simulate as sim  # noqa: E402


def cluster_objects(n_nodes, n_workloads, seed=3):
    rng = np.random.default_rng(seed)
    nodes = []
    for j in range(n_nodes):
        cpu, mem = [("8", "16Gi"), ("16", "32Gi"), ("32", "64Gi")][int(rng.integers(0, 3))]
        nodes.append({"apiVersion": "v1", "kind": "Node", "metadata": {"name": f"node-{j}", "labels": {k8s.LABEL_HOSTNAME: f"node-{j}", k8s.LABEL_ZONE: f"z{j % 3}"}},
                      "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": "110"}, "capacity": {"cpu": cpu, "memory": mem}}})
    objs = []
    for w in range(n_workloads):
        app = f"app{w}"
        spec = {"containers": [{"name": "c", "image": "busybox", "resources": {"requests": {
            "cpu": str(rng.choice(["100m", "250m", "500m", "1", "2"])), "memory": str(rng.choice(["128Mi", "256Mi", "1Gi", "2Gi"]))}}}]}
        objs.append({"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": app, "namespace": "default"},
                     "spec": {"replicas": int(rng.integers(20, 181)), "selector": {"matchLabels": {"app": app}},
                              "template": {"metadata": {"labels": {"app": app}}, "spec": spec}}})
    services = [{"apiVersion": "v1", "kind": "Service", "metadata": {"name": f"svc-{w}", "namespace": "default"}, "spec": {"selector": {"app": f"app{w}"}}}
                for w in range(n_workloads) if w % 5]
    ds = [{"apiVersion": "apps/v1", "kind": "DaemonSet", "metadata": {"name": "agent", "namespace": "kube-system"},
           "spec": {"selector": {"matchLabels": {"app": "agent"}}, "template": {"metadata": {"labels": {"app": "agent"}},
                    "spec": {"containers": [{"name": "a", "image": "x", "resources": {"requests": {"cpu": "100m", "memory": "128Mi"}}}]}}}}]
    return k8s.group_resources(nodes + services + ds), [sim.AppResource("app", k8s.group_resources(objs))]


class TimedEngine(sim.HipEngine):
    """HipEngine.run with a clock around every step of a node-subset batch."""

    def __init__(self):
        super().__init__()
        self.t = {"load": 0.0, "staging": 0.0, "run": 0.0}
        self.launches = []

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, segments=None, present=None):
        if present is None:
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices, segments)
        with capi.Context(self.device_id) as ctx:
            t0 = time.perf_counter()
            ctx.load_problem(prob)
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


def main():
    n_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 1512
    n_workloads = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    warnings.simplefilter("error", sim.FailureFallbackWarning)
    cluster, apps = cluster_objects(n_nodes, n_workloads)
    with capi.Context(0):                                                                 # (device and library warm before the clock starts)
        pass
    eng = TimedEngine()
    t0 = time.perf_counter()
    sw = sim.sweep_failures(cluster, apps, "node", engine=eng)
    total = time.perf_counter() - t0
    names = [n["metadata"]["name"] for n in cluster["Node"]]
    rng = np.random.default_rng(0)
    one = []
    for d in rng.choice(len(names), 10, replace=False).tolist():
        t0 = time.perf_counter()
        res = sim.simulate(*sim.cluster_without(cluster, apps, [names[d]]), engine=sim.HipEngine())
        one.append(round(time.perf_counter() - t0, 3))
        assert len(res.unscheduled_pods) == sw.unscheduled[d], (d, len(res.unscheduled_pods), sw.unscheduled[d])
    engine = sum(eng.t.values())
    print(json.dumps({"nodes": n_nodes, "pods": len(sw.placement(0)), "scenarios": len(sw.domains) + 1, "batched": sw.batched,
                      "total_s": round(total, 3), "flatten_s": round(total - engine, 3), "load_s": round(eng.t["load"], 3),
                      "staging_s": round(eng.t["staging"], 3), "run_s": round(eng.t["run"], 3),
                      "launches (scenarios, launches, generation, kernel ms)": eng.launches,
                      "critical": len(sw.critical), "baseline_unscheduled": sw.baseline["unscheduled"],
                      "simulate_s_each": one, "simulate_s_median": float(np.median(one))}))


if __name__ == "__main__":
    main()

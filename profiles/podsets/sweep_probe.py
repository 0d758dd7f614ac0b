#!/usr/bin/env python3
"""What sweep_apps buys: all 4 096 subsets of 12 apps on a typical cluster (profiles/e2e_sweep.py --typical's objects: Deployments behind
Services, anti-affinity, zone constraints, tolerations, node selectors) in pod-subset batches, end to end, against the same subsets through
simulate() one by one -- a SAMPLE of the one-by-one runs is timed and the total extrapolated.
usage: python profiles/podsets/sweep_probe.py [--nodes 500] [--workloads 120] [--max-replicas 50] [--sample 64]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                  # noqa: E402
import randk8s                                                      # noqa: E402
from open_simulator_amd import k8s, simulate as sim, synth          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=500)
    ap.add_argument("--workloads", type=int, default=120)
    ap.add_argument("--max-replicas", type=int, default=50)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    nodes, workloads, services = synth.typical_cluster_objects(1, a.nodes, a.workloads, a.max_replicas)
    for j, n in enumerate(nodes):
        n["metadata"]["labels"][randk8s.ZONE] = f"z{j % 3}"
        n["status"]["allocatable"]["pods"] = "110"
    cluster = k8s.group_resources(nodes + services)
    apps = [sim.AppResource(f"app{i}", k8s.group_resources(workloads[i::12])) for i in range(12)]
    eng = sim.HipEngine()
    sim.sweep_apps(cluster, apps[:2], engine=eng)                    # (warm-up: library load, first context)
    t0 = time.perf_counter()
    res = sim.sweep_apps(cluster, apps, engine=eng)
    t_batch = time.perf_counter() - t0
    assert res.batched, res.fallback
    rng = np.random.default_rng(0)
    pick = sorted(rng.choice(len(res.subsets), a.sample, replace=False).tolist())
    t0 = time.perf_counter()
    for u in pick:
        sub = [apps[i] for i in res.subsets[u]]
        n_pods = sum(len(x) for app in sub for x in app.resource.values())
        if not n_pods:
            continue
        one = sim.simulate(cluster, sub, engine=eng)
        assert len(one.unscheduled_pods) == res.unscheduled[u][0], (u, len(one.unscheduled_pods), res.unscheduled[u][0])
    t_each = time.perf_counter() - t0
    print("SWEEP " + json.dumps({"nodes": a.nodes, "workloads": a.workloads, "apps": 12, "scenarios": len(res.subsets),
                                 "sweep_apps_s": round(t_batch, 3), "kernel_variant": int(eng.last_stats.kernel_variant), "kernel_generation": int(eng.last_stats.kernel_generation),
                                 "kernel_ms": round(float(eng.last_stats.kernel_ms), 3), "sampled": len(pick), "sampled_simulate_s": round(t_each, 3),
                                 "extrapolated_one_by_one_s": round(t_each / len(pick) * len(res.subsets), 1),
                                 "speedup_extrapolated": round(t_each / len(pick) * len(res.subsets) / t_batch, 1),
                                 "fitting_subsets": int(sum(f[0] for f in res.fits)), "maximal": len(res.maximal), "best": res.best}), flush=True)


if __name__ == "__main__":
    main()

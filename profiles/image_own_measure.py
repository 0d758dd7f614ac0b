"""Measurements of the own-nodes image states (docs/KERNELS.md 5.6): run from the repository root on the GPU.

1. simon_set_scenario_nodes on a 1 000-node failure sweep (1 001 scenarios, about half of the nodes listing a 500 MB image the pods run):
   image_states_kernel against SIMON_IMAGE_STAGE=host.  The call also builds the subset arrays and re-stages the tables, in both.
2. sweep_failures on a 200-node image cluster: the batched road against the one-by-one road (an engine without supports_image_own_nodes
   takes the fallback, which is what the sweep ran before the feature).

Warm, the median of --runs runs (default 5) after one that is thrown away.  Prints one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def staging(runs):
    import image_own_util as U
    import mix_util as MU
    import randprob
    import evict_util as EU
    from open_simulator_amd import capi
    N = 1000
    rng = np.random.default_rng(1)
    prob, _ = MU.segmentable(randprob.rand_problem(1, N=N, P=400, n_node_classes=5, n_pod_classes=20), fixed=0)
    lists = [rng.random(N) < 0.5]
    sizes = [np.full(N, 500 << 20)]
    im = U.pool_order_image(rng, N, lists, [[0]] * 20, sizes)
    prob = EU.replaced(prob, image_locality=im)
    masks = np.stack([np.ones(N, bool)] + [np.arange(N) != j for j in range(N)])
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    orders = np.arange(prob.n_pods, dtype=np.int32)[None]
    out = {}
    for stage in ("device", "host"):
        if stage == "host":
            os.environ["SIMON_IMAGE_STAGE"] = "host"
        else:
            os.environ.pop("SIMON_IMAGE_STAGE", None)
        with capi.Context(0) as ctx:
            ctx.load_problem(prob)
            times = []
            for r in range(runs + 1):
                ctx.load_scenarios(scen, orders)
                t = time.perf_counter()
                ctx.set_scenario_nodes(masks)
                times.append(time.perf_counter() - t)
            out[stage] = {"median_ms": round(1e3 * statistics.median(times[1:]), 2), "runs_ms": [round(1e3 * x, 2) for x in times[1:]]}
            try:                                                      # (so many listing nodes may leave the score table: the route is part of the record)
                ctx.run_loaded(True, False)
            except capi.SimonError as e:
                out[stage]["refused_without_opt_in"] = str(e)
                ctx.set_own_nodes_all_feature(True)
                ctx.run_loaded(True, False)
            st = ctx.stats()
            out[stage].update(kernel_variant=int(st.kernel_variant), kernel_generation=int(st.kernel_generation), run_ms=round(float(st.kernel_ms), 2))
    os.environ.pop("SIMON_IMAGE_STAGE", None)
    print(json.dumps({"what": "set_scenario_nodes, 1000 nodes x 1001 scenarios", **out}), flush=True)


def failures(runs, batched_only=False):
    import image_util as IU
    from open_simulator_amd import simulate as sim

    class OneByOne(sim.HipEngine):
        supports_image_own_nodes = False

    import image_own_util as U
    cluster, apps, _ = IU.image_sweep_case(0, n_nodes=200, n_workloads=60, listing_share=0.6)
    U.table_friendly(apps)                                            # (what only the all-feature kernel takes goes: the batch is to show the score table's route)
    out = {}
    for name, eng in (("batched", sim.HipEngine()), ("batched_all_feature_opt_in", sim.HipEngine(own_nodes_all_feature=True)),
                      ("one_by_one", OneByOne()))[:2 if batched_only else 3]:
        times = []
        for r in range(runs + 1):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t = time.perf_counter()
                res = sim.sweep_failures(cluster, apps, "node", engine=eng)
                times.append(time.perf_counter() - t)
        st = eng.last_stats
        out[name] = {"median_s": round(statistics.median(times[1:]), 3), "runs_s": [round(x, 3) for x in times[1:]], "batched": bool(res.batched),
                     "fallback": res.fallback, "kernel_variant": None if st is None else int(st.kernel_variant),
                     "kernel_generation": None if st is None else int(st.kernel_generation), "unscheduled_sum": int(sum(res.unscheduled))}
    print(json.dumps({"what": "sweep_failures, 200 nodes x 201 scenarios", **out}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=["staging", "failures"])
    ap.add_argument("--batched-only", action="store_true", help="sweep_failures: skip the one-by-one road (a route trace with SIMON_DEBUG_ROUTE=1)")
    a = ap.parse_args()
    if a.only != "failures":
        staging(a.runs)
    if a.only != "staging":
        failures(a.runs, a.batched_only)

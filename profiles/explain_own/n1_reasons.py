"""N-1 with rescheduling AND reasons, end to end: simulate.sweep_failures(domains="node", reschedule="owned", reasons=True) over the
synthetic live cluster of profiles/evictions/n1_evict.py, sized so that most nodes are critical (profiles/explain_own/README.md).

    python profiles/explain_own/n1_reasons.py [n_nodes] [n_workloads] [repeats]

Prints one JSON line: the sweep's wall time per repeat, the failing domains, and -- where the engine explains own-nodes batches
(HipEngine.supports_explain_own) -- the time inside HipEngine.explain_own_batch and inside the simon_explain_own_batch calls alone.
The script only uses what both roads share, so a copy of it in a checkout of the commit before times that commit's road (one simulate()
per failing domain) on the same box: run the two alternately and take the best of each.  A sweep that falls back is an error here."""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "evictions"))

from open_simulator_amd import capi, simulate as sim  # noqa: E402
from n1_evict import live_cluster  # noqa: E402


def main():
    n_nodes = int(sys.argv[1]) if len(sys.argv) > 1 else 160
    n_workloads = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    warnings.simplefilter("error", sim.FailureFallbackWarning)
    live, left_out = live_cluster(n_nodes, n_workloads)
    own = getattr(sim.HipEngine, "supports_explain_own", False)
    spent = {"engine": 0.0, "library": 0.0, "calls": 0, "replays": 0}
    if own:
        lib_call, eng_call = capi.Context.explain_own_batch, sim.HipEngine.explain_own_batch

        def timed_lib(self, *a, **kw):
            t0 = time.perf_counter()
            try:
                return lib_call(self, *a, **kw)
            finally:
                spent["library"] += time.perf_counter() - t0
                spent["calls"] += 1

        def timed_eng(self, *a, **kw):
            t0 = time.perf_counter()
            try:
                return eng_call(self, *a, **kw)
            finally:
                spent["engine"] += time.perf_counter() - t0

        capi.Context.explain_own_batch, sim.HipEngine.explain_own_batch = timed_lib, timed_eng
    replay = sim._failure_replay

    def counted(*a, **kw):
        spent["replays"] += 1
        return replay(*a, **kw)

    sim._failure_replay = counted
    walls, plain = [], []
    for _ in range(repeats):
        for k in spent:
            spent[k] = 0
        t0 = time.perf_counter()
        sw = sim.sweep_failures(live, [], "node", engine=sim.HipEngine(), reschedule="owned", reasons=True)
        walls.append(round(time.perf_counter() - t0, 3))
        t0 = time.perf_counter()
        sim.sweep_failures(live, [], "node", engine=sim.HipEngine(), reschedule="owned")
        plain.append(round(time.perf_counter() - t0, 3))
    assert sw.batched and [len(lst) for lst in sw.unscheduled_pods] == sw.unscheduled
    print(json.dumps({"nodes": n_nodes, "pods": len(live["Pod"]), "left_unscheduled_by_the_whole_cluster_run": left_out,
                      "failing_domains": sum(u > 0 for u in sw.unscheduled), "unscheduled_pods_listed": sum(sw.unscheduled),
                      "explains_own_batches": bool(own), "sweep_with_reasons_s": walls, "sweep_without_reasons_s": plain,
                      "simulate_replays (last repeat)": spent["replays"], "simon_explain_own_batch calls (last repeat)": spent["calls"],
                      "in HipEngine.explain_own_batch_s (last repeat)": round(spent["engine"], 3),
                      "in simon_explain_own_batch_s (last repeat)": round(spent["library"], 3)}))


if __name__ == "__main__":
    main()

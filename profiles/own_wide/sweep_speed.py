"""What the own-nodes run forms of the all-feature kernel buy the sweeps of an Open-Local cluster, on one box:

  mix   simulate.sweep_mix over an 8 x 8 grid of the two node types of the reference's Open-Local example (tests/mix_util.py), on
        HipEngine(own_nodes_all_feature=True) -- one segmented batch -- and on HipEngine() -- the refusal, then one simulate() per mix
        (the road of the commit before; the default engine runs that commit's code, its kernels are unchanged);
  n1    the N-1 question at array level on a random Open-Local problem (tests/randprob.py, local=True) of ~300 nodes: the whole pool
        and the pool without each node, as ONE node-subset batch against one context + load + run per scenario on that scenario's own
        (restricted) problem, which is what the sweeps' fallback does after flattening.

    python profiles/own_wide/sweep_speed.py [n_nodes] [n_pods] [repeats]

Prints one JSON line: wall seconds (best of `repeats`) and the engine's kernel milliseconds (simon_get_stats) of both roads.
The script uses only what both commits share: a copy of it (with tests/ of that commit) in a checkout of the commit before, whose
engine has no opt-in, times that commit's road alone -- one run per scenario -- for the A/B on the same box."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mix_util as MU  # noqa: E402
import randprob  # noqa: E402
from open_simulator_amd import capi, simulate as sim  # noqa: E402


OPT_IN = hasattr(sim.HipEngine, "supports_own_nodes_all_feature")      # (the commit before: no such engine, the fallback road only)


def engine(opt_in):
    return Timed(own_nodes_all_feature=True) if opt_in else Timed()


class Timed(sim.HipEngine):
    kernel_ms = 0.0
    runs = 0

    def run(self, *a, **kw):
        out = super().run(*a, **kw)
        self.kernel_ms += self.last_stats.kernel_ms
        self.runs += 1
        return out


def best(fn, repeats):
    rows = [fn() for _ in range(repeats)]
    return min(rows, key=lambda r: r[0])


def mix(repeats):
    cluster, apps, types = MU.example_open_local()
    grid = [range(0, 8), range(0, 8)]

    def road(opt_in):
        eng = engine(opt_in)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", sim.MixFallbackWarning)
            sw = sim.sweep_mix(cluster, apps, types, grid, engine=eng)
        wall = time.perf_counter() - t0
        assert sw.batched == opt_in
        return wall, eng.kernel_ms, eng.runs, (sw.unscheduled, sw.best, sw.vg_pct)
    b = best(lambda: road(False), repeats)
    if not OPT_IN:
        return {"mixes": 64, "per_mix_wall_s": round(b[0], 3), "per_mix_kernel_ms": round(b[1], 3), "per_mix_engine_runs": b[2]}
    a = best(lambda: road(True), repeats)
    assert a[3] == b[3], "the two roads disagree"
    return {"mixes": 64, "batched_wall_s": round(a[0], 3), "batched_kernel_ms": round(a[1], 3), "batched_engine_runs": a[2],
            "per_mix_wall_s": round(b[0], 3), "per_mix_kernel_ms": round(b[1], 3), "per_mix_engine_runs": b[2]}


def n1(N, P, repeats):
    prob, _ = MU.segmentable(randprob.rand_problem(5, N=N, P=P, local=True, n_node_classes=9, n_pod_classes=12), fixed=0)
    mask = np.ones((N + 1, N), bool)
    mask[np.arange(1, N + 1), np.arange(N)] = False
    scen = np.stack([mask.sum(1), np.zeros(N + 1, np.int64)], 1).astype(np.int32)
    orders = np.arange(P, dtype=np.int32)[None]

    def batched():
        eng = engine(True)
        t0 = time.perf_counter()
        out = eng.run(prob, scen, orders, present=(mask, None))
        return time.perf_counter() - t0, eng.kernel_ms, eng.runs, out.unscheduled.tolist(), out.used_vg.tolist()

    subs = [MU.restrict_nodes(prob, np.flatnonzero(mask[s]))[0] for s in range(N + 1)]      # (outside the clock: flattening is not timed either)

    def one_by_one():
        eng = Timed()
        t0 = time.perf_counter()
        outs = [eng.run(subs[s], scen[s:s + 1], orders) for s in range(N + 1)]
        return time.perf_counter() - t0, eng.kernel_ms, eng.runs, [int(o.unscheduled[0]) for o in outs], [int(o.used_vg[0]) for o in outs]
    b = best(one_by_one, repeats)
    if not OPT_IN:
        return {"nodes": N, "pods": P, "scenarios": N + 1, "one_by_one_wall_s": round(b[0], 3), "one_by_one_kernel_ms": round(b[1], 3),
                "one_by_one_engine_runs": b[2]}
    a = best(batched, repeats)
    assert a[3:] == b[3:], "the two roads disagree"
    return {"nodes": N, "pods": P, "scenarios": N + 1, "scenarios_with_unscheduled_pods": sum(u > 0 for u in a[3]),
            "batched_wall_s": round(a[0], 3), "batched_kernel_ms": round(a[1], 3), "one_by_one_wall_s": round(b[0], 3),
            "one_by_one_kernel_ms": round(b[1], 3), "one_by_one_engine_runs": b[2]}


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    print(json.dumps({"engine_has_the_opt_in": OPT_IN, "sweep_mix_8x8_open_local": mix(repeats), "n_minus_1_open_local": n1(N, P, repeats)}))


if __name__ == "__main__":
    main()

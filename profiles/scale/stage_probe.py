#!/usr/bin/env python3
"""Staging cost of a replica-scaling grid: explicit order and pod rows against rows composed on the device.

A config-3-like synthetic problem (synth.build_problem: 10 000 pods, 1 000 nodes) whose stream is cut into the cluster's pods and two
apps; each app has one target at 64 levels, every level with an order of its own (a seeded shuffle of the level's pods, the absent pods
appended), so the grid is 4 096 combos = 4 096 distinct orders, one scenario each (counts (0,)).  Timed, host clock around calls that end
in a device synchronise, median of --reps repetitions after one warm-up, the two roads alternating:
  (a) OrderSegments.compose() in numpy + simon_load_scenarios + simon_set_scenario_pods   -- the road without the composed call
  (b) simon_load_scenarios_composed
  (c) simon_run_loaded after either load (the kernel must not care where the rows came from; the results are compared)

  python profiles/scale/stage_probe.py [--pods 10000] [--levels 64] [--reps 5] [--out FILE.json]
Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from open_simulator_amd import capi, synth  # noqa: E402


def grid(P, levels, seed=1):
    """capi.OrderSegments of the grid: segment 0 = the first fifth of the stream, then two apps of equal size."""
    rng = np.random.default_rng(seed)
    n0 = P // 5
    n1 = (P - n0) // 2
    seg_start = np.array([0, n0, n0 + n1, P], np.int32)
    variants, live = [np.arange(n0, dtype=np.int32)[None, :]], [np.array([n0], np.int32)]
    for g in (1, 2):
        lo, hi = int(seg_start[g]), int(seg_start[g + 1])
        rows, lives = [], []
        for v in range(levels):
            r = (hi - lo) * (v + 1) // levels
            rows.append(np.concatenate([lo + rng.permutation(r), np.arange(lo + r, hi)]).astype(np.int32))
            lives.append(r)
        variants.append(np.stack(rows))
        live.append(np.array(lives, np.int32))
    a, b = np.meshgrid(np.arange(levels), np.arange(levels), indexing="ij")
    choice = np.stack([np.zeros(levels * levels, np.int64), a.reshape(-1), b.reshape(-1)], 1).astype(np.int32)
    return capi.OrderSegments(seg_start, variants, live, choice)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=10000)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prob = synth.build_problem(1, args.pods, args.nodes // 2, args.nodes)
    segs = grid(args.pods, args.levels)
    S = segs.n_orders
    scen = np.stack([np.full(S, args.nodes), np.arange(S)], 1).astype(np.int32)
    t = {"compose_numpy": [], "load_scenarios": [], "set_scenario_pods": [], "explicit_total": [], "composed": [], "run_after_explicit": [],
         "run_after_composed": []}
    results = {}
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        for rep in range(args.reps + 1):                               # (repetition 0 warms both roads up)
            t0 = time.perf_counter()
            orders, present = segs.compose()
            t1 = time.perf_counter()
            ctx.load_scenarios(scen, orders)
            t2 = time.perf_counter()
            ctx.set_scenario_pods(present)                             # (S = n_orders here: row s is order s's)
            t3 = time.perf_counter()
            ctx.run_loaded(False)
            t4 = time.perf_counter()
            results["explicit"] = ctx.fetch(True)
            t5 = time.perf_counter()
            ctx.load_scenarios_composed(scen, segs)
            t6 = time.perf_counter()
            ctx.run_loaded(False)
            t7 = time.perf_counter()
            results["composed"] = ctx.fetch(True)
            if rep:
                for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t3 - t0, t6 - t5, t4 - t3, t7 - t6)):
                    t[k].append(v * 1e3)
        stats = ctx.stats()
    a, b = results["explicit"], results["composed"]
    same = bool((a.placement == b.placement).all() and (a.unscheduled == b.unscheduled).all() and (a.used_cpu == b.used_cpu).all())
    table_bytes = int(sum(v.nbytes for v in segs.variants) * 2 + segs.choice.nbytes)
    out = {"pods": args.pods, "nodes": args.nodes, "levels": args.levels, "orders": S, "reps": args.reps,
           "explicit_upload_bytes": int(2 * orders.nbytes + S * ((args.pods + 31) // 32) * 4), "composed_upload_bytes": table_bytes,
           "kernel_variant": int(stats.kernel_variant), "kernel_generation": int(stats.kernel_generation), "results_equal": same,
           "median_ms": {k: round(statistics.median(v), 3) for k, v in t.items()}, "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

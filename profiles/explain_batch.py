#!/usr/bin/env python3
"""Why-does-it-not-fit for every failing size of a sweep: ONE simon_explain_batch against the loop of simon_explain_loaded.

  python profiles/explain_batch.py [--out FILE.json] [--single N | --single-batch N]

Two workloads, interleaved in one process on one context each: synth.typical_cluster_sweep reduced to what replays within a minute,
and a sweep of config-2-sized scenarios (1 000 pods, 16 .. 63 nodes).  Per workload, after a warm-up of both, best of three of
  (a) one explain_batch over all failing scenarios (bins only: what sweep(..., reasons=True) asks for first), and
  (b) explain_loaded for the same scenarios one after the other (full code rows, binned on the host by np.unique),
by wall clock around the calls -- the replays record no events of their own, and the copies back are part of what a host waits for;
the kernels' own time is read from a `rocprofv3 --kernel-trace --stats` run of this script.
Both must name the same failed pods and the same histograms.  --single N: only single replays (explain_loaded: no histogram) of the
first failing scenario, four passes of N (a warm-up and three samples; call_ms = the best pass's wall clock per call, the figure that
shows a change of the host path), the run such a trace wraps to read the EXPLAIN kernel's time; --single-batch N: the same scenario N times through
explain_batch([s]), one workgroup with the histogram -- the difference between the two is the histogram's cost."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_simulator_amd import capi, synth  # noqa: E402

MAX_FAILED = 64


def workloads():
    prob, scen, orders = synth.typical_cluster_sweep(n_nodes=40, new_nodes=200, n_workloads=60, max_replicas=120, n_counts=48)
    yield "typical_cluster_sweep(40 + 0..200 nodes)", prob, scen, orders
    prob, _, orders = synth.config2()
    yield "config2 pods on 16 .. 63 nodes", prob, np.array([[n, 0] for n in range(16, 64)], np.int32), orders


def binned(codes):
    return [tuple(map(tuple, np.stack(np.unique(row, return_counts=True), 1).tolist())) for row in codes]


def measure(name, prob, scen, orders):
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders, want_placement=False)
        failing = [s for s in range(len(scen)) if res.unscheduled[s] > 0]
        rec = {"workload": name, "pods": int(prob.n_pods), "pool_nodes": int(prob.n_nodes), "scenarios": len(scen), "failing": len(failing),
               "unscheduled_max": int(res.unscheduled.max())}
        if not failing:
            return rec

        def batch():
            return ctx.explain_batch(failing, MAX_FAILED, 32)

        def loop():
            return [ctx.explain_loaded(s, MAX_FAILED) for s in failing]

        eb, singles = batch(), loop()                                   # warm-up; and the two must agree
        for k, (nf, failed, codes) in enumerate(singles):
            assert nf == eb.n_failed[k] and failed.tolist() == eb.failed_pods[k, :len(failed)].tolist(), (name, k)
            assert [tuple(eb.pod_bins(k, i)) for i in range(len(failed))] == binned(codes), (name, k)
        ta, tb = [], []
        for _ in range(3):
            t0 = time.perf_counter(); batch(); t1 = time.perf_counter(); loop(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        rec.update(batch_ms=round(min(ta) * 1e3, 2), loop_ms=round(min(tb) * 1e3, 2), speedup=round(min(tb) / min(ta), 2),
                   batch_ms_all=[round(t * 1e3, 2) for t in ta], loop_ms_all=[round(t * 1e3, 2) for t in tb])
        return rec


def single(n, batch):
    name, prob, scen, orders = next(workloads())
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders, want_placement=False)
        s = int(np.argmax(res.unscheduled > 0))
        per_call = []
        for _ in range(4):                                              # a warm-up pass and three samples of n replays each
            t0 = time.perf_counter()
            for _ in range(n):
                nf = int(ctx.explain_batch([s], MAX_FAILED, 32).n_failed[0]) if batch else ctx.explain_loaded(s, MAX_FAILED)[0]
            per_call.append((time.perf_counter() - t0) / n)
    print(json.dumps({"workload": name, "scenario": s, "n_nodes": int(scen[s, 0]), "unscheduled": int(nf), "replays": n,
                      "call": "explain_batch" if batch else "explain_loaded", "call_ms": round(min(per_call[1:]) * 1e3, 3),
                      "call_ms_all": [round(t * 1e3, 3) for t in per_call[1:]]}))


if __name__ == "__main__":
    for flag in ("--single", "--single-batch"):
        if flag in sys.argv:
            single(int(sys.argv[sys.argv.index(flag) + 1]), flag == "--single-batch")
            sys.exit(0)
    out = [measure(*w) for w in workloads()]
    for r in out:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f, indent=1)

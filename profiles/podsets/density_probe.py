#!/usr/bin/env python3
"""What an absent pod costs: config 3's problem (4 096 scenarios, profiles/ab_probe.py's `c3`) with pod rows at presence densities 1.0, 0.5
and 0.1, against the same batch without rows (no gather in load_chunk).  Kernel time (HIP events), best of `reps`.
usage: python profiles/podsets/density_probe.py [reps=5]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
from open_simulator_amd import capi, synth              # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    prob, scen, orders = synth.config3(n_counts=1024, n_orders=4, n_pods=10000, seed=synth.SEED + 3)
    S, P = len(scen), prob.n_pods
    rng = np.random.default_rng(1)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        for density in (None, 1.0, 0.5, 0.1):
            if density is None:
                ctx.set_scenario_pods(None)
                present = S * P
            else:
                rows = rng.random((S, P)) < density
                ctx.set_scenario_pods(rows)
                present = int(rows.sum())
            ts = []
            for _ in range(reps + 1):
                ctx.run_loaded(True)
                ts.append(ctx.stats().kernel_ms)
            best = min(ts[1:])
            absent = S * P - present
            print(f"DENSITY {'no rows' if density is None else density}: S={S} P={P} best_ms={best:.3f} mean_ms={np.mean(ts[1:]):.3f} present={present} absent={absent} "
                  f"ns_per_step={best * 1e6 / (S * P):.3f} unsched_sum={int(ctx.fetch(False).unscheduled.sum())}", flush=True)
        # simon_fetch_group_counts against fetching the placement matrix (both after the last run)
        group = (np.arange(P) % 12).astype(np.int32)
        import time
        for _ in range(2):
            t0 = time.perf_counter(); ctx.fetch_group_counts(group, 12); t_g = time.perf_counter() - t0
            t0 = time.perf_counter(); ctx.fetch(True); t_p = time.perf_counter() - t0
            ms_p = ctx.stats().d2h_ms
        print(f"GROUPS S={S} P={P} G=12: fetch_group_counts {t_g * 1e3:.2f} ms wall (H2D of pod_group, kernel, {S * 12 * 4} B D2H); "
              f"placement matrix {t_p * 1e3:.2f} ms wall, {ms_p:.3f} ms of it D2H on the stream ({S * P * 4} B)", flush=True)


if __name__ == "__main__":
    main()

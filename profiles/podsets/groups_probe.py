#!/usr/bin/env python3
"""simon_fetch_group_counts against fetching the placement matrix at config 3's shape (S = 4 096, P = 10 000, G = 12): wall time of each
call, five times each after one run.  Under `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python ...` the trace splits the calls
into kernel time (group_counts_kernel) and copy time.
usage: python profiles/podsets/groups_probe.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                      # noqa: E402
from open_simulator_amd import capi, synth              # noqa: E402

prob, scen, orders = synth.config3(n_counts=1024, n_orders=4, n_pods=10000, seed=synth.SEED + 3)
S, P, G = len(scen), prob.n_pods, 12
group = (np.arange(P) % G).astype(np.int32)
with capi.Context(0) as ctx:
    ctx.load_problem(prob)
    ctx.load_scenarios(scen, orders)
    ctx.run_loaded(True)
    tg, tp, d2h = [], [], []
    for _ in range(5):
        t0 = time.perf_counter(); ctx.fetch_group_counts(group, G, placed=True); tg.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); ctx.fetch(True); tp.append(time.perf_counter() - t0)
        d2h.append(ctx.stats().d2h_ms)
print(f"GROUPS S={S} P={P} G={G}: fetch_group_counts best {min(tg) * 1e3:.3f} ms wall ({2 * S * G * 4} B back); placement fetch best {min(tp) * 1e3:.3f} ms wall, "
      f"{min(d2h):.3f} ms of it D2H on the stream ({S * P * 4} B back)", flush=True)

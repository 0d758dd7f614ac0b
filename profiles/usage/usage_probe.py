#!/usr/bin/env python3
"""simon_fetch_headroom (K = 8 probes) and simon_fetch_node_usage (64 scenarios) against the only road the parent has -- fetching the
placement matrix and reducing it with numpy on the host (simulate.host_headroom / host_node_usage) -- at config 3's shape (S = 4 096,
P = 10 000, N = 1 512) or config 5's (S = 256, P = 50 000, N = 5 000).  Wall time of each call, best of five after one run; the device
figures are compared with the host's (they must be equal).  --tiles: the same calls with SIMON_USAGE_TILE set to each value (a context
per value: the knob is read when the context is made).  Under `rocprofv3 --kernel-trace --stats -- python ...` the trace gives the
kernel time of node_usage_kernel / headroom_kernel.
usage: python profiles/usage/usage_probe.py --config 3|5 [--tiles 256,512,...] [--no-host]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                                  # noqa: E402
from open_simulator_amd import capi, simulate as sim, synth          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, choices=[3, 5], default=3)
ap.add_argument("--tiles", default="")
ap.add_argument("--no-host", action="store_true", help="skip the host reduction (the traced run: only the device calls)")
args = ap.parse_args()

if args.config == 3:
    prob, scen, orders = synth.config3(n_counts=1024, n_orders=4, n_pods=10000, seed=synth.SEED + 3)
else:
    prob, scen, orders = synth.config5()
prob.normalise()
S, P, N, K = len(scen), prob.n_pods, prob.n_nodes, 8
rng = np.random.default_rng(5)
plain = np.flatnonzero((np.asarray(prob.preset_node) < 0) if prob.preset_node is not None else np.ones(P, bool))
probes = rng.choice(plain, K, replace=False).astype(np.int32)
ids = np.sort(rng.choice(S, min(64, S), replace=False)).astype(np.int32)
held = np.arange(N)[None, :] < scen[:, :1]
best = lambda f, n=5: min(_timed(f) for _ in range(n))                 # noqa: E731


def _timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def one(tile):
    if tile:
        os.environ["SIMON_USAGE_TILE"] = str(tile)
    else:
        os.environ.pop("SIMON_USAGE_TILE", None)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True)
        st = ctx.stats()
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True)     # (first call: stages the compact copies)
        usage = ctx.fetch_node_usage(ids)
        t_h = best(lambda: ctx.fetch_headroom(probes, nodes=True))
        t_u = best(lambda: ctx.fetch_node_usage(ids))
        t_p = best(lambda: ctx.fetch(True), 3)
        res = ctx.fetch(True) if not args.no_host and not tile else None
    print(f"USAGE config {args.config} S={S} P={P} N={N} tile={tile or 'default'} (run: kernel variant {st.kernel_variant}, {st.kernel_ms:.1f} ms): "
          f"fetch_headroom K={K} best {t_h:.3f} ms wall ({S * K * 12} B back); fetch_node_usage of {len(ids)} scenarios best {t_u:.3f} ms wall "
          f"({len(ids) * N * 20} B back); placement fetch best {t_p:.3f} ms wall ({S * P * 4} B back)", flush=True)
    return res, fit, nodes, exact, usage


res, fit, nodes, exact, usage = one(0)
if res is not None:
    t0 = time.perf_counter()
    hf, hn, hx = sim.host_headroom(prob, res.placement, held, probes)
    t_hh = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hu = sim.host_node_usage(prob, res.placement, held, ids)
    t_hu = (time.perf_counter() - t0) * 1e3
    same = (fit.tolist() == hf.tolist() and nodes.tolist() == hn.tolist() and exact.tolist() == hx.tolist() and usage.req_cpu.tolist() == hu.req_cpu.tolist()
            and usage.req_mem.tolist() == hu.req_mem.tolist() and usage.npods.tolist() == hu.npods.tolist())
    print(f"HOST config {args.config}: numpy headroom over the fetched matrix {t_hh:.1f} ms, numpy node usage of {len(ids)} scenarios {t_hu:.1f} ms; "
          f"device == host: {same}; exact {exact.astype(int).tolist()}; fit of scenario 0 {fit[0].tolist()}, of scenario {S - 1} {fit[-1].tolist()}", flush=True)
    assert same
for t in [int(x) for x in args.tiles.split(",") if x]:
    _, f2, n2, _, u2 = one(t)
    assert f2.tolist() == fit.tolist() and n2.tolist() == nodes.tolist() and u2.npods.tolist() == usage.npods.tolist(), t

#!/usr/bin/env python3
"""simon_fetch_gpu_usage (all scenarios) and simon_fetch_headroom_gpu (K = 8 GPU probes) against the only road the parent has --
fetching the placement matrix and gpu_slices and reducing them with numpy on the host (simulate.host_gpu_usage / host_headroom with
devices=True) -- at config 5's shape (synth.config5: S = 256, P = 50 000, N = 5 000, devices recorded).  Wall time of each call, best of
five after one run; the device figures are compared with the host's (they must be equal).  The numpy reduction runs over the first
--host-scenarios scenarios (its cost is linear in the scenarios; the line says how many).  Under `rocprofv3 --kernel-trace --stats --
python ... --no-host --only usage|headroom|fetch` the trace gives the kernel time of gpu_usage_kernel / headroom_kernel<true, false> / the
copies of the parent's road, each in a run of its own.
usage: python profiles/gpu_usage/gpu_usage_probe.py [--no-host] [--only usage|headroom|fetch] [--host-scenarios 32] [--tiles 256,512]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                                  # noqa: E402
from open_simulator_amd import capi, simulate as sim, synth          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--no-host", action="store_true", help="skip the host reduction (the traced run: only the device calls)")
ap.add_argument("--host-scenarios", type=int, default=32)
ap.add_argument("--tiles", default="")
ap.add_argument("--only", choices=["usage", "headroom", "fetch"], help="time one of the three roads alone (one traced run each)")
args = ap.parse_args()

prob, scen, orders = synth.config5()
prob.normalise()
S, P, N, K = len(scen), prob.n_pods, prob.n_nodes, 8
gm, gc = np.asarray(prob.gpu_mem), np.asarray(prob.pod_gpu_cnt)
probes, seen = [], {}
for p in np.flatnonzero(gm > 0).tolist():                              # two pods (of different classes) per (memory, count) shape
    key = (int(gm[p]), int(gc[p]))
    if len(seen.setdefault(key, set())) < 2 and int(prob.pod_class[p]) not in seen[key]:
        seen[key].add(int(prob.pod_class[p]))
        probes.append(p)
probes = np.array(probes[:K], np.int32)
held = np.arange(N)[None, :] < scen[:, :1]


def _timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


best = lambda f, n=5: min(_timed(f) for _ in range(n))                 # noqa: E731


def one(tile):
    if tile:
        os.environ["SIMON_USAGE_TILE"] = str(tile)
    else:
        os.environ.pop("SIMON_USAGE_TILE", None)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True, True)
        st = ctx.stats()
        g = ctx.fetch_gpu_usage(pods=True)                             # (first call: stages the compact copies)
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, devices=True)
        old, _, _ = ctx.fetch_headroom(probes)
        on = lambda what: args.only in (None, what)                     # noqa: E731
        t_g = best(lambda: ctx.fetch_gpu_usage()) if on("usage") else 0
        t_gp = best(lambda: ctx.fetch_gpu_usage(pods=True)) if on("usage") else 0
        t_g64 = best(lambda: ctx.fetch_gpu_usage(np.arange(64, dtype=np.int32))) if on("usage") else 0
        t_h = best(lambda: ctx.fetch_headroom(probes, nodes=True, devices=True)) if on("headroom") else 0
        t_o = best(lambda: ctx.fetch_headroom(probes, nodes=True)) if on("headroom") else 0
        t_p = best(lambda: ctx.fetch(True, True), 3) if on("fetch") else 0
        res = ctx.fetch(True, True) if not args.no_host and not tile else None
    print(f"GPU_USAGE config 5 S={S} P={P} N={N} tile={tile or 'default'} (run: kernel variant {st.kernel_variant}, {st.kernel_ms:.1f} ms): "
          f"fetch_gpu_usage of all {S} scenarios best {t_g:.3f} ms wall ({S * N * 64} B back), with dev_pods {t_gp:.3f} ms ({S * N * 96} B), "
          f"of 64 scenarios {t_g64:.3f} ms; fetch_headroom(devices) K={len(probes)} best {t_h:.3f} ms wall ({S * len(probes) * 12} B back), "
          f"simon_fetch_headroom on the same probes {t_o:.3f} ms; placement + gpu_slices fetch best {t_p:.3f} ms wall ({S * P * 12} B back)", flush=True)
    return res, g, fit, nodes, exact, old


res, g, fit, nodes, exact, old = one(0)
print(f"FIGURES exact {exact.astype(int).tolist()}; device-bounded fit of scenario 0 {fit[0].tolist()} (resource bound {old[0].tolist()}), "
      f"of scenario {S - 1} {fit[-1].tolist()} ({old[-1].tolist()}); busiest device {int(g.dev_used.max())} B, most pods on one device {int(g.dev_pods.max())}", flush=True)
if res is not None:
    n = min(args.host_scenarios, S)
    t0 = time.perf_counter()
    hg = sim.host_gpu_usage(prob, res.placement[:n], res.gpu_slices[:n], held[:n])
    t_hg = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hf, hn, hx = sim.host_headroom(prob, res.placement[:n], held[:n], probes, res.gpu_slices[:n], devices=True)
    t_hh = (time.perf_counter() - t0) * 1e3
    same = (np.array_equal(g.dev_used[:n], hg.dev_used) and np.array_equal(g.dev_pods[:n], hg.dev_pods) and np.array_equal(fit[:n], hf)
            and np.array_equal(nodes[:n], hn) and exact.tolist() == hx.tolist())
    print(f"HOST config 5, first {n} of {S} scenarios: numpy device usage {t_hg:.1f} ms, numpy headroom with the device bound {t_hh:.1f} ms "
          f"(x {S / n:.0f} for all scenarios: {t_hg * S / n:.0f} ms, {t_hh * S / n:.0f} ms); device == host: {same}", flush=True)
    assert same
for t in [int(x) for x in args.tiles.split(",") if x]:
    _, g2, f2, n2, _, _ = one(t)
    assert np.array_equal(g2.dev_used, g.dev_used) and np.array_equal(f2, fit) and np.array_equal(n2, nodes), t

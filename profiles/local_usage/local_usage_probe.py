#!/usr/bin/env python3
"""simon_fetch_local_usage and simon_fetch_headroom_local (K = 8 probes) against the only road the parent has -- fetching the placement
matrix and replaying it on the host (simulate.host_local_usage / host_headroom(storage=True)) -- on an Open-Local cluster of config 5's
size: config 5's node pool (synth.gen_nodes, N = 5 000) with 75 % of the nodes annotated (two volume groups, four exclusive devices),
config 5's pod shapes (synth.gen_pods, P = 50 000) of which 10 % ask for local volumes in five specs (named VG, any VG, SSD, HDD, mixed),
S = 64 and 256 prefix scenarios over four orders.  Wall time of each call, best of five after one run; the device figures are compared
with the host's over the first --host-scenarios scenarios (they must be equal; the host replay is a Python loop, linear in the
scenarios).  Under `rocprofv3 --kernel-trace --stats -- python ... --no-host --only usage|headroom|fetch --scenarios 256` the trace
gives the kernel time of local_usage_kernel / headroom_kernel<false, true> / the copy of the parent's road, each in a run of its own.
usage: python profiles/local_usage/local_usage_probe.py [--no-host] [--only usage|headroom|fetch] [--host-scenarios 4] [--scenarios 64,256] [--tiles 512]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                                  # noqa: E402
from open_simulator_amd import capi, simulate as sim, synth          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--no-host", action="store_true", help="skip the host replay (the traced run: only the device calls)")
ap.add_argument("--host-scenarios", type=int, default=4)
ap.add_argument("--scenarios", default="64,256")
ap.add_argument("--tiles", default="")
ap.add_argument("--pods", type=int, default=50000)
ap.add_argument("--nodes", type=int, default=5000)
ap.add_argument("--only", choices=["usage", "headroom", "fetch"], help="time one of the three roads alone (one traced run each)")
args = ap.parse_args()

GiB = 1 << 30
N, P, K = args.nodes, args.pods, 8
seed = synth.SEED + 5
rng = np.random.default_rng(5)
cpu, mem, pods, ncls = synth.gen_nodes(seed, N, N)
pcpu, pmem = synth.gen_pods(seed, P)
specs = np.zeros(5, capi.LOCAL_SPEC_DTYPE)
for i, lvm in enumerate(([(20, 0)], [(10, -1), (5, -1)], [], [], [(8, 1), (4, -1)])):
    specs[i]["n_lvm"], specs[i]["lvm_vg"][:] = len(lvm), -1
    for k, (size, vg) in enumerate(lvm):
        specs[i]["lvm_size"][k], specs[i]["lvm_vg"][k] = size * GiB, vg
specs[2]["n_ssd"], specs[2]["ssd_size"][0] = 1, 100 * GiB
specs[3]["n_hdd"], specs[3]["hdd_size"][:2] = 2, (200 * GiB, 400 * GiB)
specs[4]["n_ssd"], specs[4]["ssd_size"][0] = 1, 50 * GiB
spec_of_pod = np.where(rng.random(P) < 0.10, rng.integers(0, 5, P), -1)
ids, table, pcls = {}, [], np.empty(P, np.int32)
for p, key in enumerate(zip(pcpu.tolist(), pmem.tolist(), spec_of_pod.tolist())):
    pcls[p] = ids.setdefault(key, len(ids))
    if pcls[p] == len(table):
        table.append(key)
Cp = len(table)
flags = (rng.random(N) < 0.75).astype(np.int32)
prob = capi.Problem(alloc_cpu=cpu, alloc_mem=mem, alloc_pods=pods, node_class=ncls, req_cpu=pcpu, req_mem=pmem, pod_class=pcls,
                    n_pod_classes=Cp, n_node_classes=4, simon_raw=synth.simon_raw_table([(t[0], t[1]) for t in table]),
                    const_score=np.full(Cp, synth.CONST_SCORE, np.int64),
                    local_flags=flags, local_vg_cnt=np.where(flags > 0, 2, 0).astype(np.int32),
                    local_vg_cap=np.tile(np.array([200, 400, 1, 1], np.int64) * GiB, (N, 1)), local_vg_name=np.tile(np.array([0, 1, -1, -1], np.int32), (N, 1)),
                    init_vg_req=(rng.choice([0, 0, 10, 40], (N, 4)) * GiB * np.array([1, 1, 0, 0])).astype(np.int64),
                    local_dev_cnt=np.where(flags > 0, 4, 0).astype(np.int32),
                    local_dev_cap=np.tile(np.array([100, 200, 400, 800, 1, 1, 1, 1], np.int64) * GiB, (N, 1)),
                    local_dev_media=np.full(N, 1 | (1 << 2) | (2 << 4) | (2 << 6), np.int32),
                    init_dev_alloc=(rng.random(N) < 0.1).astype(np.int32),
                    local_specs=specs, local_spec_of=np.array([t[2] for t in table], np.int32)).normalise()
orders = synth.make_orders(seed, pcpu, pmem, int(cpu.sum()), int(mem.sum()), 4)
probes, seen = [], set()
for p in np.flatnonzero(spec_of_pod >= 0).tolist():                    # one pod per spec, then a second class of the first three
    if (int(spec_of_pod[p]), len([q for q in probes if spec_of_pod[q] == spec_of_pod[p]])) in {(s, 0) for s in range(5)} | {(s, 1) for s in range(3)} \
            and int(pcls[p]) not in seen:
        seen.add(int(pcls[p]))
        probes.append(p)
    if len(probes) == K:
        break
probes = np.array(probes, np.int32)


def _timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


best = lambda f, n=5: min(_timed(f) for _ in range(n))                 # noqa: E731


def one(S, tile):
    if tile:
        os.environ["SIMON_USAGE_TILE"] = str(tile)
    else:
        os.environ.pop("SIMON_USAGE_TILE", None)
    counts = np.linspace(N // 2, N, max(1, S // 4)).astype(np.int32)
    scen = np.ascontiguousarray(np.stack([np.repeat(counts, 4), np.tile(np.arange(4, dtype=np.int32), len(counts))], 1)[:S], np.int32)
    held = np.arange(N)[None, :] < scen[:, :1]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True, False)
        st = ctx.stats()
        t_first = _timed(lambda: ctx.fetch_local_usage())               # (first call: builds and stages the compact copies and the lists)
        use = ctx.fetch_local_usage()
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, storage=True)
        old, _, _ = ctx.fetch_headroom(probes)
        on = lambda what: args.only in (None, what)                     # noqa: E731
        t_u = best(lambda: ctx.fetch_local_usage()) if on("usage") else 0
        t_h = best(lambda: ctx.fetch_headroom(probes, nodes=True, storage=True)) if on("headroom") else 0
        t_o = best(lambda: ctx.fetch_headroom(probes, nodes=True)) if on("headroom") else 0
        t_p = best(lambda: ctx.fetch(True), 3) if on("fetch") else 0
        res = ctx.fetch(True) if not args.no_host and not tile else None
    n_storage = int((spec_of_pod >= 0).sum())
    print(f"LOCAL_USAGE S={len(scen)} P={P} N={N} storage pods {n_storage} tile={tile or 'default'} (run: kernel variant {st.kernel_variant}, {st.kernel_ms:.1f} ms): "
          f"fetch_local_usage of all scenarios best {t_u:.3f} ms wall ({len(scen) * N * 36} B back; first call with staging {t_first:.3f} ms); "
          f"fetch_headroom(storage) K={len(probes)} best {t_h:.3f} ms wall, simon_fetch_headroom on the same probes {t_o:.3f} ms; "
          f"placement fetch best {t_p:.3f} ms wall ({len(scen) * P * 4} B back)", flush=True)
    print(f"FIGURES S={len(scen)} exact {exact.astype(int).tolist()}; storage-bounded fit of scenario 0 {fit[0].tolist()} (resource bound {old[0].tolist()}), "
          f"of the last {fit[-1].tolist()} ({old[-1].tolist()}); fullest volume group {int(use.vg_req.max()) // GiB} GiB, devices in use {int(sum(bin(int(x)).count('1') for x in use.dev_alloc[-1] if x > 0))}", flush=True)
    if res is not None:
        n = min(args.host_scenarios, len(scen))
        t0 = time.perf_counter()
        hu = sim.host_local_usage(prob, res.placement, held, orders, scen, np.arange(n))
        t_hu = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        hf, hn, hx = sim.host_headroom(prob, res.placement[:n], held[:n], probes, storage=True, orders=orders, scen=scen[:n])
        t_hh = (time.perf_counter() - t0) * 1e3
        same = (np.array_equal(use.vg_req[:n], hu.vg_req) and np.array_equal(use.dev_alloc[:n], hu.dev_alloc) and np.array_equal(fit[:n], hf)
                and np.array_equal(nodes[:n], hn) and exact.tolist() == hx.tolist())
        print(f"HOST first {n} of {len(scen)} scenarios: host replay {t_hu:.1f} ms, host headroom with the storage bound {t_hh:.1f} ms "
              f"(x {len(scen) / n:.0f} for all scenarios: {t_hu * len(scen) / n:.0f} ms, {t_hh * len(scen) / n:.0f} ms); device == host: {same}", flush=True)
        assert same
    return use, fit, nodes


for S in [int(x) for x in args.scenarios.split(",") if x]:
    use, fit, nodes = one(S, 0)
    for t in [int(x) for x in args.tiles.split(",") if x]:
        u2, f2, n2 = one(S, t)
        assert np.array_equal(u2.vg_req, use.vg_req) and np.array_equal(u2.dev_alloc, use.dev_alloc) and np.array_equal(f2, fit) and np.array_equal(n2, nodes), t

"""Pod-subset batches, the host side (no GPU): sweep_apps against simulate() of every scenario on the CPU oracle -- which pins the
"a subset's stream is the full stream restricted to its pods" argument -- its fallbacks and their warnings; the rules of
simon_set_scenario_pods and simon_fetch_group_counts restated and checked on hand cases; word packing; the ctypes prototypes against the
header; the yardstick's own helpers."""
import copy
import itertools
import os
import re
import warnings

import numpy as np
import pytest

import mix_util as MU
import podset_util as PU
import randprob
import subset_util as SU
from open_simulator_amd import capi, simulate as sim, workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split(apps, daemonsets=False):
    """One app per workload object of the given apps (DaemonSets left out unless asked for)."""
    out = []
    for app in apps:
        for kind, objs in app.resource.items():
            if kind == "DaemonSet" and not daemonsets:
                continue
            if kind in ("StorageClass", "Service", "ConfigMap", "PersistentVolumeClaim"):
                continue
            for o in objs:
                out.append(sim.AppResource(f"{kind.lower()}-{o['metadata']['name']}", {kind: [o]}))
    return out


def _shrunk(cluster, keep):
    """The cluster with its first `keep` nodes only: a cluster small enough that not every combination of the apps fits."""
    nodes = list(cluster["Node"])[:keep]
    names = {n["metadata"]["name"] for n in nodes}
    pods = [p for p in cluster.get("Pod", []) if not (p.get("spec") or {}).get("nodeName") or p["spec"]["nodeName"] in names]
    return dict(cluster, Node=nodes, Pod=pods)


def _by_hand(cluster, apps, subs, tmpl, counts, caps=(100, 100, 100)):
    """simulate() of every (subset, count) on the oracle: [u][k] -> (where by pod name, [(pod ref, reason)] of the unscheduled pods)."""
    out = []
    for sub in subs:
        out.append([])
        for k in counts:
            new = wl.new_fake_nodes(tmpl, k) if k else []
            if not sim.build_stream(cluster, [apps[a] for a in sub], list(cluster["Node"]) + new, len(cluster["Node"]) + k)[0]:
                out[-1].append(({}, []))                               # (no pod at all: nothing to simulate)
                continue
            res = sim.simulate(cluster, [apps[a] for a in sub], engine=MU.OracleEngine(), new_nodes=new)
            out[-1].append((SU.names_of(res), [((u["pod"]["metadata"].get("namespace", ""), u["pod"]["metadata"]["name"]), u["reason"]) for u in res.unscheduled_pods]))
    return out


def _check(res, cluster, apps, tmpl, counts, hand):
    U, K = len(res.subsets), len(counts)
    pool = list(cluster["Node"]) + (wl.new_fake_nodes(tmpl, max(counts)) if max(counts) else [])
    mine = [{(p["metadata"].get("namespace", ""), p["metadata"]["name"]) for p in wl.app_pods(a.name, a.resource, pool)} for a in apps]
    for u in range(U):
        for k in range(K):
            where, failed = hand[u][k]
            assert res.unscheduled[u][k] == len(failed), (u, k)
            assert [((e["pod"]["metadata"].get("namespace", ""), e["pod"]["metadata"]["name"]), e["reason"]) for e in res.unscheduled_pods[u][k]] == failed, (u, k)
            assert res.unscheduled_by_app[u][k] == [sum(ref in mine[a] for ref, _ in failed) for a in range(len(apps))], (u, k)
            assert res.fits[u][k] == (len(failed) == 0), (u, k)                       # (caps 100: occupancy never refuses)
        fit = [counts[k] for k in range(K) if not hand[u][k][1]]
        assert res.min_count[u] == (min(fit) if fit else None), u
    ok = [u for u in range(U) if not hand[u][0][1]]
    sets = [frozenset(s) for s in res.subsets]
    assert res.maximal == [u for u in ok if not any(sets[u] < sets[v] for v in ok)]
    return ok


CASES = {"simple": lambda: (MU.example_simple(), 2), "gpushare": lambda: (MU.example_gpushare(), 1), "zoned_service": lambda: (MU.random_zoned(5, n_nodes=6), 3)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_apps_equals_simulate_of_every_subset(name):
    """Every subset of the apps (one per workload object) x counts (0, 2), reasons=True, on an oracle-backed engine that honours
    pod_present by running each scenario's OWN problem: names, reason texts, per-app counts, min_count and maximal equal simulate() of
    that subset alone.  `gpushare` has Open-Gpu-Share pods, `zoned_service` a Service and nodes in two zones (per-scenario node ranks)."""
    (cluster, apps, types), keep = CASES[name]()
    apps = _split(apps)[:5]
    cluster = _shrunk(cluster, keep)
    assert len(apps) >= 2
    if name == "zoned_service":
        assert cluster.get("Service")
    counts = (0, 2)
    engine = PU.PodsetOracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.AppFallbackWarning)
        res = sim.sweep_apps(cluster, apps, new_node=types[0], counts=counts, engine=engine, reasons=True)
    assert res.batched and res.fallback is None and engine.batches == 1
    assert res.subsets == [tuple(a for a in range(len(apps)) if (u >> a) & 1) for u in range(1 << len(apps))]
    hand = _by_hand(cluster, apps, res.subsets, types[0], counts)
    ok = _check(res, cluster, apps, types[0], counts, hand)
    assert 0 in ok and len(ok) < len(res.subsets), "the case must hold subsets that fit and subsets that do not"
    lens = [len(wl.app_pods(a.name, a.resource, cluster["Node"])) for a in apps]
    weight = [sum(lens[a] for a in s) for s in res.subsets]
    assert res.best == max(ok, key=lambda u: (weight[u], -u))
    # explicit subsets by name, weights of the caller's, one launch per subset
    named = [[apps[0].name], [a.name for a in apps[:2]], []]
    part = sim.sweep_apps(cluster, apps, subsets=named, new_node=types[0], counts=counts, engine=PU.PodsetOracleEngine(), weights=[1] + [0] * (len(apps) - 1),
                          batch_scenarios=2)
    idx = [res.subsets.index(s) for s in part.subsets]
    assert part.unscheduled == [res.unscheduled[u] for u in idx] and part.unscheduled_by_app == [res.unscheduled_by_app[u] for u in idx]
    assert part.cpu_pct == [res.cpu_pct[u] for u in idx] and part.mem_pct == [res.mem_pct[u] for u in idx]
    if part.best is not None:
        assert 0 in part.subsets[part.best] or not any(0 in part.subsets[u] for u in range(3) if part.fits[u][0])


def test_fallbacks_warn_and_still_answer():
    (cluster, apps, types) = MU.example_simple()
    cluster = _shrunk(cluster, 2)
    split = _split(apps)[:3]
    hand = None
    # 1. an engine without pod subsets
    with pytest.warns(sim.AppFallbackWarning, match="the engine has no pod subsets"):
        res = sim.sweep_apps(cluster, split, new_node=types[0], counts=(0, 2), engine=MU.OracleEngine(), reasons=True)
    assert not res.batched and "no pod subsets" in res.fallback
    hand = _by_hand(cluster, split, res.subsets, types[0], (0, 2))
    _check(res, cluster, split, types[0], (0, 2), hand)
    # 2. an app with a DaemonSet: the example's whole app on the whole cluster, whose own pod order at a size is not the pool's restricted to
    #    that size (the case of test_explain_batch_host's _same_stream test)
    whole, _, _ = MU.example_simple()
    full = [apps[0]] + split[:1]
    assert apps[0].resource.get("DaemonSet")
    with pytest.warns(sim.AppFallbackWarning, match=r"app simple holds a DaemonSet, and its pod order with \d+ new nodes is not the pool's"):
        res = sim.sweep_apps(whole, full, new_node=types[0], counts=(0, 2), engine=PU.PodsetOracleEngine(), reasons=True)
    assert not res.batched and "holds a DaemonSet" in res.fallback
    _check(res, whole, full, types[0], (0, 2), _by_hand(whole, full, res.subsets, types[0], (0, 2)))
    # 3. a StorageClass that only another app defines
    (lc, lapps, ltypes) = MU.example_open_local()
    app = lapps[0]
    sc_app = sim.AppResource("classes", {"StorageClass": app.resource["StorageClass"]})
    user = sim.AppResource("user", {k: v for k, v in app.resource.items() if k != "StorageClass"})
    with pytest.warns(sim.AppFallbackWarning, match="uses a StorageClass that only another app defines"):
        res = sim.sweep_apps(lc, [sc_app, user], subsets=[["classes", "user"], ["classes"], []], new_node=ltypes[0], counts=(0, 1), engine=PU.PodsetOracleEngine(),
                             reasons=True)
    assert not res.batched and len(res.subsets) == 3                   # (the subset without the classes is simulate()'s to refuse: not asked for)
    _check(res, lc, [sc_app, user], ltypes[0], (0, 1), _by_hand(lc, [sc_app, user], res.subsets, ltypes[0], (0, 1)))
    # 3b. an engine with pod subsets but without explain_batch: the failing scenarios are explained one by one, with the same texts
    class NoExplainBatch(PU.PodsetOracleEngine):
        supports_explain_batch = False
        explain_batch = None
    res = sim.sweep_apps(cluster, split, new_node=types[0], counts=(0, 2), engine=NoExplainBatch(), reasons=True)
    assert res.batched
    _check(res, cluster, split, types[0], (0, 2), hand)
    # 4. the engine refuses the batch
    class Refusing(PU.PodsetOracleEngine):
        def run(self, prob, scen, orders, **kw):
            if kw.get("pod_present") is not None:
                e = capi.SimonError("simon_run_loaded failed (-1): refused")
                e.code = capi.ESTATE
                raise e
            return super().run(prob, scen, orders, **kw)
    with pytest.warns(sim.AppFallbackWarning, match="the engine refused the pod-subset batch"):
        res = sim.sweep_apps(cluster, split, new_node=types[0], counts=(0, 2), engine=Refusing(), reasons=True)
    assert not res.batched
    _check(res, cluster, split, types[0], (0, 2), hand)


def test_more_than_twelve_apps_need_explicit_subsets():
    (cluster, apps, types) = MU.example_simple()
    one = _split(apps)[0]
    many = [sim.AppResource(f"a{i}", copy.deepcopy(one.resource)) for i in range(13)]
    with pytest.raises(ValueError, match="pass the subsets"):
        sim.sweep_apps(cluster, many, engine=PU.PodsetOracleEngine())
    with pytest.raises(ValueError, match="names app"):
        sim.sweep_apps(cluster, many, subsets=[["nobody"]], engine=PU.PodsetOracleEngine())
    with pytest.raises(ValueError, match="new node is nil"):
        sim.sweep_apps(cluster, many[:2], counts=(0, 1), engine=PU.PodsetOracleEngine())


def test_rules_restated_on_hand_cases():
    for P in (31, 32, 33):
        W = (P + 31) // 32
        full = capi.presence_words(np.ones((3, P), bool))
        assert full.shape == (3, W) and full.dtype == np.uint32
        assert PU.podset_errors(P, 3, full) == []
        assert PU.podset_errors(P, 3, None) == [] and PU.podset_errors(P, 3, full, loaded=False) == ["nothing loaded"]
        bad = full.copy()
        if P % 32:
            bad[1, W - 1] |= np.uint32(1 << (P % 32))                 # the bit at P
            assert PU.podset_errors(P, 3, bad) == ["bit beyond P"]
        else:
            assert int(full[0, W - 1]) == 0xFFFFFFFF                      # every bit of the last word names a pod: nothing to refuse
        one = np.zeros((1, P), bool)
        one[0, P - 1] = True
        w = capi.presence_words(one)
        assert int(w[0, (P - 1) >> 5]) == 1 << ((P - 1) & 31) and int(w.sum()) == int(w[0, (P - 1) >> 5])
    g = np.array([0, 1, -1, 6, 6], np.int32)
    assert PU.group_errors(5, g, 7) == [] and PU.group_errors(5, g, 6) == ["group id"] and PU.group_errors(5, g, 0) == ["G"]
    assert PU.group_errors(5, g, 1025) == ["G"] and PU.group_errors(5, g, 1024) == [] and PU.group_errors(5, g, 7, have_placement=False) == ["no placements"]
    assert PU.group_errors(5, np.array([-2, 0, 0, 0, 0]), 3) == ["group id"]
    place = np.array([[0, -1, -1, -2, 3], [-2, -2, -2, -2, -2]], np.int32)
    uns, pl = PU.group_counts(place, g, 7)
    assert uns.tolist() == [[0, 1, 0, 0, 0, 0, 0], [0] * 7] and pl.tolist() == [[1, 0, 0, 0, 0, 0, 1], [0] * 7]


def test_host_checks_compile_alone_and_agree(tmp_path):
    """simon_podsets.h -- the validators behind both calls -- is plain C++: a stand-alone program built with the address and undefined-
    behaviour sanitizers runs them on the word edges."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('''
        #include "simon_podsets.h"
        #include <cstdio>
        #include <vector>
        int main() {
            for (int P : {1, 31, 32, 33, 64, 65}) {
                const int W = simon::pod_row_words(P);
                std::vector<uint32_t> w(3 * W, 0u);
                for (int s = 0; s < 3; ++s) for (int p = 0; p < P; ++p) w[s * W + (p >> 5)] |= 1u << (p & 31);
                int bit = -1;
                if (simon::pod_rows_first_bad(w.data(), 3, P, &bit) != -1) return 1;
                if (P & 31) {
                    w[2 * W + W - 1] |= 1u << (P & 31);
                    if (simon::pod_rows_first_bad(w.data(), 3, P, &bit) != 2 || bit != P) return 2;
                }
            }
            std::vector<int32_t> g = {0, -1, 6};
            if (simon::pod_groups_first_bad(g.data(), 3, 7) != -1 || simon::pod_groups_first_bad(g.data(), 3, 6) != 2) return 3;
            g[1] = -2;
            if (simon::pod_groups_first_bad(g.data(), 3, 7) != 1) return 4;
            std::puts("ok");
            return 0;
        }''')
    exe = tmp_path / "t"
    subprocess.check_call([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "open-simulator_amd", "csrc"),
                           "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "ok"


def test_prototypes_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simon_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert "int simon_set_scenario_pods(simon_ctx* ctx, const uint32_t* present );" in hdr
    assert "int simon_fetch_group_counts(simon_ctx* ctx, const int32_t* pod_group , int32_t G, int32_t* unscheduled , int32_t* placed );" in hdr
    assert "#define SIMON_MAX_POD_GROUPS 1024" in hdr and capi.MAX_POD_GROUPS == 1024
    assert {"simon_set_scenario_pods", "simon_fetch_group_counts"} <= set(capi.EXPORTS)
    lib = capi.load_library()
    C = capi.C
    assert lib.simon_set_scenario_pods.argtypes == [C.c_void_p, C.POINTER(C.c_uint32)] and lib.simon_set_scenario_pods.restype is C.c_int
    assert lib.simon_fetch_group_counts.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert lib.simon_fetch_group_counts.restype is C.c_int
    assert sim.HipEngine.supports_pod_subsets


def test_own_problem_is_the_restricted_problem():
    """The yardstick's helper: deleting no pod changes nothing; an absent pod's row reads GATED; the empty scenario's used sums are the state
    before the stream (checked against a problem whose only pod is gated out); every pod-indexed field of capi.Problem is sliced."""
    import dataclasses
    prob = randprob.rand_problem(7, N=20, P=60, gates=True, init_state=True, nz_differs=True, gpu=True, eph=True, scalars=2, pins=True)
    P = prob.n_pods
    sliced = set(PU.POD_1D + PU.POD_COL)
    for f in dataclasses.fields(prob):
        v = getattr(prob, f.name)
        if isinstance(v, np.ndarray) and v.shape and v.shape[-1] == P and f.name not in sliced:
            assert P in (prob.n_nodes, prob.n_pod_classes) or f.name in ("static_reason",), f"{f.name} looks pod-indexed and is not sliced"
    order = np.random.default_rng(1).permutation(P).astype(np.int32)
    import oracle_lib as O
    ref = O.run(prob, [[15, 0]], order[None], want_gpu_slices=True)
    same = PU.oracle_prefix(prob, np.ones(P, bool), 15, order)
    assert same.placement.tolist() == ref.placement[0].tolist() and same.used_cpu == int(ref.used_cpu[0])
    keep = np.random.default_rng(2).random(P) < 0.5
    part = PU.oracle_prefix(prob, keep, 15, order)
    assert (part.placement[~keep] == capi.GATED).all() and (part.placement[keep] != capi.GATED).sum() > 0
    lone = PU.own_problem(prob, np.arange(P) == 0)[0]
    lone.gate_node = np.array([19], np.int32)
    lone.preset_node, lone.pin_node = np.array([-1], np.int32), np.array([-1], np.int32)
    none = O.run(lone.normalise(), [[15, 0]], np.zeros((1, 1), np.int32))
    empty = PU.oracle_prefix(prob, np.zeros(P, bool), 15, order)
    assert (empty.unscheduled, empty.used_cpu, empty.used_mem) == (0, int(none.used_cpu[0]), int(none.used_mem[0]))

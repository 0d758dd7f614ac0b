"""Per-node usage and headroom, the host side (no GPU): the header text and the ctypes prototypes; the definition of headroom against the
unmodified oracle -- fit + 3 copies of an exact probe appended to the stream, exactly fit of them placed; the usage restatement against
the oracle's used sums; the sweeps' headroom= / node_table= on oracle-backed engines against simulate() of every scenario."""
import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

import mix_util as MU
import oracle_lib as O
import usage_util as UU
from open_simulator_amd import capi, flatten as fl, quantity, simulate as sim, workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(3, 5), (4, 5), (3, 70), (4, 70)]                  # (seed, N)


def test_header_declares_and_capi_exports_both_calls():
    text = open(os.path.join(ROOT, "include", "simon_hip.h")).read()
    hdr = re.sub(r"[ \n]+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int simon_fetch_node_usage(simon_ctx* ctx, const int32_t* scen_ids , int32_t n, simon_node_usage* out);" in hdr
    assert ("int simon_fetch_headroom(simon_ctx* ctx, const int32_t* probe_pod , int32_t K, int64_t* fit , int32_t* fit_nodes , "
            "uint8_t* exact );") in hdr
    assert ("typedef struct simon_node_usage { uint32_t struct_size; int64_t* req_cpu; int64_t* req_mem; int64_t* req_eph; "
            "int64_t* scalar_req; int32_t* npods; } simon_node_usage;") in hdr
    assert "#define SIMON_MAX_PROBES 64" in hdr and capi.MAX_PROBES == 64
    assert "#define SIMON_HIP_ABI_VERSION 7 " in text and capi.ABI_VERSION == 7
    assert {"simon_fetch_node_usage", "simon_fetch_headroom"} <= set(capi.EXPORTS)
    assert "simon_group_fetch_node_usage" not in text and "simon_group_fetch_headroom" not in text
    assert not any(n.startswith("simon_group_") and ("usage" in n or "headroom" in n) for n in capi.EXPORTS)
    lib = capi.load_library()
    assert lib.simon_fetch_node_usage.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(capi.NodeUsageC)]
    assert lib.simon_fetch_headroom.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_uint8)]
    assert lib.simon_fetch_node_usage.restype is C.c_int and lib.simon_fetch_headroom.restype is C.c_int
    assert C.sizeof(capi.NodeUsageC) == 48 and capi.NodeUsageC.npods.offset == 40
    assert sim.HipEngine.supports_node_usage is True


@functools.lru_cache(maxsize=None)
def _case(seed, N):
    """(problem, named probes, order, oracle result of the one full-size scenario, its usage and held rows)."""
    prob, named = UU.constructed_problem(seed, N)
    order = np.random.default_rng(seed).permutation(prob.n_pods).astype(np.int32)
    res = O.run(prob, [[N, 0]], order[None])
    held = UU.held_rows(prob, [[N, 0]])
    return prob, named, order, res, UU.node_usage(prob, res.placement, held), held


def _probes(prob, named):
    """The constructed probes and a handful of the stream's own exact pods (one per pod class at most)."""
    out, seen = dict(named), set()
    for p in range(prob.n_pods):
        c = int(prob.pod_class[p])
        if p not in named.values() and c not in seen and UU.probe_exact(prob, p):
            seen.add(c)
            out[f"class{c}"] = p
    return out


@pytest.mark.parametrize("seed,N", CASES)
def test_headroom_is_what_the_oracle_places_of_appended_probes(seed, N):
    prob, named, order, res, usage, held = _case(seed, N)
    probes = _probes(prob, named)
    ids = list(probes.values())
    fit, nodes, exact = UU.headroom(prob, res.placement, held, ids, usage)
    for name in named:
        assert exact[ids.index(named[name])], name
    assert (fit[0] > 0).any() and (fit[0] == 0).any(), fit[0].tolist()          # (a seed whose probes all fit, or all do not, shows little)
    checked = 0
    for k, (name, p) in enumerate(probes.items()):
        assert exact[k], name
        UU.check_probe_against_oracle(prob, N, order, res.placement[0], p, fit[0, k])
        assert (fit[0, k] > 0) == (nodes[0, k] > 0)
        checked += 1
    assert checked >= 6


@pytest.mark.parametrize("seed,N", CASES)
def test_the_constructed_probes_meet_the_rules_they_were_made_for(seed, N):
    prob, named, order, res, usage, held = _case(seed, N)
    K = 1
    alloc = lambda j: [prob.alloc_cpu[j], prob.alloc_mem[j], 0 if prob.alloc_eph is None else prob.alloc_eph[j], prob.scalar_alloc[0][j]]   # noqa: E731
    used = lambda j: [usage.req_cpu[0, j], usage.req_mem[0, j], usage.req_eph[0, j], usage.scalar_req[0, 0, j]]                              # noqa: E731
    cap = lambda p, j: UU.cap_of(prob.alloc_pods[j], usage.npods[0, j], alloc(j), used(j), *UU.probe_request(prob, p))                        # noqa: E731
    assert K == len(prob.scalar_alloc)
    # BestEffort: the pod slots are the only bound, over-committed nodes included
    be = named["besteffort"]
    assert UU.probe_request(prob, be) == ([0, 0, 0, 0], 0)
    assert [cap(be, j) for j in range(N)] == [max(int(prob.alloc_pods[j]) - int(usage.npods[0, j]), 0) for j in range(N)]
    # node 0 is over-committed in cpu through a preset pod: a pod that asks for memory only still fails "Insufficient cpu" there
    assert usage.req_cpu[0, 0] > prob.alloc_cpu[0]
    assert cap(named["zero_cpu"], 0) == 0 and UU.probe_request(prob, named["zero_cpu"])[0][0] == 0
    # a scalar ENTRY of quantity 0 switches the shortcut off: the same empty request is now compared on node 0
    assert UU.probe_request(prob, named["zero_entry"]) == ([0, 0, 0, 0], 1)
    assert cap(named["zero_entry"], 0) == 0
    slots0 = max(int(prob.alloc_pods[0]) - int(usage.npods[0, 0]), 0)
    assert cap(be, 0) == slots0
    # the masked probe's class leaves nodes out
    cls = int(prob.pod_class[named["masked"]])
    assert not all(UU.static_ok(prob, cls, j) for j in range(N))
    assert cap(named["fat"], 0) == 0 and all(cap(named["fat"], j) == 0 for j in range(N))


@pytest.mark.parametrize("seed,N", CASES)
def test_usage_sums_are_the_oracle_s_used_sums_and_absent_nodes_read_minus_one(seed, N):
    prob, named, order, _, _, _ = _case(seed, N)
    scen = np.array([[N, 0], [max(1, N // 2), 0], [max(1, N - 1), 0]], np.int32)
    res = O.run(prob, scen, order[None])
    held = UU.held_rows(prob, scen)
    u = UU.node_usage(prob, res.placement, held)
    assert u.req_cpu.sum(1).tolist() == res.used_cpu.tolist()
    assert u.req_mem.sum(1).tolist() == res.used_mem.tolist()
    assert ((u.npods == -1) == ~held).all() and (u.req_cpu[~held] == 0).all() and (u.scalar_req.transpose(0, 2, 1)[~held] == 0).all()
    assert (u.npods[held].sum() == (res.placement >= 0).sum() + (0 if prob.init_npods is None else int((held * prob.init_npods[None, :]).sum())))
    # the host road of the sweeps (simulate.host_node_usage / host_headroom) is the same definition, vectorised
    h = sim.host_node_usage(prob, res.placement, held)
    for name in ("req_cpu", "req_mem", "req_eph", "scalar_req", "npods"):
        assert (getattr(h, name) == getattr(u, name)).all(), name
    ids = list(_probes(prob, named).values())
    fit, nodes, exact = UU.headroom(prob, res.placement, held, ids, u)
    hf, hn, hx = sim.host_headroom(prob, res.placement, held, ids)
    assert (hf == fit).all() and (hn == nodes).all() and hx.tolist() == exact.tolist()


def test_the_refusal_rules_restated():
    assert UU.usage_errors(6, None, 6) == [] and UU.usage_errors(6, [5, 0, 5], 3) == []
    assert UU.usage_errors(6, None, 0) == ["n"] and UU.usage_errors(6, None, 7) == ["scenario id"]
    assert UU.usage_errors(6, [0, 6], 2) == ["scenario id"] and UU.usage_errors(6, [-1], 1) == ["scenario id"]
    assert UU.usage_errors(6, None, 6, have=("req_cpu", "npods")) == ["missing array"]
    assert UU.usage_errors(6, None, 6, struct_ok=False) == ["struct_size"]
    assert UU.usage_errors(6, None, 6, have_placement=False) == ["no placements"] == UU.usage_errors(6, None, 6, reloaded=True)
    assert UU.headroom_errors(10, [0, 9], 2) == []
    assert UU.headroom_errors(10, [0], 0) == ["K"] == UU.headroom_errors(10, [0] * 65, 65)
    assert UU.headroom_errors(10, [10], 1) == ["pod id"] == UU.headroom_errors(10, [-1], 1)
    assert UU.headroom_errors(10, [0], 1, have_fit=False) == ["missing array"]
    assert UU.headroom_errors(10, [0], 1, reloaded=True) == ["no placements"]


# ---- the sweeps ----------------------------------------------------------------------------------------------------------------------

def _table_of(res):
    """reportClusterInfo's columns from a SimulateResult: requests summed per node over its pods (flatten.pod_requests_quantities)."""
    rows = []
    for st in res.node_status:
        node = st["node"]
        reqs = [fl.pod_requests_quantities(p) for p in st["pods"]]
        al = node["status"]["allocatable"]
        rows.append({"node": node["metadata"]["name"], "cpu_allocatable": quantity.parse_quantity(str(al["cpu"])).milli_value(),
                     "cpu_requests": sum(r["cpu"].milli_value() for r in reqs if "cpu" in r),
                     "memory_allocatable": quantity.parse_quantity(str(al["memory"])).int_value(),
                     "memory_requests": sum(r["memory"].int_value() for r in reqs if "memory" in r), "pods": len(st["pods"]),
                     "new": wl.LABEL_NEW_NODE in (node["metadata"].get("labels") or {})})
    return rows


def _simple_without_app_daemonset():
    cluster, apps, types = MU.example_simple()
    return cluster, [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps], types


def _by_name(rows):
    return sorted(rows, key=lambda r: r["node"])


def test_sweep_node_table_equals_simulate_of_every_size():
    cluster, apps, types = _simple_without_app_daemonset()          # (with the app's DaemonSet a size's own stream is not the pool's: _same_stream)
    counts = [0, 1, 3]
    sw = sim.sweep(cluster, apps, types[0], counts, engine=UU.UsageOracleEngine(), node_table=True)
    assert sw.headroom is None and sw.headroom_exact is None and len(sw.node_table) == len(counts)
    pool = [n["metadata"]["name"] for n in cluster["Node"]] + [n["metadata"]["name"] for n in wl.new_fake_nodes(types[0], max(counts))]
    for s, k in enumerate(counts):
        res = sim.simulate(cluster, apps, engine=MU.OracleEngine(), new_nodes=wl.new_fake_nodes(types[0], k) if k else ())
        assert [r["node"] for r in sw.node_table[s]] == pool[:len(cluster["Node"]) + k]              # pool order
        assert _by_name(sw.node_table[s]) == _by_name(_table_of(res)), k
        assert [r["new"] for r in sw.node_table[s]] == [False] * len(cluster["Node"]) + [True] * k


def _headroom_of(cluster, apps, refs):
    """The numpy figure of one cluster's own simulate(): flatten as simulate() does, the oracle's placement, the restatement."""
    nodes = list(cluster["Node"])
    pods, _ = sim.build_stream(cluster, apps, nodes, len(nodes))
    from open_simulator_amd import k8s
    arrival = [n["metadata"]["name"] for n in nodes]
    nodes = [nodes[j] for j in k8s.canonical_node_order(nodes)]
    flat = fl.flatten(nodes, pods, cluster.get("Service", []), cluster.get("ReplicaSet", []), cluster.get("StatefulSet", []),
                      image_total=len(nodes), node_arrival_order=arrival)
    res = O.run(flat.problem, [[len(nodes), 0]], np.arange(len(pods), dtype=np.int32)[None])
    ids = [flat.pod_refs.index(r) for r in refs]
    fit, _, exact = UU.headroom(flat.problem, res.placement, np.ones((1, len(nodes)), bool), ids)
    return fit[0].tolist(), exact.tolist()


def _app_refs(cluster, apps, n=3):
    """(namespace, name) of the first pods of n distinct workloads of the apps."""
    pods, _ = sim.build_stream(cluster, apps, list(cluster["Node"]), len(cluster["Node"]))
    refs, seen = [], set()
    for p in pods:
        owner = (p["metadata"].get("ownerReferences") or [{}])[0].get("name")
        if owner and owner not in seen and not (p.get("spec") or {}).get("nodeName") and "_daemon_node" not in p:
            seen.add(owner)
            refs.append((p["metadata"]["namespace"], p["metadata"]["name"]))
    return refs[:n]


def test_sweep_failures_headroom_equals_the_figure_of_every_reduced_cluster():
    cluster, apps, _ = _simple_without_app_daemonset()
    refs = _app_refs(cluster, apps)
    assert len(refs) >= 2
    eng = UU.UsageOracleEngine()
    sw = sim.sweep_failures(cluster, apps, "node", engine=eng, headroom=refs, node_table=True)
    assert sw.batched and len(sw.headroom) == len(sw.domains) + 1 == len(sw.node_table)
    exact_all = None
    for s, names in enumerate([[]] + sw.domains):
        fit, exact = _headroom_of(*sim.cluster_without(cluster, apps, names), refs)
        assert sw.headroom[s] == fit, (s, names)
        exact_all = exact if exact_all is None else exact_all
        assert [r["node"] for r in sw.node_table[s]] == [n["metadata"]["name"] for n in cluster["Node"] if n["metadata"]["name"] not in names]
    assert sw.headroom_exact == exact_all
    assert any(v > 0 for row in sw.headroom for v in row)


def test_an_engine_without_the_calls_warns_and_returns_the_same_figures():
    cluster, apps, types = _simple_without_app_daemonset()
    refs = _app_refs(cluster, apps)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                             # the device road warns nowhere
        a = sim.sweep(cluster, apps, types[0], [0, 2], engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
        fa = sim.sweep_failures(cluster, apps, "node", engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
        plain = sim.sweep(cluster, apps, types[0], [0, 2], engine=UU.UsageOracleEngine())
    assert plain.headroom is None and plain.headroom_exact is None and plain.node_table is None       # defaults leave the result alone
    with pytest.warns(sim.UsageFallbackWarning, match="supports_node_usage"):
        b = sim.sweep(cluster, apps, types[0], [0, 2], engine=UU.PlainOracleEngine(), headroom=refs, node_table=True)
    with pytest.warns(sim.FailureFallbackWarning, match="supports_node_usage"):
        fb = sim.sweep_failures(cluster, apps, "node", engine=UU.PlainOracleEngine(), headroom=refs, node_table=True)
    with pytest.warns(sim.FailureFallbackWarning, match="one by one"):                                # no node subsets at all: scenario by scenario
        fc = sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine(), headroom=refs, node_table=True)
    for x, y in ((a, b), (fa, fb), (fa, fc)):
        assert x.headroom == y.headroom and x.headroom_exact == y.headroom_exact and x.node_table == y.node_table
    assert not fc.batched and fb.batched
    with pytest.warns(sim.FailureFallbackWarning), pytest.raises(ValueError, match="namespace, name"):
        sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine(), headroom=[0])
    with pytest.raises(ValueError, match="not a pod of the stream"):
        sim.sweep(cluster, apps, types[0], [0], engine=UU.UsageOracleEngine(), headroom=[("default", "no-such-pod")])


def test_sweep_mix_and_sweep_apps_carry_the_fields():
    cluster, apps, types = _simple_without_app_daemonset()
    refs = _app_refs(cluster, apps)
    with pytest.warns(sim.MixFallbackWarning):                                     # (no pool segments on this engine: every mix on its own)
        mx = sim.sweep_mix(cluster, apps, types, [[0, 1], [0, 1]], engine=UU.PlainOracleEngine(), headroom=refs, node_table=True)
    assert len(mx.headroom) == 4 == len(mx.node_table) and len(mx.headroom_exact) == len(refs)
    for s, mix in enumerate(mx.counts):
        new = [n for nn in sim.mix_fake_nodes(types, mix) for n in nn]
        fit, _ = _headroom_of(dict(cluster, Node=list(cluster["Node"]) + new), apps, refs)
        assert mx.headroom[s] == fit, mix
        assert [r["node"] for r in mx.node_table[s]] == [n["metadata"]["name"] for n in list(cluster["Node"]) + new]
    split = [sim.AppResource(f"{k.lower()}-{o['metadata']['name']}", {k: [o]}) for a in apps for k, v in a.resource.items()
             if k in ("Deployment", "StatefulSet", "ReplicaSet", "Job") for o in v][:3]
    ap = sim.sweep_apps(cluster, split, new_node=types[0], counts=[0, 1], engine=UU.UsageOracleEngine(), headroom=_app_refs(cluster, split, 2), node_table=True)
    assert ap.batched and np.asarray(ap.headroom).shape == (len(ap.subsets), 2, 2) and len(ap.node_table[0][1]) == len(cluster["Node"]) + 1
    with pytest.warns(sim.AppFallbackWarning, match="supports_node_usage"):
        bp = sim.sweep_apps(cluster, split, new_node=types[0], counts=[0, 1], engine=UU.PlainOracleEngine(), headroom=_app_refs(cluster, split, 2), node_table=True)
    assert ap.headroom == bp.headroom and ap.headroom_exact == bp.headroom_exact and ap.node_table == bp.node_table

"""Open-Local usage and the storage bound of headroom, host side: simulate.host_local_usage / host_headroom(storage=True) -- the replay
the device kernels are compared against in test_local_usage.py -- checked against the unmodified oracle three independent ways (the
cluster total used_vg, appended copies of every exact storage probe, the per-node numbers of the oracle's own error detail), the hand
cases of the definition, header and ctypes prototypes, and the sweeps' storage=True on oracle-backed engines."""
import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

import local_usage_util as LU
import mix_util as MU
import oracle_lib as O
import usage_util as UU
from open_simulator_amd import capi, simulate as sim

GiB = LU.GiB


@functools.lru_cache(maxsize=None)
def _case(N, P):
    prob, scen, orders = LU.random_case(N, P)
    ref = O.run(prob, scen, orders)
    held = UU.held_rows(prob, scen)
    use = sim.host_local_usage(prob, ref.placement, held, orders, scen)
    return prob, scen, orders, ref, held, use


# ---- 1. the sum against used_vg -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", LU.CASES)
def test_vg_req_summed_over_a_scenario_is_the_oracle_s_used_vg(N, P):
    prob, scen, orders, ref, held, use = _case(N, P)
    assert scen[0, 1] == 1 and sorted(orders[1].tolist()) == list(range(P)) and orders[1].tolist() != list(range(P))   # a permuted order
    ann = (np.asarray(prob.local_flags) & 1) != 0
    live = np.arange(capi.MAX_VG)[None, :] < np.asarray(prob.local_vg_cnt)[:, None]
    for s in range(len(scen)):
        total = int((use.vg_req[s] * (held[s] & ann)[:, None] * live).sum())
        assert total == int(use.vg_req[s].sum()), "vg_req is 0 outside the held annotated nodes' own groups"
        assert total == int(ref.used_vg[s]), (s, total, int(ref.used_vg[s]))
    assert ref.used_vg[0] > (np.asarray(prob.init_vg_req) * ann[:, None] * live).sum(), "the stream committed nothing"
    assert ((use.dev_alloc == -1) == ~held).all()
    assert not use.dev_alloc[held & ~ann[None, :]].any()


# ---- 2. appended copies: what `exact` promises ----------------------------------------------------------------------------------------
def _bounds(prob, scen, orders, ref, held, probes):
    """(fit with the storage bound, fit without) [S][K] and the per-node pairs (resource cap, storage cap) of scenario 0."""
    fit, nodes, exact = sim.host_headroom(prob, ref.placement, held, probes, storage=True, orders=orders, scen=scen)
    plain, _, px = sim.host_headroom(prob, ref.placement, held, probes)
    assert exact.all() and not px.any()
    pairs = []
    state = sim._local_states(prob, ref.placement[0], orders[int(scen[0][1])])
    for k, p in enumerate(probes):
        one = np.zeros_like(held[:1])
        for j in np.flatnonzero(held[0]).tolist():
            one[:] = False
            one[0, j] = True
            res_cap = int(sim.host_headroom(prob, ref.placement[:1], one, [p])[0][0, 0])
            big = np.full(prob.n_nodes, 1 << 20, np.int64)
            loc = int(sim._local_caps(prob, LU.spec_of_pod(prob, p), state, big)[j]) if UU.static_ok(prob, int(prob.pod_class[p]), j) else 0
            pairs.append((res_cap, loc))
    return fit, plain, pairs


@pytest.mark.parametrize("N,P", LU.CASES)
def test_exactly_fit_appended_copies_of_a_storage_probe_are_placed(N, P):
    prob, scen, orders, ref, held, use = _case(N, P)
    probes = LU.storage_probes(prob)
    assert len(probes) >= 3
    fit, plain, _ = _bounds(prob, scen, orders, ref, held, probes)
    assert (fit <= plain).all()
    for k, p in enumerate(probes):
        UU.check_probe_against_oracle(prob, int(scen[0, 0]), orders[scen[0, 1]], ref.placement[0], p, fit[0, k])


def test_the_random_cases_cover_every_volume_kind_and_both_orders_of_the_bounds():
    kinds, below, above = set(), False, False
    for N, P in LU.CASES:
        prob, scen, orders, ref, held, use = _case(N, P)
        probes = LU.storage_probes(prob)
        for p in probes:
            kinds |= LU.kinds_of(prob, p)
        _, _, pairs = _bounds(prob, scen, orders, ref, held, probes)
        below = below or any(loc < res for res, loc in pairs)
        above = above or any(0 < res < loc for res, loc in pairs)
    assert kinds == {"named", "any", "device"}
    assert below and above


# ---- 3. per-node state through the oracle's own error detail ---------------------------------------------------------------------------
def _detail_problem():
    """5 annotated nodes with 2 or 3 of the volume groups named 0, 1, 2, ample pod slots; a mixed stream of named-VG and any-VG pods
    (and device pods); at its end one BestEffort pod per VG name asking for 2^60 bytes of that group, and one asking for 4 SSDs."""
    rng = np.random.default_rng(5)
    nodes = []
    for j in range(5):
        names = rng.permutation(3)[:2 + j % 2].tolist()
        nodes.append(LU.node(vgs=[(v, int(rng.choice([60, 100, 150])), int(rng.choice([0, 5]))) for v in names],
                             devs=[(LU.SSD, int(rng.choice([50, 100])), int(rng.random() < 0.2)) for _ in range(int(rng.integers(2, 6)))],
                             pods=500))
    pods = []
    for _ in range(60):
        kind = int(rng.integers(0, 4))
        size = int(rng.choice([2, 5, 9, 14]))
        if kind == 0:
            pods.append(LU.pod(lvm=[(size, int(rng.integers(0, 3)))]))
        elif kind == 1:
            pods.append(LU.pod(lvm=[(size, -1), (3, -1)]))
        elif kind == 2:
            pods.append(LU.pod(lvm=[(size, int(rng.integers(0, 3))), (size, -1)]))
        else:
            pods.append(LU.pod(ssd=[int(rng.choice([10, 40]))]))
    tail = [LU.pod(lvm=[(1 << 30, v)], cpu=0, mem=0) for v in range(3)] + [LU.pod(ssd=[1, 1, 1, 1], cpu=0, mem=0)]
    return LU.problem(nodes, pods + tail), len(pods)


def test_vg_req_and_free_devices_equal_the_numbers_in_the_oracle_s_error_detail():
    prob, n_stream = _detail_problem()
    N, P = prob.n_nodes, prob.n_pods
    order = np.concatenate([np.random.default_rng(2).permutation(n_stream), np.arange(n_stream, P)]).astype(np.int32)
    scen = np.array([[N, 0]], np.int32)
    ref, (nf, failed, codes) = O.run(prob, scen, order[None], explain_scenario=0, max_failed=8)
    detail = O.LAST_LOCAL_DETAIL[0]
    assert (ref.placement[0, :n_stream] >= 0).sum() >= n_stream - 5
    use = sim.host_local_usage(prob, ref.placement, UU.held_rows(prob, scen), order[None], scen)
    compared = set()
    for v in range(3):                                                  # the 2^60-byte probes: one per VG name
        p = n_stream + v
        assert ref.placement[0, p] == capi.UNSCHEDULED
        row = detail[failed.tolist().index(p)]
        for j in range(N):
            names = np.asarray(prob.local_vg_name)[j, :prob.local_vg_cnt[j]].tolist()
            if v not in names:
                assert row[j, 0] == capi.LOCAL_ERR_NO_SUCH_VG
                continue
            q = names.index(v)
            assert row[j].tolist() == [capi.LOCAL_ERR_LVM, 1 << 60, int(use.vg_req[0, j, q]), int(prob.local_vg_cap[j, q])], (v, j, row[j])
            compared.add((j, q))
    assert compared == {(j, q) for j in range(N) for q in range(int(prob.local_vg_cnt[j]))}, "every volume group of every node was compared"
    assert (use.vg_req[0] > np.asarray(prob.init_vg_req)).sum() >= 5
    p = P - 1                                                           # the 4-SSD probe
    row = detail[failed.tolist().index(p)]
    short = 0
    for j in range(N):
        free = [d for d in range(int(prob.local_dev_cnt[j])) if not (int(use.dev_alloc[0, j]) >> d) & 1]
        if len(free) < 4:
            assert row[j].tolist() == [capi.LOCAL_ERR_DEVICE, 4, len(free), int(prob.local_dev_cnt[j])], (j, row[j])
            short += 1
    assert short >= 2
    assert (use.dev_alloc[0] != np.asarray(prob.init_dev_alloc)).any()


# ---- hand cases ------------------------------------------------------------------------------------------------------------------------
def _two_orders():
    """One node whose groups have 10 and 20 GiB free; A asks 8 GiB, B 12 GiB, both of any group."""
    prob = LU.problem([LU.node(vgs=[(0, 10, 0), (1, 20, 0)])], [LU.pod(lvm=[(8, -1)]), LU.pod(lvm=[(12, -1)])])
    return prob, np.array([[1, 0], [1, 1]], np.int32), np.array([[0, 1], [1, 0]], np.int32)


def test_the_same_placements_in_another_order_leave_another_state():
    prob, scen, orders = _two_orders()
    ref = O.run(prob, scen, orders)
    assert ref.placement.tolist() == [[0, 0], [0, 0]]
    use = sim.host_local_usage(prob, ref.placement, UU.held_rows(prob, scen), orders, scen)
    assert (use.vg_req[:, 0, :2] // GiB).tolist() == [[8, 12], [0, 20]]
    assert ref.used_vg.tolist() == [20 * GiB, 20 * GiB]
    rev = sim.host_local_usage(prob, ref.placement, UU.held_rows(prob, scen), orders, scen, [1, 0, 1])
    assert rev.scenarios.tolist() == [1, 0, 1] and (rev.vg_req[:, 0, :2] // GiB).tolist() == [[0, 20], [8, 12], [0, 20]]


def test_a_device_shortfall_without_a_too_small_last_device_commits_fewer_devices():
    # free SSDs of 10, 20 and 100 GiB; volumes of 50 and 60: the 10 and the 20 are skipped, the 100 takes the 50, and the list ends --
    # the 60 is never matched, yet the match "fits" and one device is committed
    prob = LU.problem([LU.node(devs=[(LU.SSD, 10, 0), (LU.SSD, 20, 0), (LU.SSD, 100, 0)])], [LU.pod(ssd=[50, 60])])
    scen, order = np.array([[1, 0]], np.int32), np.array([[0]], np.int32)
    ref = O.run(prob, scen, order)
    assert ref.placement.tolist() == [[0]]
    use = sim.host_local_usage(prob, ref.placement, UU.held_rows(prob, scen), order, scen)
    assert use.dev_alloc.tolist() == [[0b100]]
    # and the event itself: the last device too small for the volume in turn
    assert sim._local_allocate(prob, 0, [0] * 4, 0b100, LU.spec_of_pod(prob, 0)) is None
    fit, _, exact = sim.host_headroom(prob, ref.placement, UU.held_rows(prob, scen), [0], storage=True, orders=order, scen=scen)
    assert fit.tolist() == [[0]] and exact.all()
    UU.check_probe_against_oracle(prob, 1, order[0], ref.placement[0], 0, 0)


def test_a_pod_bound_by_node_name_commits_nothing():
    prob = LU.problem([LU.node(vgs=[(0, 100, 5)], devs=[(LU.SSD, 50, 0)])], [LU.pod(lvm=[(10, -1)], ssd=[10], preset=0), LU.pod(lvm=[(7, -1)])])
    scen, order = np.array([[1, 0]], np.int32), np.array([[0, 1]], np.int32)
    ref = O.run(prob, scen, order)
    assert ref.placement.tolist() == [[0, 0]]
    use = sim.host_local_usage(prob, ref.placement, UU.held_rows(prob, scen), order, scen)
    assert (use.vg_req[0, 0] // GiB).tolist() == [12, 0, 0, 0] and use.dev_alloc.tolist() == [[0]]
    assert ref.used_vg.tolist() == [12 * GiB]


def test_a_probe_whose_volumes_have_size_0_is_bounded_by_the_resources_alone():
    prob = LU.problem([LU.node(vgs=[(0, 10, 10)], pods=7), LU.node(annotated=False, pods=7)], [LU.pod(lvm=[(0, -1)]), LU.pod()])
    scen, order = np.array([[2, 0]], np.int32), np.array([[1, 0]], np.int32)
    ref = O.run(prob, scen, order)
    held = UU.held_rows(prob, scen)
    fit, nodes, exact = sim.host_headroom(prob, ref.placement, held, [0, 1], storage=True, orders=order, scen=scen)
    res, _, _ = sim.host_headroom(prob, ref.placement, held, [0, 1])
    on0 = int((ref.placement[0] == 0).sum())
    assert fit[0].tolist() == [7 - on0, int(res[0, 1])] and nodes[0, 0] == 1        # the full group still holds any number of size-0 volumes; node 1: no annotation
    UU.check_probe_against_oracle(prob, 2, order[0], ref.placement[0], 0, fit[0, 0])


def test_a_node_without_the_annotation_holds_no_storage_pod():
    prob = LU.problem([LU.node(annotated=False), LU.node(vgs=[(0, 10, 0)])], [LU.pod(lvm=[(4, -1)])])
    scen, order = np.array([[2, 0], [1, 0]], np.int32), np.array([[0]], np.int32)
    ref = O.run(prob, scen, order)
    assert ref.placement.tolist() == [[1], [capi.UNSCHEDULED]]
    held = UU.held_rows(prob, scen)
    fit, nodes, exact = sim.host_headroom(prob, ref.placement, held, [0], storage=True, orders=order, scen=scen)
    assert fit.tolist() == [[1], [0]] and nodes.tolist() == [[1], [0]]
    use = sim.host_local_usage(prob, ref.placement, held, order, scen)
    assert use.dev_alloc.tolist() == [[0, 0], [0, -1]] and (use.vg_req[:, :, 0] // GiB).tolist() == [[0, 4], [0, 0]]


# ---- header, prototypes ----------------------------------------------------------------------------------------------------------------
def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "simon_hip.h")).read()


def test_header_block_and_ctypes_prototypes_agree():
    h = _header()
    m = re.search(r"typedef struct simon_local_usage \{(.*?)\} simon_local_usage;", h, re.S)
    fields = re.findall(r"^\s*(uint32_t|int64_t\*|int32_t\*)\s+(\w+);", m.group(1), re.M)
    ctype = {"uint32_t": C.c_uint32, "int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32)}
    assert [(n, ctype[t]) for t, n in fields] == list(capi.LocalUsageC._fields_)
    assert re.search(r"int simon_fetch_local_usage\(simon_ctx\* ctx, const int32_t\* scen_ids /\*.*?\*/, int32_t n, simon_local_usage\* out\);", h)
    assert re.search(r"int simon_fetch_headroom_local\(simon_ctx\* ctx, const int32_t\* probe_pod /\*.*?\*/, int32_t K,\s*int64_t\* fit /\*.*?\*/, int32_t\* fit_nodes /\*.*?\*/, uint8_t\* exact /\*.*?\*/\);", h)
    assert "#define SIMON_HIP_ABI_VERSION 7 " in h
    assert {"simon_fetch_local_usage", "simon_fetch_headroom_local"} <= set(capi.EXPORTS)
    assert sim.HipEngine.supports_local_usage
    text = h[h.index("simon_fetch_local_usage: the"):h.index("typedef struct simon_local_usage")]
    for word in ("simon_group_*", "Go shim", "not pods of the loaded stream", "the ABI stays 7"):
        assert word in text



# ---- the sweeps ------------------------------------------------------------------------------------------------------------------------

FIELDS = ("unscheduled", "headroom", "headroom_exact", "node_table", "storage_table")


@functools.lru_cache(maxsize=None)
def _example():
    """The reference's example/application/open_local on cluster/demo_1 (tests/golden/example), its apps without DaemonSets, and two
    probes: an nginx-lvm pod (two LVM volumes and an exclusive HDD) and a cluster pod without volumes."""
    cluster, apps, types = MU.example_open_local()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    batch = sim.sweep_batch(cluster, apps, types[0], [0])
    refs = batch.flat.pod_refs
    lvm = next(r for p, r in enumerate(refs) if LU.spec_of_pod(batch.flat.problem, p) is not None and LU.probe_exact_local(batch.flat.problem, p))
    plain = next(r for p, r in enumerate(refs) if LU.spec_of_pod(batch.flat.problem, p) is None and batch.flat.problem.preset_node[p] < 0)
    return cluster, apps, types, [lvm, plain]


def _same(a, b, fields=FIELDS):
    for f in fields:
        assert getattr(a, f) == getattr(b, f), f


def _warned(rec, cls):
    return [w for w in rec if issubclass(w.category, cls) and "on the host" in str(w.message)]


def test_sweep_with_storage_on_engines_with_and_without_the_calls():
    cluster, apps, types, refs = _example()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=LU.LocalUsageOracleEngine(), headroom=refs, node_table=True, storage=True)
    assert not _warned(rec, sim.UsageFallbackWarning)
    with pytest.warns(sim.UsageFallbackWarning, match="supports_local_usage"):
        b = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=LU.GpuUsageOnlyEngine(), headroom=refs, node_table=True, storage=True)
    _same(a, b)
    assert a.headroom_exact[0] and len(a.storage_table) == 3
    old = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=LU.LocalUsageOracleEngine(), headroom=refs, node_table=True)
    assert not old.headroom_exact[0] and old.headroom_exact[1] == a.headroom_exact[1] and old.storage_table is None
    assert all(x <= y for ra, ro in zip(a.headroom, old.headroom) for x, y in zip(ra, ro))
    assert any(ra[k] < ro[k] for ra, ro in zip(a.headroom, old.headroom) for k in (0,)), "storage is the bottleneck somewhere"
    assert [ra[1] for ra in a.headroom] == [ro[1] for ro in old.headroom]
    # more nodes, more rows: every scenario lists the annotated nodes it holds
    assert len({r["node"] for r in a.storage_table[0]}) < len({r["node"] for r in a.storage_table[2]})


def test_storage_false_leaves_the_sweeps_results_as_they_are():
    cluster, apps, types, refs = _example()
    eng = LU.LocalUsageOracleEngine
    for call, kw in ((sim.sweep, dict(new_node=types[0], counts=[0, 2])), (sim.sweep_failures, dict(domains="node")),
                     (sim.sweep_apps, dict(new_node=types[0], counts=[0, 1]))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x = call(cluster, apps, engine=eng(), headroom=refs, node_table=True, **kw)
            y = call(cluster, apps, engine=eng(), headroom=refs, node_table=True, storage=False, **kw)
        _same(x, y, ("unscheduled", "headroom", "headroom_exact", "node_table", "gpu_table", "storage_table"))
        assert y.storage_table is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = sim.sweep_mix(cluster, apps, types, [[0, 1], [0, 1]], engine=eng(), headroom=refs, node_table=True)
        y = sim.sweep_mix(cluster, apps, types, [[0, 1], [0, 1]], engine=eng(), headroom=refs, node_table=True, storage=False)
    _same(x, y, ("unscheduled", "headroom", "headroom_exact", "node_table", "gpu_table", "storage_table"))


@pytest.mark.parametrize("which", ["mix", "failures", "apps"])
def test_the_other_sweeps_with_storage_on_engines_with_and_without_the_calls(which):
    cluster, apps, types, refs = _example()
    call, kw, warn = {"mix": (sim.sweep_mix, dict(new_nodes=types, counts=[[0, 1], [0, 2]]), sim.MixFallbackWarning),
                      "failures": (sim.sweep_failures, dict(domains="node"), sim.FailureFallbackWarning),
                      "apps": (sim.sweep_apps, dict(new_node=types[0], counts=[0, 2]), sim.AppFallbackWarning)}[which]
    out = []
    for eng in (LU.LocalUsageOracleEngine(), LU.GpuUsageOnlyEngine()):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out.append((call(cluster, apps, engine=eng, headroom=refs, node_table=True, storage=True, **kw), list(rec)))
    (a, wa), (b, wb) = out
    _same(a, b)
    if getattr(a, "batched", True):                                    # one engine batch: the engine without the calls falls back on the host, visibly
        assert not _warned(wa, warn) and _warned(wb, warn) and "supports_local_usage" in str(_warned(wb, warn)[0].message)
    else:                                                               # the scenarios ran one by one on both: the road's own warning
        assert [w for w in wa if issubclass(w.category, warn)] and [w for w in wb if issubclass(w.category, warn)]
    assert a.headroom_exact[0] and a.storage_table is not None
    flat_tabs = a.storage_table if which != "apps" else [t for row in a.storage_table for t in row]
    assert all(t for t in flat_tabs) and len(a.storage_table) == len(a.headroom) == len(a.node_table)          # one table per scenario


def test_storage_table_rows_of_the_open_local_example():
    cluster, apps, types, refs = _example()
    eng = LU.LocalUsageOracleEngine()
    res = sim.sweep(cluster, apps, types[0], [0, 3], engine=eng, storage=True)
    batch = sim.sweep_batch(cluster, apps, types[0], [0, 3])
    prob = batch.flat.problem
    ref = O.run(prob, batch.scen, batch.orders)
    for s, rows in enumerate(res.storage_table):
        n = int(batch.scen[s, 0])
        names = [nd["metadata"]["name"] for nd in batch.pool[:n] if (nd["metadata"].get("annotations") or {}).get("simon/node-local-storage")]
        assert [r["node"] for r in rows if r == next(x for x in rows if x["node"] == r["node"])] == names, "annotated nodes, pool order"
        vg_rows = [r for r in rows if r["kind"] == "VG"]
        dev_rows = [r for r in rows if r["kind"] != "VG"]
        assert sum(r["requests"] for r in vg_rows) == int(ref.used_vg[s])
        for r in vg_rows:
            assert set(r) == {"node", "kind", "name", "allocatable", "requests", "pct"}
            assert r["pct"] == int(float(r["requests"]) / float(r["allocatable"]) * 100) and r["name"] in batch.flat.info["vg_names"]
        for r in dev_rows:
            assert set(r) == {"node", "kind", "name", "allocatable", "used"} and r["kind"] in ("Device(ssd)", "Device(hdd)") and r["name"].startswith("/dev/")
            assert isinstance(r["used"], bool)
        # as many devices in use as device pods were placed, on top of the annotation's own state
        j_of = {nd["metadata"]["name"]: j for j, nd in enumerate(batch.pool)}
        init = sum(bin(int(prob.init_dev_alloc[j_of[nm]])).count("1") for nm in names)
        placed = sum(1 for p in range(prob.n_pods) if ref.placement[s, p] >= 0 and LU.spec_of_pod(prob, p) is not None
                     and int(LU.spec_of_pod(prob, p)["n_ssd"]) + int(LU.spec_of_pod(prob, p)["n_hdd"]) > 0
                     and (prob.preset_node is None or prob.preset_node[p] < 0))
        assert sum(r["used"] for r in dev_rows) == init + placed and placed > 0
    assert any(r["pct"] > 0 for r in res.storage_table[1] if r["kind"] == "VG")

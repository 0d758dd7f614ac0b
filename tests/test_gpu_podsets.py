"""Pod-subset batches on the device (simon_set_scenario_pods, simon_fetch_group_counts): every kernel route against the unmodified CPU oracle
on each scenario's OWN problem (podset_util: absent pods deleted, order compacted), pod by pod; absent pods on the edges of the 64-step
chunks and of the 32-pod presence words; composition with node subsets, eviction and segments; the replays; group counts against numpy;
preempt-risk flags; refusals and the state machine; sweep_apps end to end.  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest

import evict_util as EU
import mix_util as MU
import podset_util as PU
import randprob
import subset_util as SU
from open_simulator_amd import capi, simulate as sim, workloads as wl
from test_gpu_evict import ROUTES

pytestmark = pytest.mark.gpu


def _run(prob, scen, orders, rows, want_gpu=False, nodes=None, evict=None, segments=None, ranks=None, rows_first=True):
    """The batch with pod rows `rows` (None: none loaded).  nodes = (mask, zone): a node-subset batch; segments = (starts, counts); the
    pod rows are set before the node call (rows_first) or after it."""
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        if evict is not None:
            ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        if rows is not None and rows_first:
            ctx.set_scenario_pods(rows)
        if nodes is not None:
            ctx.set_scenario_nodes(*nodes)
        if segments is not None:
            ctx.set_scenario_segments(*segments)
        if ranks is not None:
            ctx.set_node_ranks(ranks)
        if rows is not None and not rows_first:
            ctx.set_scenario_pods(rows)
        ctx.run_loaded(rows is None, want_gpu)                         # (with rows the placement matrix is stored whatever the flag says)
        res = ctx.fetch(True, want_gpu)
        if prob.priority is not None:
            res.preempt_risk = ctx.fetch_preempt_risk()
        return res, ctx.stats()


def _assert_conditions(want):
    """By the oracle alone, before the device runs: absence lets a pod in that the all-present scenario leaves out, and moves a present pod."""
    a, b = PU.conditions(want[0], want[1:])
    assert a, "no scenario places a pod that the all-present scenario leaves unscheduled"
    assert b, "no present pod lands on another node than in the all-present scenario"


def _all_present_equals_no_rows(prob, scen, orders, res, want_gpu=False, **kw):
    plain, _ = _run(prob, scen[:1], orders, None, want_gpu, **kw)
    assert (plain.placement[0] == res.placement[0]).all()
    assert (int(plain.unscheduled[0]), int(plain.used_cpu[0]), int(plain.used_mem[0])) == (int(res.unscheduled[0]), int(res.used_cpu[0]), int(res.used_mem[0]))
    if want_gpu:
        assert (plain.gpu_slices[0] == res.gpu_slices[0]).all()


# ---- every route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,env,gen,wg", ROUTES, ids=[r[0] for r in ROUTES])
def test_absent_pods_match_the_oracle_on_every_score_table_route(case, env, gen, wg, monkeypatch):
    """podset_util.route_case: eight prefix scenarios over both orders -- all pods, no pods, only stream position 0, all but the last, one
    whole pod class absent, three random rows at density 0.5 (the last two on a few nodes more: gated pods come and go with the rows).
    Absent pods include preset pods and gated pods, a REST pod in `anti`, soft-spread pods in `service_*`, GPU pods in `gpu_*`."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, scen, orders, rows, want = PU.route_case(case)
    _assert_conditions(want)
    want_gpu = prob.gpu_mem is not None
    gone = ~rows[1:].all(0)
    assert (np.asarray(prob.preset_node)[gone] >= 0).any()
    if prob.gate_node is not None and (np.asarray(prob.gate_node) >= 0).any():
        assert (np.asarray(prob.gate_node)[gone] >= 0).any()
    cls = np.asarray(prob.pod_class)
    if case == "anti":
        assert any(prob.anti_off[c + 1] > prob.anti_off[c] for c in cls[~rows[5]])
    if case.startswith("service"):
        assert any(prob.spread_soft_off[c + 1] > prob.spread_soft_off[c] for c in cls[~rows[5]])
    res, st = _run(prob, scen, orders, rows, want_gpu)
    assert (st.kernel_variant, st.kernel_generation, st.workgroup_size) == (capi.KERNEL_NARROW_CACHE, gen, wg)
    PU.compare(res, want, want_gpu)
    _all_present_equals_no_rows(prob, scen, orders, res, want_gpu)


@functools.lru_cache(maxsize=None)
def _plain_case(pins):
    """A problem the register-resident kernels take (cpu + memory only, gates, presets on nodes 0 and 1); pins: with pinned pods, for the
    all-feature kernel."""
    prob = randprob.rand_problem(41, N=70, P=200, gates=True, nz_differs=True, pins=pins)
    P = prob.n_pods
    ok = EU.eligible(prob)
    pre = np.full(P, -1, np.int32)
    pre[ok[:4]] = [0, 1, 0, 1]
    prob = EU.replaced(prob, preset_node=pre)
    orders = np.stack([np.arange(P), np.random.default_rng(41).permutation(P)]).astype(np.int32)
    return PU.search_case(prob, orders, 41)


@pytest.mark.parametrize("name,env,variant", [("narrow", {"SIMON_NARROW_V1": "1", "SIMON_NO_CACHE": "1"}, capi.KERNEL_NARROW),
                                              ("fast", {"SIMON_NO_CACHE": "1"}, capi.KERNEL_NARROW_FAST),
                                              ("wide", {"SIMON_FORCE_WIDE": "1"}, capi.KERNEL_WIDE)])
def test_absent_pods_on_the_register_kernels_and_the_all_feature_kernel(name, env, variant, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, scen, orders, rows, want = _plain_case(name == "wide")
    _assert_conditions(want)
    gone = ~rows[1:].all(0)
    assert (np.asarray(prob.preset_node)[gone] >= 0).any() and (np.asarray(prob.gate_node)[gone] >= 0).any()
    if name == "wide":
        assert (np.asarray(prob.pin_node)[gone] >= 0).any()
    res, st = _run(prob, scen, orders, rows)
    assert st.kernel_variant == variant
    PU.compare(res, want)
    _all_present_equals_no_rows(prob, scen, orders, res)


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_case(N, P, many=False):
    """Absent pods at stream positions 0, 63, 64 and P - 1 (those below P) under the identity, a reversed and a shuffled order -- the table
    kernel sees positions through order[] -- and absent pod IDS 31, 32, 33 for the word edges; pinned, gated and preset pods among them.
    many: every pod its own request signature (more than 128: the MANY instantiations).  The first of a few seeded problems in which
    absence changes what the other pods get (podset_util.search_case) is the case."""
    for k in range(8):
        try:
            return _edge_problem(N, P, many, 100 * N + P + 1000 * k)
        except AssertionError:
            continue
    raise AssertionError(f"N={N} P={P}: no seeded problem in which absence changes what the other pods get")


def _edge_problem(N, P, many, seed):
    prob = randprob.rand_problem(seed, N=N, P=P, n_node_classes=min(5, N), nz_differs=True, gates=True, pins=True)
    ok = EU.eligible(prob)
    pre = np.full(P, -1, np.int32)
    pre[ok[:4]] = [0, 1, 0, 1]
    changes = dict(preset_node=pre)
    if many:
        changes["req_cpu"] = (100 + 10 * np.arange(P)).astype(np.int64)
        changes["nz_cpu"] = (100 + 10 * np.arange(P)).astype(np.int64)
    prob = EU.replaced(prob, **changes)
    rng = np.random.default_rng(N + P)
    orders = np.stack([np.arange(P), np.arange(P)[::-1], rng.permutation(P)]).astype(np.int32)
    pos = [q for q in (0, 63, 64, P - 1) if q < P]
    ids = [p for p in (31, 32, 33) if p < P]

    def rows_of(scen):
        rows = np.ones((8, P), bool)
        for s in (1, 2, 3):
            rows[s, orders[scen[s, 1]][pos]] = False
        rows[4, ids] = False
        rows[5, ids] = False
        rows[5, orders[scen[5, 1]][pos]] = False
        rows[6] = rng.random(P) < 0.5
        rows[7] = rng.random(P) < 0.5
        return rows
    return PU.search_case(prob, orders, N + P, rows_of=rows_of, order_of=[0, 0, 1, 2, 0, 2, 1, 2], more=0)


@pytest.mark.parametrize("P", [31, 32, 33, 65, 130])
@pytest.mark.parametrize("N", [24, 65])
def test_absent_pods_on_chunk_and_word_edges(N, P):
    prob, scen, orders, rows, want = _edge_case(N, P)
    _assert_conditions(want)
    res, st = _run(prob, scen, orders, rows)
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE
    PU.compare(res, want)
    _all_present_equals_no_rows(prob, scen, orders, res)


@pytest.mark.parametrize("P", [129, 193])
def test_absent_pods_with_more_than_128_signatures(P, monkeypatch, capfd):
    """The MANY instantiations: the library's own route line (SIMON_DEBUG_ROUTE) must show more than 128 signatures on the two-level layout,
    which is what selects them (simon_table.hip: MANY = KQ 2, COARSE)."""
    import re
    prob, scen, orders, rows, want = _edge_case(40, P, many=True)
    assert len({(int(prob.req_cpu[p]), int(prob.req_mem[p]), int(prob.pod_class[p])) for p in range(P)}) > 128
    _assert_conditions(want)
    monkeypatch.setenv("SIMON_DEBUG_ROUTE", "1")
    monkeypatch.setenv("SIMON_LDS_WS", "0")                           # (the workspace in HBM, as the chunk tests of the MANY route run it)
    capfd.readouterr()
    res, st = _run(prob, scen, orders, rows)
    route = re.findall(r"\[route\] variant \d+ .*? coarse (\d+) n_sigs (\d+)", capfd.readouterr().err)
    assert route and all(int(c) == 1 and int(k) > 128 for c, k in route), route
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation == 5
    PU.compare(res, want)
    _all_present_equals_no_rows(prob, scen, orders, res)


# ---- composition with the node dimension ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _subset_case():
    """A node-subset batch over three zones with flagged pods (evict_util.route_case): scenario 0 every node and every pod; the others on
    the node rows that lose flagged nodes.  The pod that fits nowhere once evicted is absent in scenario 3 and evicted in scenario 2."""
    prob, evict, mask, zone, scen, orders, ranks, _ = EU.route_case("gates_fine")
    pick = [2, 2, 2, 2, 1, 4, 5, 2]                                   # (row 2 loses all three flagged nodes)
    mask, scen, ranks = mask[pick], scen[pick], ranks[pick]
    P = prob.n_pods
    huge = int(np.flatnonzero(evict)[np.argmax(np.asarray(prob.req_cpu)[evict])])
    rows = PU.standard_rows(prob, orders, scen, seed=3)
    rows[0] = True
    rows[1] = np.random.default_rng(4).random(P) < 0.5
    rows[2] = True
    rows[2, np.flatnonzero(~evict)[::3]] = False
    rows[2, huge] = True
    rows[3, huge] = False
    want = [PU.oracle_nodes(prob, rows[s], mask[s], orders[scen[s, 1]], ranks[s], evict) for s in range(8)]
    return prob, evict, mask, zone, scen, orders, ranks, rows, want, huge


def test_pod_rows_compose_with_node_subsets_and_eviction():
    prob, evict, mask, zone, scen, orders, ranks, rows, want, huge = _subset_case()
    _assert_conditions(want)
    assert want[2].placement[huge] == capi.UNSCHEDULED and want[3].placement[huge] == capi.GATED and not mask[2][prob.preset_node[huge]]
    assert want[0].placement[huge] == capi.UNSCHEDULED              # (evicted there too: the all-present scenario of this node row)
    before, st = _run(prob, scen, orders, rows, nodes=(mask, zone), evict=evict, rows_first=True)
    after, _ = _run(prob, scen, orders, rows, nodes=(mask, zone), evict=evict, rows_first=False)
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE
    PU.compare(before, want)
    PU.compare(after, want)
    for s in range(8):
        got = before.placement[s]
        assert mask[s][got[got >= 0]].all(), s
    _all_present_equals_no_rows(prob, scen, orders, before, nodes=(mask[:1], zone), evict=evict)
    # the replay of the own-nodes batch, each scenario with its pod row
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        ctx.set_scenario_pods(rows)
        listed = [0, 2, 3, 1, 7]
        eb = ctx.explain_own_batch(listed, 64, 32, rows=True)
    seen = 0
    for k, s in enumerate(listed):
        nf, failed, codes = PU.explain_nodes(prob, rows[s], mask[s], orders[scen[s, 1]], ranks[s], evict)
        assert int(eb.n_failed[k]) == nf == want[s].unscheduled, s
        assert eb.failed_pods[k, :nf].tolist() == failed.tolist(), s
        for i in range(nf):
            assert eb.rows[k, i].tolist() == codes[i].tolist(), (s, i)
            assert eb.pod_bins(k, i) == PU.bins_of(codes[i]), (s, i)
        seen += nf
    assert seen > 0


def test_pod_rows_compose_with_two_segments():
    prob, orders = EU.route_problem("gates_fine")
    N, P = prob.n_nodes, prob.n_pods
    best = None
    for F in (10, 6, 4, 2):                                           # fewer fixed nodes until the all-present scenario leaves pods out
        starts = np.array([F, F + 12], np.int32)
        counts = np.array([[2, 1], [2, 1], [0, 3], [5, 0], [1, 1], [3, 2], [2, 1], [0, 0]], np.int32)
        scen = np.stack([F + counts.sum(1), np.arange(8) % len(orders)], 1).astype(np.int32)
        rows = PU.standard_rows(prob, orders, scen, seed=9)
        rows[6] = np.random.default_rng(10).random(P) < 0.5           # (same nodes as scenario 0, half the pods)
        present = [MU.present_mask(N, starts, counts[s]) for s in range(8)]
        want = [PU.oracle_nodes(prob, rows[s], present[s], orders[scen[s, 1]]) for s in range(8)]
        if all(PU.conditions(want[0], want[1:])):
            best = (starts, counts, scen, rows, want)
            break
    assert best is not None, "no split at which absence changes what the other pods get"
    starts, counts, scen, rows, want = best
    # (the segments are [F, F + 12) and [F + 12, N))
    assert counts[:, 0].max() <= 12 and counts[:, 1].max() <= N - starts[1]
    before, st = _run(prob, scen, orders, rows, segments=(starts, counts), rows_first=True)
    after, _ = _run(prob, scen, orders, rows, segments=(starts, counts), rows_first=False)
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE
    PU.compare(before, want)
    PU.compare(after, want)
    _all_present_equals_no_rows(prob, scen, orders, before, segments=(starts, counts[:1]))


def test_explain_batch_replays_a_prefix_scenario_with_its_row():
    prob, scen, orders, rows, want = PU.route_case("gates_fine")
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_pods(rows)
        listed = [0, 3, 4, 1, 6]
        eb = ctx.explain_batch(listed, 64, 32, rows=True)
        one = ctx.explain_loaded(3, 64)
        with pytest.raises(capi.SimonError, match="pod rows are loaded") as e:
            ctx.explain(int(scen[0, 0]), orders[0], 8)
        assert e.value.code == capi.ESTATE
    seen = 0
    for k, s in enumerate(listed):
        n = int(scen[s, 0])
        nf, failed, codes = PU.explain_prefix(prob, rows[s], n, orders[scen[s, 1]])
        assert int(eb.n_failed[k]) == nf == want[s].unscheduled, s
        assert eb.failed_pods[k, :nf].tolist() == failed.tolist(), s
        for i in range(nf):
            assert eb.rows[k, i, :n].tolist() == codes[i].tolist(), (s, i)
            assert eb.pod_bins(k, i) == PU.bins_of(codes[i]), (s, i)
        seen += nf
    assert seen > 0
    nf, failed, codes = PU.explain_prefix(prob, rows[3], int(scen[3, 0]), orders[scen[3, 1]])
    assert one[0] == nf and one[1].tolist() == failed.tolist() and (one[2] == codes).all()


# ---- group counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 7, 1024])
def test_group_counts_equal_numpy_on_the_fetched_placements(G):
    prob, scen, orders, rows, want = PU.route_case("gates_fine")
    P = prob.n_pods
    group = np.random.default_rng(G).integers(-1, G, P).astype(np.int32)
    group[:3] = [-1, G - 1, 0]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_pods(rows)
        ctx.run_loaded(False)
        res = ctx.fetch(True)
        uns, placed = ctx.fetch_group_counts(group, G, placed=True)
        only = ctx.fetch_group_counts(group, G)                       # placed == NULL
    PU.compare(res, want)
    ref_uns, ref_placed = PU.group_counts(res.placement, group, G)
    assert (res.placement == capi.GATED).any() and ref_uns.sum() > 0 and ref_placed.sum() > 0
    assert (uns == ref_uns).all() and (placed == ref_placed).all() and (only == ref_uns).all()
    assert uns.shape == (len(scen), G) and (uns[1] == 0).all() and (placed[1] == 0).all()      # the scenario of no pods


# ---- priorities ----------------------------------------------------------------------------------------------------------------------
def test_preempt_risk_with_rows_loaded():
    prob, scen, orders, rows, _ = PU.route_case("gates_fine")
    P = prob.n_pods
    prio = np.random.default_rng(5).integers(0, 3, P).astype(np.int32)
    prob = EU.replaced(prob, priority=prio)
    want = [PU.oracle_prefix(prob, rows[s], int(scen[s, 0]), orders[scen[s, 1]]) for s in range(8)]
    risk = [w.preempt_risk for w in want]
    assert 0 in risk and 1 in risk                                    # the flag set and unset, by the oracle alone
    res, _ = _run(prob, scen, orders, rows)
    PU.compare(res, want)
    assert res.preempt_risk.tolist() == risk


# ---- state and refusals --------------------------------------------------------------------------------------------------------------
def _expect(rc, code, ctx, match):
    assert rc == code, (rc, ctx.lib.simon_last_error(ctx.h))
    assert match in ctx.lib.simon_last_error(ctx.h).decode()


def test_refusals_and_the_state_machine():
    prob, scen, orders, rows, want = PU.route_case("gates_fine")
    P, S = prob.n_pods, len(scen)
    assert P % 32 != 0
    C = capi.C
    words = capi.presence_words(rows)
    u32 = lambda a: capi._ptr(np.ascontiguousarray(a, np.uint32), C.c_uint32)     # noqa: E731
    i32 = lambda a: capi._ptr(np.ascontiguousarray(a, np.int32), C.c_int32)       # noqa: E731
    group = (np.arange(P) % 7).astype(np.int32)
    out = np.zeros((S, 1025), np.int32)
    with capi.Context(0) as ctx:
        # before anything is loaded
        _expect(ctx.lib.simon_set_scenario_pods(ctx.h, u32(words)), capi.ESTATE, ctx, "load scenarios first")
        ctx.load_problem(prob)
        _expect(ctx.lib.simon_set_scenario_pods(ctx.h, u32(words)), capi.ESTATE, ctx, "load scenarios first")
        _expect(ctx.lib.simon_fetch_group_counts(ctx.h, i32(group), 7, i32(out), None), capi.ESTATE, ctx, "no placements")
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_pods(rows)

        def still_runs():
            ctx.run_loaded(True)
            PU.compare(ctx.fetch(True), want)

        still_runs()
        bad = words.copy()
        bad[2, -1] |= np.uint32(1 << (P % 32))                        # the bit at P
        assert PU.podset_errors(P, S, bad) == ["bit beyond P"]
        _expect(ctx.lib.simon_set_scenario_pods(ctx.h, u32(bad)), capi.EINVAL, ctx, f"sets bit {P}")
        still_runs()                                                  # the failed call left the rows as they were
        for G, g, what in ((0, group, "groups outside"), (1025, group, "groups outside"), (6, group, "has group 6")):
            assert PU.group_errors(P, g, G)
            _expect(ctx.lib.simon_fetch_group_counts(ctx.h, i32(g), G, i32(out), None), capi.EINVAL, ctx, what)
            still_runs()
        with pytest.raises(capi.SimonError, match="pod rows are loaded") as e:
            ctx.explain(int(scen[0, 0]), orders[0], 8)
        assert e.value.code == capi.ESTATE
        still_runs()
        # a run with rows loaded stores the placement matrix whatever want_placement says; without rows it does not
        ctx.run_loaded(False)
        PU.compare(ctx.fetch(True), want)
        # NULL detaches: every scenario holds every pod again
        ctx.set_scenario_pods(None)
        ctx.run_loaded(False)
        _expect(ctx.lib.simon_fetch_group_counts(ctx.h, i32(group), 7, i32(out), None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(True)
        detached = ctx.fetch(True)
        full = [PU.oracle_prefix(prob, np.ones(P, bool), int(scen[s, 0]), orders[scen[s, 1]]) for s in range(S)]
        PU.compare(detached, full)
        nf, _, _ = ctx.explain(int(scen[0, 0]), orders[0], 8)         # ... and the ad-hoc replay is allowed again
        assert nf == full[0].unscheduled
        # simon_load_scenarios clears the rows
        ctx.set_scenario_pods(rows)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True)
        PU.compare(ctx.fetch(True), full)
        # the rows survive the node calls: ranks on and off
        ctx.set_scenario_pods(words)                                  # (packed words are taken as they are)
        ctx.set_node_ranks(np.tile(np.arange(prob.n_nodes, dtype=np.int32), (S, 1)))
        still_runs()
        ctx.set_node_ranks(None)
        still_runs()
        with pytest.raises(ValueError, match="shape"):
            ctx.set_scenario_pods(np.ones((S, P + 1), bool))
        with pytest.raises(ValueError, match="pod rows for"):
            ctx.set_scenario_pods(np.ones((S + 1, P), bool))


# ---- sweep_apps end to end -----------------------------------------------------------------------------------------------------------
def _deployment(name, replicas, cpu, mem):
    return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": name, "namespace": "default"},
            "spec": {"replicas": replicas, "selector": {"matchLabels": {"app": name}},
                     "template": {"metadata": {"labels": {"app": name}},
                                  "spec": {"containers": [{"name": "c", "image": name, "resources": {"requests": {"cpu": cpu, "memory": mem}}}]}}}}


def test_sweep_apps_on_the_device_equals_simulate_per_scenario():
    cluster, _, types = MU.example_simple()
    nodes = list(cluster["Node"])[:2]
    names = {n["metadata"]["name"] for n in nodes}
    cluster = dict(cluster, Node=nodes, Pod=[p for p in cluster.get("Pod", []) if (p.get("spec") or {}).get("nodeName") in names | {None}])
    apps = [sim.AppResource("web", {"Deployment": [_deployment("web", 6, "2", "2Gi")]}),
            sim.AppResource("batch", {"Deployment": [_deployment("batch", 4, "4", "8Gi")]}),
            sim.AppResource("cache", {"Deployment": [_deployment("cache", 3, "1", "16Gi")]})]
    counts = (0, 2)
    eng = sim.HipEngine()
    res = sim.sweep_apps(cluster, apps, new_node=types[0], counts=counts, engine=eng, reasons=True)
    assert res.batched and res.fallback is None and len(res.subsets) == 8
    ok = []
    for u, sub in enumerate(res.subsets):
        fit = []
        for k, c in enumerate(counts):
            one = sim.simulate(cluster, [apps[a] for a in sub], engine=eng, new_nodes=wl.new_fake_nodes(types[0], c) if c else ())
            mine = [(e["pod"]["metadata"]["name"], e["reason"]) for e in res.unscheduled_pods[u][k]]
            assert mine == [(e["pod"]["metadata"]["name"], e["reason"]) for e in one.unscheduled_pods], (u, k)
            assert res.unscheduled[u][k] == len(one.unscheduled_pods) and sum(res.unscheduled_by_app[u][k]) == len(one.unscheduled_pods)
            assert all(res.unscheduled_by_app[u][k][a] == 0 for a in range(3) if a not in sub)
            if not one.unscheduled_pods:
                fit.append(c)
        assert res.min_count[u] == (min(fit) if fit else None), u
        if fit and fit[0] == 0:
            ok.append(u)
    assert ok and len(ok) < 8 and any(res.unscheduled_pods[u][0] for u in range(8))
    lens = [6, 4, 3]
    assert res.best == max(ok, key=lambda u: (sum(lens[a] for a in res.subsets[u]), -u))
    sets = [frozenset(s) for s in res.subsets]
    assert res.maximal == [u for u in ok if not any(sets[u] < sets[v] for v in ok)]

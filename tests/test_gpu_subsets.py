"""Node-subset batches on the device (simon_set_scenario_nodes): the staging kernel against its yardsticks without any scheduling run;
presence rows that spell segment prefixes, bit-identical to simon_set_scenario_segments on every score-table route; arbitrary subsets
against the CPU oracle pod by pod; preset pods gated on their own node; the plan's caps over each scenario's own nodes; refusals and the
setter's state machine; sweep_failures on the reference's example clusters.  Run with -m gpu on an MI355X."""
import dataclasses

import numpy as np
import pytest

import mix_util as MU
import randprob
import subset_util as SU
from open_simulator_amd import capi, k8s, simulate as sim
from test_gpu_mix import ROUTES, _route_case

pytestmark = pytest.mark.gpu

STAGES = ("device", "host")


def _ctx(monkeypatch, stage):
    """A context whose node-subset staging runs on `stage` (the knob is read once, when the context is made)."""
    if stage == "host":
        monkeypatch.setenv("SIMON_SUBSET_STAGE", "host")
    else:
        monkeypatch.delenv("SIMON_SUBSET_STAGE", raising=False)
    return capi.Context(0)


def _scen_of(mask, order_ids=None):
    mask = np.asarray(mask, bool)
    return np.stack([mask.sum(1), np.zeros(len(mask), np.int64) if order_ids is None else order_ids], 1).astype(np.int32)


# ---- 1. the staging against its yardsticks: no scheduling kernel runs -----------------------------------------------------------------
@pytest.mark.parametrize("Z", [1, 3, 64])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 131])
def test_staged_rank_rows_equal_the_node_tree_order_of_every_scenario(N, Z, monkeypatch):
    """simon_fetch_node_ranks after simon_set_scenario_nodes = simulate.mix_node_ranks of the same pool and presence rows (absent: N), on
    word boundaries (31 / 32 / 33 / 64 / 65 nodes), with one, three and 64 zones, staged by the device and by the host loops."""
    rng = np.random.default_rng(1000 * N + Z)
    prob, _ = MU.segmentable(randprob.rand_problem(N, N=N, P=12, n_node_classes=min(5, N)), fixed=0)
    zone = rng.integers(0, Z, N).astype(np.int32)
    pool = [{"metadata": {"name": f"n{j}", "labels": {k8s.LABEL_ZONE: f"z{zone[j]}"}}} for j in range(N)]
    mask = SU.staging_masks(N, zone, seed=N + Z)
    assert mask.shape == (12, N)
    want = sim.mix_node_ranks(pool, mask)
    want = np.where(want < 0, N, want)
    assert (want == np.where(SU.zone_ranks(mask, zone) < 0, N, SU.zone_ranks(mask, zone))).all()
    orders = np.arange(prob.n_pods, dtype=np.int32)[None]
    for stage in STAGES:
        with _ctx(monkeypatch, stage) as ctx:
            ctx.load_problem(prob)
            ctx.load_scenarios(_scen_of(mask), orders)
            with pytest.raises(capi.SimonError) as e:                 # a prefix batch has no rank rows
                ctx.fetch_node_ranks()
            assert e.value.code == capi.ESTATE
            ctx.set_scenario_nodes(mask, zone, n_zones=Z)
            got = ctx.fetch_node_ranks()
            assert got.tolist() == want.tolist(), stage
            if Z == 1:                                                # no zones given = one zone = pool order over the scenario
                ctx.set_scenario_nodes(mask)
                assert ctx.fetch_node_ranks().tolist() == want.tolist(), stage
                assert (want == np.where(mask, np.cumsum(mask, 1) - 1, N)).all()


# ---- 2. presence rows that spell segment prefixes: bit-identical to the segmented batch on every route ------------------------------------
def _same(a, b, gpu):
    assert (a.placement == b.placement).all() and a.unscheduled.tolist() == b.unscheduled.tolist()
    assert a.used_cpu.tolist() == b.used_cpu.tolist() and a.used_mem.tolist() == b.used_mem.tolist()
    if gpu:
        assert (a.gpu_slices == b.gpu_slices).all()


@pytest.mark.parametrize("case,env,gen,wg", ROUTES, ids=[r[0] for r in ROUTES])
def test_rows_that_spell_segments_equal_the_segmented_batch(case, env, gen, wg, monkeypatch):
    """One segment behind the batch's smallest size (the route case's own scenarios), then two and three segments with random counts:
    simon_set_scenario_segments and simon_set_scenario_nodes with the same node sets on ONE context give the same placements, counts,
    used resources and GPU slices, on the pinned route, whether the device or the host loops staged the subset arrays."""
    prob, scen, orders = _route_case(case)
    prob, F = MU.segmentable(prob, scen)
    N, want_gpu = prob.n_nodes, prob.gpu_mem is not None
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(len(case))
    batches = [(np.array([F], np.int32), (scen[:, :1] - F).astype(np.int32), scen)]
    for n_seg in (2, 3):
        starts = np.sort(np.concatenate([[F], rng.choice(np.arange(F + 1, N), n_seg - 1, replace=False)])).astype(np.int32)
        lens = np.append(starts[1:], N) - starts
        cnt = np.stack([rng.integers(0, n + 1, len(scen)) for n in lens], 1).astype(np.int32)
        batches.append((starts, cnt, np.stack([F + cnt.sum(1), scen[:, 1]], 1).astype(np.int32)))
    refs = []
    for stage in STAGES:
        with _ctx(monkeypatch, stage) as ctx:
            ctx.load_problem(prob)
            for b, (starts, cnt, sc) in enumerate(batches):
                mask = np.stack([MU.present_mask(N, starts, cnt[s]) for s in range(len(sc))])
                ctx.load_scenarios(sc, orders)
                if stage == STAGES[0]:
                    ctx.set_scenario_segments(starts, cnt)
                    seg_ranks = ctx.fetch_node_ranks()
                    ctx.run_loaded(True, want_gpu)
                    st = ctx.stats()
                    assert (st.kernel_variant, st.kernel_generation, st.workgroup_size) == (capi.KERNEL_NARROW_CACHE, gen, wg), (b, stage)
                    refs.append((ctx.fetch(True, want_gpu), seg_ranks))
                ctx.set_scenario_nodes(mask)
                assert (ctx.fetch_node_ranks() == refs[b][1]).all(), (b, stage)
                ctx.run_loaded(True, want_gpu)
                st = ctx.stats()
                assert (st.kernel_variant, st.kernel_generation, st.workgroup_size) == (capi.KERNEL_NARROW_CACHE, gen, wg), (b, stage)
                _same(ctx.fetch(True, want_gpu), refs[b][0], want_gpu)


# ---- 3. arbitrary subsets against the oracle ----------------------------------------------------------------------------------------------
def _random_rows(rng, N, S=8):
    """S seeded presence rows: one drops a single node, one keeps three nodes, the others keep 30 % ... 95 % of the pool."""
    mask = np.stack([rng.random(N) < p for p in np.linspace(0.3, 0.95, S)])
    mask[0] = True
    mask[0, int(rng.integers(0, N))] = False
    mask[1] = False
    mask[1, rng.choice(N, 3, replace=False)] = True
    assert mask.any(1).all()
    return mask


@pytest.mark.parametrize("case,env", [("gates", {}), ("gpu", {}), ("anti", {}), ("service_wave", {"SIMON_TEAM": "0"}), ("service_team", {"SIMON_TEAM": "1"})],
                         ids=["gates", "gpu", "anti", "service_wave", "service_team"])
def test_arbitrary_subsets_match_the_oracle_pod_by_pod(case, env, monkeypatch):
    """Seeded random node sets, each in the nodeTree order of its own nodes over three zones, against the oracle on the scenario's own
    node set (its nodes moved to the front of the same problem, in rank order); two of them also against the oracle on the scenario's
    nodes ALONE (restrict_nodes).  Every case has to run on the score-table kernel."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, _, orders = _route_case(case)
    prob, _ = MU.segmentable(prob, fixed=0)
    N, want_gpu = prob.n_nodes, prob.gpu_mem is not None
    rng = np.random.default_rng(sum(map(ord, case)))
    mask = _random_rows(rng, N)
    zone = (rng.integers(0, 3, N)).astype(np.int32)
    scen = _scen_of(mask, rng.integers(0, len(orders), len(mask)))
    ranks = SU.zone_ranks(mask, zone)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        assert (ctx.fetch_node_ranks() == np.where(ranks < 0, N, ranks)).all()
        ctx.run_loaded(True, want_gpu)
        res = ctx.fetch(True, want_gpu)
        st = ctx.stats()
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation >= 4
    for s in range(len(mask)):
        row, ref = MU.oracle_of_scenario(prob, mask[s], orders[scen[s, 1]], ranks[s])
        assert res.placement[s].tolist() == row.tolist(), s
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s
        if want_gpu:
            assert (res.gpu_slices[s] == ref.gpu_slices[0]).all(), s
        if s in (1, 5):
            other, _ = MU.oracle_of_restricted(prob, mask[s], orders[scen[s, 1]], ranks[s])
            assert other.tolist() == row.tolist(), s
        placed = res.placement[s][res.placement[s] >= 0]
        assert mask[s][placed].all()                                  # nobody lands on an absent node


# ---- 4. a preset pod gated on its own node ------------------------------------------------------------------------------------------------
def test_a_preset_pod_gated_on_its_own_node_vanishes_with_it_and_is_bound_where_it_stands():
    base, _, orders = _route_case("gates")
    assert base.preset_node is not None and (base.preset_node >= 0).any()
    prob, _ = MU.segmentable(base, fixed=0)                           # (clears the initial state and turns every preset into a plain gate)
    pre = np.asarray(base.preset_node)
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    kw["preset_node"] = pre.copy()
    kw["gate_node"] = np.where(pre >= 0, pre, prob.gate_node).astype(np.int32)   # ... and back: preset to, and gated on, the same node
    prob = capi.Problem(**kw).normalise()
    N = prob.n_nodes
    rng = np.random.default_rng(4)
    mask = _random_rows(rng, N)
    targets = np.unique(pre[pre >= 0])
    mask[2, targets[0]] = False                                       # some preset's node absent here, present there
    mask[3, targets[0]] = True
    scen = _scen_of(mask, rng.integers(0, len(orders), len(mask)))
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
    seen_gone = seen_bound = 0
    for s in range(len(mask)):
        row, ref = MU.oracle_of_scenario(prob, mask[s], orders[scen[s, 1]])
        assert res.placement[s].tolist() == row.tolist(), s
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s
        there = mask[s][np.maximum(pre, 0)]
        assert (res.placement[s][(pre >= 0) & ~there] == capi.GATED).all()
        assert (res.placement[s][(pre >= 0) & there] == pre[(pre >= 0) & there]).all()
        seen_gone += int(((pre >= 0) & ~there).sum())
        seen_bound += int(((pre >= 0) & there).sum())
    assert seen_gone > 0 and seen_bound > 0


# ---- 5. the plan's caps use each scenario's own totals ------------------------------------------------------------------------------------
def test_min_plan_caps_use_each_subset_s_own_nodes():
    prob, _, orders = _route_case("gates")
    prob, _ = MU.segmentable(prob, fixed=0)
    N = prob.n_nodes
    rng = np.random.default_rng(5)
    mask = np.concatenate([_random_rows(rng, N), _random_rows(rng, N)[2:]])
    scen = _scen_of(mask)
    a, m = prob.alloc_cpu.astype(np.int64), prob.alloc_mem.astype(np.int64)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        found = []
        for cap in (100, 60, 30, 10):
            plan, _ = ctx.min_plan_vg(cap, cap, 100)
            ok = [s for s in range(len(mask)) if not res.unscheduled[s] and sim.occupancy_pct(int(res.used_cpu[s]), int(a[mask[s]].sum())) <= cap
                  and sim.occupancy_pct(int(res.used_mem[s]) * 1000, int(m[mask[s]].sum()) * 1000) <= cap]
            best = min(ok, key=lambda s: (int(scen[s, 0]), s)) if ok else None
            assert (plan.found, plan.scenario if plan.found else -1) == ((1, best) if best is not None else (0, -1)), cap
            if best is not None:
                assert plan.cpu_pct == sim.occupancy_pct(int(res.used_cpu[best]), int(a[mask[best]].sum())), cap
            found.append(best is not None)
        assert True in found


# ---- 6. refusals, and what replaces what ----------------------------------------------------------------------------------------------------
def _expect(ctx, code, words, zone=None, n_zones=0, match=None):
    rc = ctx.lib.simon_set_scenario_nodes(ctx.h, capi._ptr(np.ascontiguousarray(words, np.uint32), capi.C.c_uint32),
                                          capi._ptr(None if zone is None else np.ascontiguousarray(zone, np.int32), capi.C.c_int32), n_zones)
    assert rc == code, (rc, ctx.lib.simon_last_error(ctx.h))
    if match:
        assert match in ctx.lib.simon_last_error(ctx.h).decode()


@pytest.mark.parametrize("stage", STAGES)
def test_refusals_leave_a_usable_prefix_batch(stage, monkeypatch):
    """Every SIMON_EINVAL of simon_set_scenario_nodes, with subset_util.subset_errors (the rules restated) naming the same rule; after
    each the batch runs as the prefix batch it was loaded as.  SIMON_ESTATE: nothing loaded, ImageLocality in effect."""
    import image_util
    base, scen, orders = _route_case("gates_fine")
    prob, _ = MU.segmentable(base, fixed=0)
    N, P = prob.n_nodes, prob.n_pods
    rng = np.random.default_rng(6)
    mask = np.stack([np.arange(N) < n for n in scen[:, 0]])           # the prefix scenarios as rows: valid as they stand
    mask[0] = rng.permutation(mask[0])                                # ... and one that is no prefix
    words = capi.presence_words(mask)
    zone = (np.arange(N) % 3).astype(np.int32)
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    lost = int(np.flatnonzero(~mask.all(0))[0])
    busy = np.zeros(N, np.int32)
    busy[lost] = 1
    pre, gate = np.full(P, -1, np.int32), np.full(P, -1, np.int32) if prob.gate_node is None else np.array(prob.gate_node)
    pre[3], gate[3] = lost, N - 1 if lost != N - 1 else 0
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ref = ctx.run_batch(scen, orders)
    with _ctx(monkeypatch, stage) as ctx:
        ctx.load_problem(prob)
        _expect(ctx, capi.ESTATE, words, match="load scenarios first")
        assert ctx.lib.simon_fetch_node_ranks(ctx.h, capi._ptr(np.zeros((len(scen), N), np.int32), capi.C.c_int32)) == capi.ESTATE
        ctx.load_scenarios(scen, orders)
        assert SU.subset_errors(prob, scen, words) == []
        bad = []
        assert N % 32
        w = words.copy()
        w[1, -1] |= np.uint32(1 << 31)                                # a node at or beyond N
        bad.append((w, scen, None, 0, "bits beyond N"))
        s2 = scen.copy()
        s2[2, 0] -= 1
        bad.append((words, s2, None, 0, "n_nodes mismatch"))
        w = words.copy()
        w[1] = 0
        s2 = scen.copy()
        s2[1, 0] = 0
        bad.append((w, s2, None, 0, "empty scenario"))
        bad.append((words, scen, zone, 2, "zone ids"))
        bad.append((words, scen, zone - 1, 3, "zone ids"))
        bad.append((words, scen, zone, 65, "n_zones"))
        bad.append((words, scen, zone, 0, "n_zones"))
        for w, sc, z, nz, rule in bad:
            assert SU.subset_errors(prob, sc, w, z, nz if z is not None else None) == [rule]
            ctx.load_scenarios(sc, orders)
            ctx.set_scenario_nodes(mask if sc is scen else None)      # a refusal abandons whatever was there
            _expect(ctx, capi.EINVAL, w, z, nz)
            with pytest.raises(capi.SimonError):
                ctx.fetch_node_ranks()
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        _expect(ctx, capi.EINVAL, words, zone, 2)
        ctx.run_loaded(True)                                          # ... and what is left is the prefix batch
        after = ctx.fetch(True)
        assert (after.placement == ref.placement).all() and after.unscheduled.tolist() == ref.unscheduled.tolist()
    for change, rule in ((dict(init_npods=busy), "init state"), (dict(preset_node=pre, gate_node=gate), "preset")):
        bad_prob = capi.Problem(**dict(kw, **change)).normalise()
        assert SU.subset_errors(bad_prob, scen, words) == [rule]
        with _ctx(monkeypatch, stage) as ctx:
            ctx.load_problem(bad_prob)
            ctx.load_scenarios(scen, orders)
            _expect(ctx, capi.EINVAL, words)
            ctx.run_loaded(True)
            assert ctx.stats().kernel_variant != 0
    cluster, apps, tmpl = image_util.image_sweep_case(3)
    b = sim.sweep_batch(cluster, apps, tmpl, [0, 1, 2], image_batch=True)
    assert b.flat.problem.image_locality is not None
    with _ctx(monkeypatch, stage) as ctx:
        ctx.load_problem(b.flat.problem)
        ctx.load_scenarios(b.scen, b.orders)
        with pytest.raises(capi.SimonError) as e:
            ctx.set_scenario_nodes(np.arange(len(b.pool))[None, :] < b.scen[:, :1])
        assert e.value.code == capi.ESTATE and "ImageLocality" in str(e.value)
        ctx.run_loaded(True)


def test_the_all_feature_kernel_and_explain_refuse_a_subset_batch(monkeypatch):
    prob, scen, orders = _route_case("gates_fine")
    prob, _ = MU.segmentable(prob, fixed=0)
    N = prob.n_nodes
    mask = np.stack([np.arange(N) < n for n in scen[:, 0]])
    mask[0] = np.random.default_rng(8).permutation(mask[0])
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask)
        ctx.run_loaded(True)
        for call in (lambda: ctx.explain_loaded(0), lambda: ctx.explain(int(scen[0, 0]), orders[0], 4), lambda: ctx.explain_batch([0, 1], 4, 8)):
            with pytest.raises(capi.SimonError) as e:
                call()
            assert e.value.code == capi.ESTATE and "node-subset batch" in str(e.value)
        ctx.set_scenario_nodes(None)
        ctx.explain_loaded(0)                                         # the prefix batch explains again
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask)
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE and "node-subset batch" in str(e.value)
        ctx.set_scenario_nodes(None)
        ctx.run_loaded(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_WIDE


def _assert_subsets(res, prob, scen, orders, mask, ranks=None):
    for s in range(len(scen)):
        row, ref = MU.oracle_of_scenario(prob, mask[s], orders[scen[s, 1]], None if ranks is None else ranks[s])
        assert res.placement[s].tolist() == row.tolist(), s
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s


@pytest.mark.parametrize("stage", STAGES)
def test_subsets_segments_ranks_and_batches_replace_each_other_on_one_context(stage, monkeypatch):
    """One context: subsets over three zones -> caller rank rows over the same sets -> simon_set_node_ranks(NULL) (the sets' own nodeTree
    order again) -> segments -> other subsets -> none (the prefix batch) -> a fresh prefix batch -> subsets again.  Every run with own node
    sets against the oracle, every prefix run against a fresh context."""
    monkeypatch.setenv("SIMON_TABLE_COARSE", "0")
    N, F, S = 150, 60, 6
    prob, _ = MU.segmentable(randprob.rand_problem(31, N=N, P=400, gates=True, pins=True, n_node_classes=9, n_pod_classes=8), fixed=0)
    rng = np.random.default_rng(7)
    orders = np.stack([np.arange(prob.n_pods), rng.permutation(prob.n_pods), rng.permutation(prob.n_pods)]).astype(np.int32)
    starts = np.array([F, 97, 131], np.int32)
    cnt = np.stack([rng.integers(0, n + 1, S) for n in (37, 34, 19)], 1).astype(np.int32)
    seg_mask = np.stack([MU.present_mask(N, starts, cnt[s]) for s in range(S)])
    scen = _scen_of(seg_mask, rng.integers(0, 3, S))
    mask_a = np.stack([rng.permutation(seg_mask[s]) for s in range(S)])         # other node sets of the same sizes
    mask_b = np.stack([rng.permutation(seg_mask[s]) for s in range(S)])
    zone = rng.integers(0, 3, N).astype(np.int32)
    caller = rng.integers(-3, N + 3, (S, N)).astype(np.int32)
    for s in range(S):
        own = np.flatnonzero(mask_a[s])
        caller[s, own] = rng.permutation(len(own))
    scen2 = np.array([[N, 0], [90, 2], [33, 1], [120, 1]], np.int32)

    def fresh(sc):
        with capi.Context(0) as c2:
            c2.load_problem(prob)
            return c2.run_batch(sc, orders)

    with _ctx(monkeypatch, stage) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)

        def run():
            ctx.run_loaded(True)
            st = ctx.stats()
            assert (st.kernel_variant, st.kernel_generation) == (capi.KERNEL_NARROW_CACHE, 4)
            return ctx.fetch(True)

        ctx.set_scenario_nodes(mask_a, zone)
        own_a = run()
        _assert_subsets(own_a, prob, scen, orders, mask_a, SU.zone_ranks(mask_a, zone))
        ctx.set_node_ranks(caller)
        _assert_subsets(run(), prob, scen, orders, mask_a, caller)
        ctx.set_node_ranks(None)
        assert (ctx.fetch_node_ranks() == np.where(mask_a, SU.zone_ranks(mask_a, zone), N)).all()
        _same(run(), own_a, False)
        ctx.set_scenario_segments(starts, cnt)
        _assert_subsets(run(), prob, scen, orders, seg_mask)
        ctx.set_scenario_nodes(mask_b)
        _assert_subsets(run(), prob, scen, orders, mask_b)
        ctx.set_scenario_nodes(None)
        _same(run(), fresh(scen), False)
        ctx.load_scenarios(scen2, orders)
        _same(run(), fresh(scen2), False)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask_a, zone)
        _same(run(), own_a, False)
        ctx.set_scenario_segments(None, None)                         # segments' own way back to prefix scenarios clears subsets too
        _same(run(), fresh(scen), False)


# ---- 7. sweep_failures on the device ---------------------------------------------------------------------------------------------------------
def _no_app_daemonset(cluster, apps):
    return cluster, [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]


EXAMPLES = {"simple_no_ds": lambda: _no_app_daemonset(*MU.example_simple()[:2]), "gpushare": lambda: MU.example_gpushare()[:2],
            "zoned": lambda: MU.random_zoned(11, n_nodes=14)[:2]}


@pytest.mark.parametrize("name", sorted(EXAMPLES))
def test_sweep_failures_on_the_device_equals_the_oracle_engine(name):
    cluster, apps = EXAMPLES[name]()
    eng = sim.HipEngine()
    hip = sim.sweep_failures(cluster, apps, "node", engine=eng, reasons=True)
    ref = sim.sweep_failures(cluster, apps, "node", engine=SU.SubsetOracleEngine(), reasons=True)
    assert hip.batched and ref.batched and hip.fallback is None
    assert eng.last_stats.kernel_variant == capi.KERNEL_NARROW_CACHE
    assert hip.placements == ref.placements and hip.domains == ref.domains
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.vg_pct, hip.survives, hip.needs_reference, hip.baseline, hip.critical) == \
           (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.vg_pct, ref.survives, ref.needs_reference, ref.baseline, ref.critical)
    names = lambda lists: [[(u["pod"]["metadata"]["name"], u["reason"]) for u in lst] for lst in lists]   # noqa: E731
    assert names(hip.unscheduled_pods) == names(ref.unscheduled_pods)
    answers = SU.reduced_answers(cluster, apps, hip.domains)
    assert [w for w, _ in answers] == hip.placements


@pytest.mark.parametrize("name", ["simple", "open_local"])
def test_examples_that_cannot_batch_fall_back_visibly_and_still_match(name):
    """example_simple's app holds a DaemonSet and the pod order without worker-1 is not the cluster's; Open-Local needs the all-feature
    kernel, which takes no node subsets.  sweep_failures warns, says why, runs every scenario as its own problem -- the oracle's answers."""
    cluster, apps, _ = {"simple": MU.example_simple, "open_local": MU.example_open_local}[name]()
    with pytest.warns(sim.FailureFallbackWarning, match="pod order" if name == "simple" else "refused"):
        hip = sim.sweep_failures(cluster, apps, "node", engine=sim.HipEngine())
    assert not hip.batched and ("DaemonSet" if name == "simple" else "node-subset batch") in hip.fallback
    with pytest.warns(sim.FailureFallbackWarning):
        ref = sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine())
    assert hip.placements == ref.placements
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.vg_pct, hip.baseline) == (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.vg_pct, ref.baseline)

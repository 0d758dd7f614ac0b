"""Node-type mixes on the device (simon_set_scenario_segments): one segment reproducing prefix sizes is bit-identical to the plain batch
on every score-table route; two and three segments match the CPU oracle on each mix's own problem, by object names; refusals leave a
usable context; a slice of the fuzz regime (fuzz_mix.py) with the route of every case pinned; the setter's state machine on one
context; degenerate segment shapes; 4 096 mixes in one launch; preempt-risk flags of a segmented batch.  Run with -m gpu on an MI355X."""
import itertools

import numpy as np
import pytest

import mix_util as MU
import oracle_lib as O
import randprob
from open_simulator_amd import capi, flatten as fl, simulate as sim, synth

pytestmark = pytest.mark.gpu

CASES = {"simple": MU.example_simple, "gpushare": MU.example_gpushare, "zoned": lambda: MU.random_zoned(11, n_nodes=14)}


def _pool_problem(cluster, apps, types, top):
    base = list(cluster.get("Node", []))
    pool = base + [n for nn in sim.mix_fake_nodes(types, top) for n in nn]
    pods, gates = sim.build_stream(cluster, apps, pool, len(base))
    flat = fl.flatten(pool, pods, cluster.get("Service", []), cluster.get("ReplicaSet", []), cluster.get("StatefulSet", []), gates,
                      storage_classes=sim._storage_classes(cluster, apps))
    return flat, pool, base


def _run(prob, scen, env, monkeypatch, segments=None, ranks=None, want_gpu=False):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, np.arange(prob.n_pods, dtype=np.int32)[None])
        if segments is not None:
            ctx.set_scenario_segments(*segments)
        if ranks is not None:
            ctx.set_node_ranks(ranks)
        ctx.run_loaded(True, want_gpu)
        res = ctx.fetch(True, want_gpu)
        return res, ctx.stats()


_segmentable = MU.segmentable


def _route_case(name):
    if name.startswith("config3"):
        return synth.config3(n_counts=8, n_orders=2, n_pods=600, n_het=40)
    if name == "classes160":
        return synth.config3_classes(160, n_counts=6, n_orders=2, n_pods=1500)
    if name.startswith("service"):
        prob, scen, orders = synth.config_service(n_counts=24, n_pods=1500, n_shapes=30)
        return prob, scen[[0, 5, 12, 20]], orders
    kw = {"gates": dict(gates=True, presets=True, init_state=True, nz_differs=True), "gpu": dict(gpu=True, gates=True, presets=True),
          "anti": dict(anti=True, gates=True)}[name.split("_")[0]]
    prob = randprob.rand_problem(17, N=48, P=240, **kw)
    scen, orders = randprob.rand_scenarios(17, prob, S=8, min_n=20)
    return prob, scen, orders


# (case, environment, generation, threads per scenario): every score-table route a segmented batch takes
ROUTES = [("config3_fine_hbm", {"SIMON_TABLE_COARSE": "0", "SIMON_LDS_WS": "0"}, 4, 64),
          ("config3_fine_lds", {"SIMON_TABLE_COARSE": "0", "SIMON_LDS_WS": "1"}, 4, 64),
          ("config3_coarse", {"SIMON_TABLE_COARSE": "1"}, 5, 64),
          ("classes160", {}, 4, 64),
          ("service_wave", {"SIMON_TEAM": "0"}, 7, 64),
          ("service_team", {"SIMON_TEAM": "1"}, 7, 256),
          ("gpu_fold", {}, 5, 64),
          ("gpu_lds", {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "1"}, 6, 64),
          ("gpu_hbm", {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "0"}, 6, 64),
          ("anti", {}, 6, 64),
          ("gates_fine", {"SIMON_TABLE_COARSE": "0"}, 4, 64),
          ("gates_coarse", {"SIMON_TABLE_COARSE": "1"}, 5, 64)]


@pytest.mark.parametrize("case,env,gen,wg", ROUTES, ids=[r[0] for r in ROUTES])
def test_one_segment_is_bit_identical_to_the_prefix_batch(case, env, gen, wg, monkeypatch):
    """Scenario sizes expressed as one segment behind the batch's smallest size: the same placements, counts, used resources and GPU
    slices as the plain (prefix) batch, on a pinned route.  Includes gated pods that are neither preset nor pinned, on fixed nodes and on
    segment nodes (the "gates" cases)."""
    prob, scen, orders = _route_case(case)
    prob, F = _segmentable(prob, scen)
    want_gpu = prob.gpu_mem is not None
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    runs = []
    for seg in (None, ([F], scen[:, :1] - F)):
        with capi.Context(0) as ctx:
            ctx.load_problem(prob)
            ctx.load_scenarios(scen, orders)
            if seg is not None:
                ctx.set_scenario_segments(*seg)
            ctx.run_loaded(True, want_gpu)
            runs.append((ctx.fetch(True, want_gpu), ctx.stats()))
    (plain, st0), (seg, st1) = runs
    assert (st1.kernel_variant, st1.kernel_generation, st1.workgroup_size) == (capi.KERNEL_NARROW_CACHE, gen, wg)
    assert (st0.kernel_variant, st0.kernel_generation) == (capi.KERNEL_NARROW_CACHE, gen)
    assert (seg.placement == plain.placement).all()
    assert seg.unscheduled.tolist() == plain.unscheduled.tolist()
    assert seg.used_cpu.tolist() == plain.used_cpu.tolist() and seg.used_mem.tolist() == plain.used_mem.tolist()
    if want_gpu:
        assert (seg.gpu_slices == plain.gpu_slices).all()


MULTI = [("gates", 2), ("gates", 3), ("gpu", 2), ("anti", 3)]


@pytest.mark.parametrize("case,n_seg", MULTI)
def test_random_segments_match_the_oracle_pod_by_pod(case, n_seg):
    """Two and three segments with random counts (node classes spanning segments) against the oracle on each scenario's own node set
    (its nodes moved to the front of the same problem: mix_util.permute_nodes), every pod."""
    prob, scen, orders = _route_case(case)
    prob, F = _segmentable(prob, scen)
    N = prob.n_nodes
    rng = np.random.default_rng(n_seg)
    starts = np.sort(np.concatenate([[F], rng.choice(np.arange(F + 1, N), n_seg - 1, replace=False)])).astype(np.int32)
    ends = np.append(starts[1:], N)
    S = 10
    cnt = np.stack([rng.integers(0, ends[g] - starts[g] + 1, S) for g in range(n_seg)], 1).astype(np.int32)
    sc = np.stack([F + cnt.sum(1), rng.integers(0, len(orders), S)], 1).astype(np.int32)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(sc, orders)
        ctx.set_scenario_segments(starts, cnt)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
    for s in range(S):
        present = np.zeros(N, bool)
        present[:F] = True
        for g in range(n_seg):
            present[starts[g]:starts[g] + cnt[s, g]] = True
        row, ref = MU.oracle_of_scenario(prob, present, orders[sc[s, 1]])
        assert res.placement[s].tolist() == row.tolist(), s
        assert int(res.unscheduled[s]) == int(ref.unscheduled[0])
        assert int(res.used_cpu[s]) == int(ref.used_cpu[0]) and int(res.used_mem[s]) == int(ref.used_mem[0])


class _Recording(sim.HipEngine):
    def run(self, prob, scen, orders, **kw):
        self.seen = (prob, scen, kw)
        self.out = super().run(prob, scen, orders, **kw)
        return self.out


@pytest.mark.parametrize("case,n_types", [("simple", 2), ("simple", 3), ("gpushare", 2), ("zoned", 2), ("zoned", 3)])
def test_segments_match_the_oracle_on_every_mix(case, n_types):
    cluster, apps, types = CASES[case]()
    while len(types) < n_types:
        types.append(MU.shaped(types[0], 2 + 2 * len(types), "4Gi", f"extra-{len(types)}"))
    rng = np.random.default_rng(n_types)
    grid = [sorted(set(rng.integers(0, 4, 3).tolist()) | {0}) for _ in range(n_types)]
    eng = _Recording()
    hip = sim.sweep_mix(cluster, apps, types, grid, engine=eng)
    ref = sim.sweep_mix(cluster, apps, types, grid, engine=MU.OracleEngine())
    assert hip.batched and not ref.batched
    assert eng.last_stats.kernel_generation >= 4
    assert hip.counts == ref.counts and hip.unscheduled == ref.unscheduled
    assert hip.cpu_pct == ref.cpu_pct and hip.mem_pct == ref.mem_pct and hip.vg_pct == ref.vg_pct
    assert hip.best == ref.best and hip.cost == ref.cost
    # pod by pod: every mix equals the oracle on the same pool problem with the mix's nodes moved to the front (in the mix's own
    # nodeTree order); the pods gated out are exactly those whose gate node the mix lacks
    top = [max(g) for g in grid]
    flat, pool, base = _pool_problem(cluster, apps, types, top)
    starts = np.cumsum([len(base)] + top[:-1])
    gate = np.asarray(flat.problem.gate_node) if flat.problem.gate_node is not None else np.full(flat.problem.n_pods, -1)
    for s, mix in enumerate(hip.counts):
        row = eng.out.placement[s]
        present = np.zeros(len(pool), bool)
        present[:len(base)] = True
        for g, st in enumerate(starts):
            present[st:st + mix[g]] = True
        assert ((row == capi.GATED) == ((gate >= 0) & ~present[np.maximum(gate, 0)])).all(), mix
        ranks = eng.seen[2].get("node_ranks")
        ref, _ = MU.oracle_of_scenario(flat.problem, present, np.arange(flat.problem.n_pods), None if ranks is None else ranks[s])
        assert row.tolist() == ref.tolist(), mix


def test_min_plan_caps_use_each_mix_s_own_nodes(monkeypatch):
    cluster, apps, types = MU.example_simple()
    flat, pool, base = _pool_problem(cluster, apps, types, [3, 3])
    mixes = np.array(list(itertools.product(range(4), range(4))), np.int32)
    scen = np.stack([len(base) + mixes.sum(1), np.zeros(len(mixes), np.int32)], 1).astype(np.int32)
    seg = ([len(base), len(base) + 3], mixes)
    with capi.Context(0) as ctx:
        ctx.load_problem(flat.problem)
        ctx.load_scenarios(scen, np.arange(flat.problem.n_pods, dtype=np.int32)[None])
        ctx.set_scenario_segments(*seg)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        a = flat.problem.alloc_cpu.astype(np.int64)
        m = flat.problem.alloc_mem.astype(np.int64)
        for cap in (100, 60, 30):
            plan, _ = ctx.min_plan_vg(cap, cap, 100)
            best = None
            for s, mix in enumerate(mixes):
                own = list(range(len(base))) + [len(base) + i for i in range(mix[0])] + [len(base) + 3 + i for i in range(mix[1])]
                if res.unscheduled[s] or sim.occupancy_pct(int(res.used_cpu[s]), int(a[own].sum())) > cap or \
                        sim.occupancy_pct(int(res.used_mem[s]) * 1000, int(m[own].sum()) * 1000) > cap:
                    continue
                key = (int(scen[s, 0]), s)
                best = key if best is None or key < best else best
            assert (plan.found, plan.scenario if plan.found else -1) == ((1, best[1]) if best else (0, -1)), cap
        with pytest.raises(capi.SimonError) as e:
            ctx.explain_loaded(0)
        assert e.value.code == capi.ESTATE


def test_refusals_leave_a_usable_context_and_clearing_restores_prefix_results():
    cluster, apps, types = MU.example_simple()
    flat, pool, base = _pool_problem(cluster, apps, types, [3, 2])
    N, B = len(pool), len(base)
    mixes = np.array([[0, 0], [1, 2], [3, 1]], np.int32)
    scen = np.stack([B + mixes.sum(1), np.zeros(3, np.int32)], 1).astype(np.int32)
    orders = np.arange(flat.problem.n_pods, dtype=np.int32)[None]
    with capi.Context(0) as ctx:
        ctx.load_problem(flat.problem)
        ctx.load_scenarios(scen, orders)
        bad = [([B + 3, B], mixes),                                  # starts not ascending
               ([B, B + 3], np.array([[0, 0], [4, 2], [3, 1]])),     # a count beyond its segment
               ([B, B + 3], np.array([[0, 0], [1, 1], [3, 1]])),     # n_nodes mismatch
               (list(range(B, B + 9)), np.zeros((3, 9), np.int32))]  # more than SIMON_MAX_SEGMENTS
        for st, cn in bad:
            with pytest.raises(capi.SimonError) as e:
                ctx.set_scenario_segments(st, cn)
            assert e.value.code == capi.EINVAL
        ctx.set_scenario_segments([B, B + 3], mixes)
        ctx.run_loaded(True)
        seg = ctx.fetch(True)
        ctx.set_scenario_segments(None, None)
        ctx.run_loaded(True)
        plain = ctx.fetch(True)
    with capi.Context(0) as ctx:
        ctx.load_problem(flat.problem)
        ref = ctx.run_batch(scen, orders)
    assert (plain.placement == ref.placement).all() and plain.unscheduled.tolist() == ref.unscheduled.tolist()
    assert seg.unscheduled.tolist()[0] == ref.unscheduled.tolist()[0]


def test_more_refusals_and_the_context_still_runs(monkeypatch):
    """SIMON_EINVAL: a segment node with pods bound before the stream, a preset pod's target in a segment, n_seg < 0; SIMON_ESTATE:
    ImageLocality loaded, a problem on the all-feature kernel (forced here) at run time.  Each leaves the batch a usable prefix batch."""
    import image_util
    prob, scen, orders = _route_case("gates_fine")
    seg_prob, F = _segmentable(prob, scen)
    cnt = scen[:, :1] - F
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)                                        # init state and presets everywhere
        ctx.load_scenarios(scen, orders)
        for st, cn in (([F], cnt), ([0], scen[:, :1]), ([-1], cnt)):
            with pytest.raises(capi.SimonError) as e:
                ctx.set_scenario_segments(st, cn)
            assert e.value.code == capi.EINVAL
        assert ctx.lib.simon_set_scenario_segments(ctx.h, -1, None, None) == capi.EINVAL
        ctx.run_loaded(True)
        after = ctx.fetch(True)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ref = ctx.run_batch(scen, orders)
    assert (after.placement == ref.placement).all()
    # ImageLocality
    cluster, apps, tmpl = image_util.image_sweep_case(3)
    b = sim.sweep_batch(cluster, apps, tmpl, [0, 1, 2], image_batch=True)
    assert b.flat.problem.image_locality is not None
    with capi.Context(0) as ctx:
        ctx.load_problem(b.flat.problem)
        ctx.load_scenarios(b.scen, b.orders)
        with pytest.raises(capi.SimonError) as e:
            ctx.set_scenario_segments([len(b.base)], b.scen[:, :1] - len(b.base))
        assert e.value.code == capi.ESTATE
        ctx.run_loaded(True)
    # the all-feature kernel
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    with capi.Context(0) as ctx:
        ctx.load_problem(seg_prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments([F], cnt)
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE
        ctx.set_scenario_segments(None, None)
        ctx.run_loaded(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_WIDE


def test_open_local_mixes_fall_back_visibly_and_match_the_oracle():
    """Open-Local needs the all-feature kernel, which takes no segments: sweep_mix warns, says why, and runs every mix as its own
    problem -- with the oracle's answers."""
    cluster, apps, types = MU.example_open_local()
    grid = [range(0, 4), range(0, 2)]
    with pytest.warns(sim.MixFallbackWarning):
        hip = sim.sweep_mix(cluster, apps, types, grid, engine=sim.HipEngine())
    assert not hip.batched and "refused" in hip.fallback
    with pytest.warns(sim.MixFallbackWarning):
        ref = sim.sweep_mix(cluster, apps, types, grid, engine=MU.OracleEngine())
    assert hip.counts == ref.counts and hip.unscheduled == ref.unscheduled and hip.vg_pct == ref.vg_pct
    assert hip.cpu_pct == ref.cpu_pct and hip.mem_pct == ref.mem_pct and hip.best == ref.best


# ---- the fuzz regime's slice, the state machine, degenerate shapes, the advertised batch size ---------------------------------------
def _slice():
    import fuzz_mix
    return sorted(fuzz_mix.SLICE)


@pytest.mark.parametrize("case", _slice())
def test_fuzz_mix_slice_on_its_pinned_route(case):
    """One case of tests/fuzz_mix.py (segments with starts anywhere, 1 ... 8 of them, caller ranks, plan caps, priorities -- see its
    docstring) with the kernel every run of it must take: the slice cannot drift onto another route unnoticed.  Array-level cases: every
    field of every scenario against the oracle on the scenario's own nodes; cases from 500 000 on: sweep_mix by object names against
    Simulate() of every mix alone."""
    import fuzz_mix
    ok, info = fuzz_mix.one_case(case)
    print(info)
    routes, fams = fuzz_mix.SLICE[case]
    assert not info["refused"], info
    assert info.get("slice_missing", []) == [], info
    assert [tuple(r) for r in info["routes"]] == [tuple(r) for r in routes], info
    assert sorted(info["families"]) == sorted(fams + ["multi_segment"]), info      # what the case is in the slice for: still so
    assert ok, info


def _assert_segmented(res, prob, scen, orders, starts, counts, ranks=None, gpu=False):
    for s in range(len(scen)):
        row, ref = MU.oracle_of_scenario(prob, MU.present_mask(prob.n_nodes, starts, counts[s]), orders[scen[s, 1]], None if ranks is None else ranks[s])
        assert res.placement[s].tolist() == row.tolist(), s
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s
        if gpu:
            assert (res.gpu_slices[s] == ref.gpu_slices[0]).all(), s


def _assert_same(a, b):
    assert (a.placement == b.placement).all() and a.unscheduled.tolist() == b.unscheduled.tolist()
    assert a.used_cpu.tolist() == b.used_cpu.tolist() and a.used_mem.tolist() == b.used_mem.tolist()


STATE = {"generation4": (dict(gates=True, pins=True, n_node_classes=9, n_pod_classes=8), {"SIMON_TABLE_COARSE": "0"}, 4),
         "generation7": (dict(spread_soft=True, gates=True, n_node_classes=4, n_pod_classes=8), {}, 7)}


@pytest.mark.parametrize("name", sorted(STATE))
def test_segments_ranks_and_batches_replace_each_other_on_one_context(name, monkeypatch):
    """The state machine of one context: three segments -> two other segments with other counts (same totals) -> caller rank rows ->
    simon_set_node_ranks(NULL) (pool order over each scenario's nodes again) -> no segments (the prefix batch) -> a new prefix batch.
    Every segmented run against the oracle on each scenario's own nodes, every prefix run against a fresh context."""
    kw, env, gen = STATE[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N, F, S = 150, 60, 6
    prob, _ = MU.segmentable(randprob.rand_problem(31, N=N, P=400, **kw), fixed=F)
    rng = np.random.default_rng(7)
    orders = np.stack([np.arange(prob.n_pods), rng.permutation(prob.n_pods), rng.permutation(prob.n_pods)]).astype(np.int32)
    st_a, st_b = np.array([F, 97, 131], np.int32), np.array([F, 110], np.int32)
    cnt_a = np.stack([rng.integers(0, n + 1, S) for n in (37, 34, 19)], 1).astype(np.int32)
    tot = cnt_a.sum(1)
    b0 = np.array([rng.integers(max(0, t - 40), min(t, 50) + 1) for t in tot])
    cnt_b = np.stack([b0, tot - b0], 1).astype(np.int32)
    assert (cnt_b >= 0).all() and (cnt_b <= [50, 40]).all()
    scen = np.stack([F + tot, rng.integers(0, 3, S)], 1).astype(np.int32)
    ranks = rng.integers(-3, N + 3, (S, N)).astype(np.int32)
    for s in range(S):
        own = np.flatnonzero(MU.present_mask(N, st_b, cnt_b[s]))
        ranks[s, own] = rng.permutation(len(own))
    scen2 = np.array([[N, 0], [90, 2], [33, 1], [120, 1]], np.int32)

    def fresh(sc):
        with capi.Context(0) as c2:
            c2.load_problem(prob)
            return c2.run_batch(sc, orders)

    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)

        def run():
            ctx.run_loaded(True)
            st = ctx.stats()
            assert (st.kernel_variant, st.kernel_generation) == (capi.KERNEL_NARROW_CACHE, gen)
            return ctx.fetch(True)

        ctx.set_scenario_segments(st_a, cnt_a)
        _assert_segmented(run(), prob, scen, orders, st_a, cnt_a)
        ctx.set_scenario_segments(st_b, cnt_b)
        after_b = run()
        _assert_segmented(after_b, prob, scen, orders, st_b, cnt_b)
        ctx.set_node_ranks(ranks)
        _assert_segmented(run(), prob, scen, orders, st_b, cnt_b, ranks)
        ctx.set_node_ranks(None)
        _assert_same(run(), after_b)
        ctx.set_scenario_segments(st_a, cnt_a)                       # back to A after ranks: pool order, A's class counts
        _assert_segmented(run(), prob, scen, orders, st_a, cnt_a)
        ctx.set_scenario_segments(None, None)
        _assert_same(run(), fresh(scen))
        ctx.load_scenarios(scen2, orders)
        _assert_same(run(), fresh(scen2))
        ctx.load_scenarios(scen, orders)                             # and a segmented batch after a prefix batch of another size
        ctx.set_scenario_segments(st_b, cnt_b)
        _assert_same(run(), after_b)


def test_degenerate_segment_shapes():
    """What the validator admits at the edges: eight segments, an empty one among them (two equal starts, and one that starts at N), no
    fixed nodes (seg_start[0] == 0), scenarios that hold every segment in full, nothing but the fixed nodes, or one single node.  A
    scenario of NO nodes (all counts 0 without fixed nodes) is refused with SIMON_EINVAL and leaves a usable batch."""
    N, P = 100, 300
    rng = np.random.default_rng(3)
    orders = np.stack([np.arange(P), rng.permutation(P)]).astype(np.int32)
    for F, starts in ((0, [0, 7, 7, 30, 41, 63, 64, 100]), (13, [13, 14, 29, 29, 50, 77, 99, 100])):
        prob, _ = MU.segmentable(randprob.rand_problem(40 + F, N=N, P=P, gates=True, pins=True, tight_pods=True, n_node_classes=9, n_pod_classes=8), fixed=F)
        starts = np.array(starts, np.int32)
        lens = np.append(starts[1:], N) - starts
        assert len(starts) == capi.MAX_SEGMENTS and (lens == 0).sum() == 2
        cnt = np.stack([rng.integers(0, n + 1, 6) for n in lens], 1).astype(np.int32)
        cnt[0] = lens                                                 # the whole pool
        cnt[1] = 0                                                    # nothing but the fixed nodes ...
        if F == 0:
            cnt[1, 3] = 1                                             # ... or one single node from the middle of the pool
        cnt[2] = 0
        cnt[2, 5] = lens[5]                                           # one whole segment far from the fixed nodes, nothing else
        scen = np.stack([F + cnt.sum(1), rng.integers(0, 2, 6)], 1).astype(np.int32)
        with capi.Context(0) as ctx:
            ctx.load_problem(prob)
            if F == 0:                                                # an empty scenario: refused before anything is laid out
                none = cnt.copy()
                none[1] = 0
                ctx.load_scenarios(np.stack([none.sum(1), scen[:, 1]], 1).astype(np.int32), orders)
                with pytest.raises(capi.SimonError) as e:
                    ctx.set_scenario_segments(starts, none)
                assert e.value.code == capi.EINVAL and "no node" in str(e.value)
            ctx.load_scenarios(scen, orders)
            ctx.set_scenario_segments(starts, cnt)
            ctx.run_loaded(True)
            res = ctx.fetch(True)
            assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
        _assert_segmented(res, prob, scen, orders, starts, cnt)
        assert res.unscheduled[1] > 0 and (res.placement[0] >= F).any()


def test_a_64_by_64_grid_of_mixes_in_one_launch():
    """The batch size sweep_mix advertises: 4 096 mixes of two node types (0 ... 63 nodes of each) behind 30 fixed nodes, one launch.
    Against the oracle: a fixed sample of the mixes that holds the grid's four corners and both edges (>= 256 of them); simon_min_plan_vg
    over ALL 4 096 results, recomputed in numpy with each mix's own allocatable totals."""
    F, K = 30, 63
    N, P = F + 2 * K, 300
    prob, _ = MU.segmentable(randprob.rand_problem(64, N=N, P=P, gates=True, tight_pods=True, n_node_classes=9, n_pod_classes=8), fixed=F)
    mixes = np.array(list(itertools.product(range(K + 1), range(K + 1))), np.int32)
    starts = np.array([F, F + K], np.int32)
    scen = np.stack([F + mixes.sum(1), np.zeros(len(mixes), np.int32)], 1).astype(np.int32)
    orders = np.arange(P, dtype=np.int32)[None]
    caps = (100, 70, 45, 20)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(starts, mixes)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        st = ctx.stats()
        plans = [ctx.min_plan_vg(cap, cap, 100)[0] for cap in caps]
        plans = [(int(p.found), int(p.scenario) if p.found else -1) for p in plans]
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.n_launches == 1 and len(mixes) == 4096
    idx = lambda a, b: a * (K + 1) + b                               # noqa: E731
    sample = sorted({idx(a, b) for a in (0, K) for b in (0, K)} | {idx(0, b) for b in range(K + 1)} | {idx(a, 0) for a in range(K + 1)} |
                    set(range(0, 4096, 11)))
    assert len(sample) >= 256
    sub = sample
    _assert_segmented(type("R", (), dict(placement=res.placement[sub], unscheduled=res.unscheduled[sub], used_cpu=res.used_cpu[sub],
                                         used_mem=res.used_mem[sub])), prob, scen[sub], orders, starts, mixes[sub])
    ca = np.concatenate([[0], np.cumsum(prob.alloc_cpu.astype(np.int64))])
    cm = np.concatenate([[0], np.cumsum(prob.alloc_mem.astype(np.int64))])
    tot = lambda c: c[F] + (c[F + mixes[:, 0]] - c[F]) + (c[F + K + mixes[:, 1]] - c[F + K])   # noqa: E731
    ac, am = tot(ca), tot(cm)
    cpu = np.array([sim.occupancy_pct(int(u), int(a)) for u, a in zip(res.used_cpu, ac)])
    mem = np.array([sim.occupancy_pct(int(u) * 1000, int(a) * 1000) for u, a in zip(res.used_mem, am)])
    assert (res.unscheduled == 0).any() and (res.unscheduled > 0).any()
    for cap, got in zip(caps, plans):
        ok = np.flatnonzero((res.unscheduled == 0) & (cpu <= cap) & (mem <= cap))
        want = (1, int(min(ok, key=lambda s: (int(scen[s, 0]), s)))) if len(ok) else (0, -1)
        assert got == want, cap
    assert plans[0][0] == 1


def _risk_case():
    N, F = 47, 12
    prob, _ = MU.segmentable(randprob.rand_problem(6101, N=N, P=160, presets=True, gates=True, tight_pods=True), fixed=F)
    rng = np.random.default_rng(1)
    prob.priority = rng.choice([0, 0, 0, 10, 1000, -5], prob.n_pods).astype(np.int32)
    prob.init_min_priority = 100
    starts = np.array([F, 25, 38], np.int32)
    lens = np.array([13, 13, 9])
    cnt = np.stack([rng.integers(0, n + 1, 10) for n in lens], 1).astype(np.int32)
    cnt[0], cnt[1] = lens, 0
    scen = np.stack([F + cnt.sum(1), rng.integers(0, 2, 10)], 1).astype(np.int32)
    orders = np.stack([np.arange(160), rng.permutation(160)]).astype(np.int32)
    return prob, scen, orders, starts, cnt


def test_preempt_risk_flags_of_a_segmented_batch():
    """simon_fetch_preempt_risk on a segmented batch of pods with unequal priorities: the oracle's flag of every scenario on its own nodes
    (flags set and flags unset in the batch), next to placements and aggregates."""
    prob, scen, orders, starts, cnt = _risk_case()
    want = []
    for s in range(len(scen)):
        _, ref = MU.oracle_of_scenario(prob, MU.present_mask(prob.n_nodes, starts, cnt[s]), orders[scen[s, 1]])
        want.append(int(ref.preempt_risk[0]))
    assert 0 in want and 1 in want
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(starts, cnt)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        assert ctx.fetch_preempt_risk().tolist() == want
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
    _assert_segmented(res, prob, scen, orders, starts, cnt)

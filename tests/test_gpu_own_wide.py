"""Segmented and node-subset batches on the all-feature kernel (simon_set_own_nodes_all_feature, the own-nodes run forms of
simon_wide_own.hip): the option off and on; presence rows that spell prefixes, bit for bit against the prefix batch on the same
kernel; arbitrary subsets and two- / three-segment batches of every plugin family against the CPU oracle on each scenario's own
problem, pod by pod; pods flagged for eviction; pod sets next to node sets; one scenario per launch against the whole batch; the plan's
caps over each scenario's own nodes; explain on a wide-routed batch; sweep_mix and sweep_failures on an Open-Local cluster end to end,
with the storage table and headroom against their host twins.  Every test sets the option.  Run with -m gpu on an MI355X."""
import dataclasses
import functools
import itertools
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import evict_util as EU
import explain_own_util as OU
import mix_util as MU
import oracle_lib as O
import podset_util as PU
import randprob
import subset_util as SU
from open_simulator_amd import capi, simulate as sim
from test_gpu_subsets import _random_rows, _scen_of

pytestmark = pytest.mark.gpu

P = 120
# (name, pool nodes, environment): two nodes per lane of one wave; a second load batch of five nodes per lane and a ragged last one;
# more than one wave, two nodes per lane in the first 44 lanes
SHAPES = [("wg64_n70", 70, {"SIMON_WG": "64"}), ("wg64_n330", 330, {"SIMON_WG": "64"}), ("wg256_n300", 300, {})]
# family -> randprob.rand_problem keywords (`ports` beside `anti` is what the family is named for; randprob binds host ports only in
# its node-level topology, which "ports_host" draws)
FAMILIES = {
    "plain": dict(),
    "gpu": dict(gpu=True),
    "anti_aff_ports": dict(anti=True, aff=True, ports=True),
    "ports_host": dict(ports=True, anti_host=True, tight_pods=True),
    "spread_hard": dict(spread_hard=True),
    "hard_simple": dict(hard_simple=True),
    "soft_ipa": dict(spread_soft=True, ipa=True, ipa_self=True),
    "soft_ipa_self": dict(spread_soft=True, ipa_self=True),
    "local": dict(local=True),
    "eph_scalars": dict(eph=True, scalars=2, tight_pods=True),
    "static": dict(static_mask=True, pins=True, gates=True, presets=True),
    "classes3": dict(n_node_classes=3),          # the single-pass cycle (class mode, at most 8 node classes)
    "classes20": dict(n_node_classes=20),        # class mode
    # more than 64 node classes: the class rows in LDS.  The all-feature kernel goes by the DECLARED class count (WideArgs::Cn =
    # n_node_classes; class mode needs Cn <= 64), so a 70-node pool that draws fewer distinct classes takes that path too
    "classes70": dict(n_node_classes=70),
}
ALL = [(f, sh) for f in FAMILIES for sh in range(len(SHAPES))]
IDS = [f"{f}-{SHAPES[sh][0]}" for f, sh in ALL]


def _replaced(prob, **changes):
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    return capi.Problem(**dict(kw, **changes)).normalise()


@functools.lru_cache(maxsize=None)
def family_problem(family, N):
    """The family's problem over N nodes, subset-ready (no state before the stream); a preset pod stays preset to, and gated on, its node."""
    seed = 100 + sorted(FAMILIES).index(family)
    base = randprob.rand_problem(seed, N=N, P=P, **FAMILIES[family])
    prob, _ = MU.segmentable(base, fixed=0)
    if base.preset_node is not None:
        pre = np.asarray(base.preset_node)
        prob = _replaced(prob, preset_node=pre.copy(), gate_node=np.where(pre >= 0, pre, prob.gate_node).astype(np.int32))
    rng = np.random.default_rng(seed)
    orders = np.stack([np.arange(P), rng.permutation(P)]).astype(np.int32)
    assert prob.n_node_classes == FAMILIES[family].get("n_node_classes", 5)      # (what decides class mode / rows in LDS / neither)
    if family == "classes70" and N >= 300:
        assert len(np.unique(prob.node_class)) > 64
    return prob, orders


def _env(monkeypatch, shape, **more):
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    for k in ("SIMON_WG", "SIMON_STATE_BUDGET_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(SHAPES[shape][2], **more).items():
        monkeypatch.setenv(k, v)


def _ctx(on=True):
    ctx = capi.Context(0)
    if on:
        ctx.set_own_nodes_all_feature(True)
    return ctx


def _fetch(ctx, prob):
    want_gpu = prob.gpu_mem is not None
    ctx.run_loaded(True, want_gpu)
    st = ctx.stats()
    assert (st.kernel_variant, st.kernel_generation) == (capi.KERNEL_WIDE, 0), (st.kernel_variant, st.kernel_generation)
    return ctx.fetch(True, want_gpu)


def _same(a, b, prob):
    assert (a.placement == b.placement).all(), np.argwhere(a.placement != b.placement)[:4].tolist()
    assert a.unscheduled.tolist() == b.unscheduled.tolist()
    assert a.used_cpu.tolist() == b.used_cpu.tolist() and a.used_mem.tolist() == b.used_mem.tolist()
    if prob.local_flags is not None:
        assert a.used_vg.tolist() == b.used_vg.tolist()
    if prob.gpu_mem is not None:
        assert (a.gpu_slices == b.gpu_slices).all()


def _against_oracle(res, s, prob, row, ref):
    assert res.placement[s].tolist() == row.tolist(), (s, np.flatnonzero(res.placement[s] != row)[:6].tolist())
    got = (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s]))
    assert got == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s
    if prob.local_flags is not None:
        assert int(res.used_vg[s]) == int(ref.used_vg[0]), s
    if prob.gpu_mem is not None:
        assert (res.gpu_slices[s] == ref.gpu_slices[0]).all(), s


@functools.lru_cache(maxsize=None)
def subset_case(family, shape):
    """(problem, mask [8][N], zone, scen, orders, ranks, oracle rows) of a family at a shape: eight seeded rows over three zones."""
    N = SHAPES[shape][1]
    prob, orders = family_problem(family, N)
    rng = np.random.default_rng(1000 * shape + sorted(FAMILIES).index(family))
    mask = _random_rows(rng, N)
    zone = rng.integers(0, 3, N).astype(np.int32)
    scen = _scen_of(mask, rng.integers(0, len(orders), len(mask)))
    ranks = SU.zone_ranks(mask, zone)
    rows = [MU.oracle_of_scenario(prob, mask[s], orders[scen[s, 1]], ranks[s]) for s in range(len(mask))]
    return prob, mask, zone, scen, orders, ranks, rows


# ---- 1. the option off and on ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["local", "hard_simple"])
def test_option_off_refuses_as_before_and_on_runs_on_the_same_context(family, monkeypatch):
    _env(monkeypatch, 0)
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, 0)
    N = prob.n_nodes
    pscen = np.array([[N, 0], [N // 2, 1], [3, 0]], np.int32)
    with _ctx(on=False) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(pscen, orders)
        fresh = _fetch(ctx, prob)
    with _ctx(on=False) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE
        assert "run_loaded: node-subset batch on a problem the score-table kernel does not take; run each scenario's own problem" in str(e.value)
        ctx.set_own_nodes_all_feature(True)
        res = _fetch(ctx, prob)
        for s in range(len(mask)):
            _against_oracle(res, s, prob, *rows[s])
        ctx.set_own_nodes_all_feature(False)                           # ... and off again: the refusal is back
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE and "node-subset batch" in str(e.value)
        ctx.set_own_nodes_all_feature(True)
        ctx.load_problem(prob)                                         # sticky across loads
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        _same(_fetch(ctx, prob), res, prob)
        ctx.load_scenarios(pscen, orders)                              # a prefix batch on that context equals a fresh context's
        _same(_fetch(ctx, prob), fresh, prob)


# ---- 2. rows that spell prefixes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", ALL, ids=IDS)
def test_rows_that_spell_prefixes_equal_the_prefix_batch_bit_for_bit(family, shape, monkeypatch):
    _env(monkeypatch, shape)
    N = SHAPES[shape][1]
    prob, orders = family_problem(family, N)
    rng = np.random.default_rng(shape)
    sizes = np.concatenate([[N, 3, N - 1, 65 if N > 65 else 33], rng.integers(4, N, 2)])
    scen = np.stack([sizes, rng.integers(0, len(orders), len(sizes))], 1).astype(np.int32)
    mask = np.arange(N)[None, :] < scen[:, :1]
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        want = _fetch(ctx, prob)
        ctx.set_scenario_nodes(mask)
        got = _fetch(ctx, prob)
    _same(got, want, prob)
    assert (want.placement >= 0).any()


# ---- 3. arbitrary subsets and segments against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", ALL, ids=IDS)
def test_arbitrary_subsets_match_the_oracle_pod_by_pod(family, shape, monkeypatch):
    _env(monkeypatch, shape)
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, shape)
    N = prob.n_nodes
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        assert (ctx.fetch_node_ranks() == np.where(ranks < 0, N, ranks)).all()
        res = _fetch(ctx, prob)
        assert ctx.stats().workgroup_size == (64 if shape < 2 else 256)
    for s in range(len(mask)):
        _against_oracle(res, s, prob, *rows[s])
        placed = res.placement[s][res.placement[s] >= 0]
        assert mask[s][placed].all()                                  # nobody lands on an absent node
        if s in (1, 5):
            other, _ = MU.oracle_of_restricted(prob, mask[s], orders[scen[s, 1]], ranks[s])
            assert other.tolist() == rows[s][0].tolist(), s
    print(family, SHAPES[shape][0], "unscheduled per scenario:", res.unscheduled.tolist())
    assert (res.placement >= 0).any()


@pytest.mark.parametrize("n_seg", [2, 3])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_segments_match_the_oracle_pod_by_pod(family, n_seg, monkeypatch):
    _env(monkeypatch, 0)
    N, S = SHAPES[0][1], 6
    base, orders = family_problem(family, N)
    F = N // 3
    prob, _ = MU.segmentable(base, fixed=F)
    rng = np.random.default_rng(10 * n_seg + sorted(FAMILIES).index(family))
    starts = np.sort(np.concatenate([[F], rng.choice(np.arange(F + 1, N), n_seg - 1, replace=False)])).astype(np.int32)
    lens = np.append(starts[1:], N) - starts
    cnt = np.stack([rng.integers(0, n + 1, S) for n in lens], 1).astype(np.int32)
    cnt[0], cnt[1] = lens, 0
    scen = np.stack([F + cnt.sum(1), rng.integers(0, len(orders), S)], 1).astype(np.int32)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(starts, cnt)
        res = _fetch(ctx, prob)
    for s in range(S):
        present = MU.present_mask(N, starts, cnt[s])
        _against_oracle(res, s, prob, *MU.oracle_of_scenario(prob, present, orders[scen[s, 1]]))
        if s in (2, 4):
            other, _ = MU.oracle_of_restricted(prob, present, orders[scen[s, 1]])
            assert other.tolist() == res.placement[s].tolist(), s
    assert (res.placement >= F).any()


# ---- 4. rescheduling ------------------------------------------------------------------------------------------------------------------------
def _local_evict_case():
    """An Open-Local problem with flagged pods on three nodes, as evict_util.route_case builds its cases."""
    prob, orders = family_problem("local", 70)
    N = prob.n_nodes
    rng = np.random.default_rng(44)
    ok = EU.eligible(prob)
    t0, t1, t2 = [int(j) for j in rng.choice(N, 3, replace=False)]
    picked = [int(p) for p in ok[:12]]
    prob, evict = EU.flag(prob, {p: (t1 if i == 0 else t2 if i % 4 == 1 else t0) for i, p in enumerate(picked)}, huge=picked[0])
    mask = np.stack([rng.random(N) < q for q in (1.0, 1.0, 1.0, 0.5, 0.7, 0.9)])
    mask[0] = True
    mask[1, t0] = False
    mask[2, [t0, t1, t2]] = False
    mask[3, t1] = False
    zone = rng.integers(0, 3, N).astype(np.int32)
    scen = _scen_of(mask, rng.integers(0, len(orders), len(mask)))
    ranks = SU.zone_ranks(mask, zone)
    return prob, evict, mask, zone, scen, orders, ranks, EU.oracle_rows(prob, evict, mask, scen, orders, ranks, restricted=(2, 4))


@pytest.mark.parametrize("case", ["gates", "gpu", "local"])
def test_pods_preset_to_an_absent_node_are_scheduled_again(case, monkeypatch):
    _env(monkeypatch, 0)
    prob, evict, mask, zone, scen, orders, ranks, rows = _local_evict_case() if case == "local" else EU.route_case(case)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
    pre = np.asarray(prob.preset_node)
    for s, (row, ref, gone) in enumerate(rows):
        _against_oracle(res, s, prob, row, ref)
        stay = evict & ~gone
        assert (res.placement[s][stay] == pre[stay]).all(), s          # bound where the node is present
        assert (res.placement[s][gone] != capi.GATED).all(), s         # ... scheduled afresh where it is not
    placed, failed = EU.evicted_counts(rows)
    assert placed > 0 and failed > 0


# ---- 5. pod sets plus node sets --------------------------------------------------------------------------------------------------------------
def _pod_rows(prob, S, seed):
    rng = np.random.default_rng(seed)
    keep = np.stack([rng.random(prob.n_pods) < q for q in np.linspace(0.4, 0.95, S)])
    keep[0] = True
    keep[1] = np.asarray(prob.pod_class) != np.bincount(np.asarray(prob.pod_class)).argmax()     # one whole class absent
    if S > 2:
        keep[2] = False                                                  # a scenario of no pod at all
    return keep


@pytest.mark.parametrize("family", ["hard_simple", "gpu", "local", "soft_ipa"])
def test_pod_sets_and_node_sets_in_one_batch(family, monkeypatch):
    _env(monkeypatch, 0)
    prob, mask, zone, scen, orders, ranks, _ = subset_case(family, 0)
    keep = _pod_rows(prob, len(mask), 5)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_pods(keep)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
    for s in range(len(mask)):
        want = PU.oracle_nodes(prob, keep[s], mask[s], orders[scen[s, 1]], ranks[s])
        assert res.placement[s].tolist() == want.placement.tolist(), s
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (want.unscheduled, want.used_cpu, want.used_mem), s
        if prob.gpu_mem is not None:
            assert (res.gpu_slices[s] == want.gpu_slices).all(), s
        assert (res.placement[s][~keep[s]] == capi.GATED).all()
    assert (res.placement[0] >= 0).any() and (res.placement[2] == capi.GATED).all()


# ---- 6. one scenario per launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,podsets", [("spread_hard", False), ("hard_simple", True), ("gpu", True)], ids=["spread_hard", "hard_simple_podsets", "gpu_podsets"])
def test_chunked_launches_equal_the_whole_batch(family, podsets, monkeypatch):
    """SIMON_STATE_BUDGET_MB=0: a launch per scenario, so the registered flags, the rank rows and the pod rows of scenario s are found
    at scen_base + s of the batch's tables."""
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, 0)
    mask, scen = mask[[7, 1, 4, 0, 5]], scen[[7, 1, 4, 0, 5]]
    keep = _pod_rows(prob, 5, 6)[[3, 0, 4, 1, 2]] if podsets else None
    out = []
    for budget in (None, "0"):
        _env(monkeypatch, 0, **({} if budget is None else {"SIMON_STATE_BUDGET_MB": budget}))
        with _ctx() as ctx:
            ctx.load_problem(prob)
            ctx.load_scenarios(scen, orders)
            if keep is not None:
                ctx.set_scenario_pods(keep)
            ctx.set_scenario_nodes(mask, zone)
            out.append(_fetch(ctx, prob))
    _same(out[1], out[0], prob)
    if not podsets:
        for k, s in enumerate([7, 1, 4, 0, 5]):
            _against_oracle(out[1], k, prob, *rows[s])
    assert len({tuple(r) for r in out[0].placement.tolist()}) > 1         # the scenarios differ: a wrong row would show


# ---- 7. the plan ------------------------------------------------------------------------------------------------------------------------------
def test_min_plan_caps_use_each_scenario_s_own_nodes(monkeypatch):
    _env(monkeypatch, 2)                                # (300 nodes: the pool at which some scenarios of the family place every pod)
    prob, mask, zone, scen, orders, ranks, _ = subset_case("local", 2)
    big = np.concatenate([mask, _random_rows(np.random.default_rng(7), prob.n_nodes)[2:]])
    scen = _scen_of(big, np.zeros(len(big), np.int64))
    ranks = SU.zone_ranks(big, zone)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(big, zone)
        res = _fetch(ctx, prob)
        own = []
        for s in range(len(big)):                       # every scenario as its own (restricted) problem on the oracle
            nodes = np.flatnonzero(big[s])
            nodes = nodes[np.argsort(ranks[s][nodes], kind="stable")]
            sub, _ = MU.restrict_nodes(prob, nodes)
            r = O.run(sub, [[len(nodes), 0]], orders[:1])
            assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s]), int(res.used_vg[s])) == \
                   (int(r.unscheduled[0]), int(r.used_cpu[0]), int(r.used_mem[0]), int(r.used_vg[0])), s
            own.append((sub, len(nodes), r))
        found = []
        for cap, vg in ((100, 100), (70, 100), (100, 3), (100, 2), (2, 100), (1, 100)):
            ok = {}
            for s, (sub, n, r) in enumerate(own):
                plan, pct = O.min_plan_vg(sub, [[n, 0]], r, cap, cap, vg)
                if plan.found:
                    ok[s] = (plan, pct)
            best = min(ok, key=lambda s: (int(scen[s, 0]), s)) if ok else None
            plan, pct = ctx.min_plan_vg(cap, cap, vg)
            assert (plan.found, plan.scenario if plan.found else -1) == ((1, best) if best is not None else (0, -1)), (cap, vg)
            if best is not None:
                assert (plan.n_nodes, plan.cpu_pct, plan.mem_pct, pct) == (ok[best][0].n_nodes, ok[best][0].cpu_pct, ok[best][0].mem_pct, ok[best][1]), (cap, vg)
            if vg == 100:                                # simon_min_plan: the same without the MaxVG cap
                p2 = ctx.min_plan(cap, cap)
                one = {s: O.min_plan(sub, [[n, 0]], r, cap, cap) for s, (sub, n, r) in enumerate(own)}
                ok2 = [s for s in one if one[s].found]
                b2 = min(ok2, key=lambda s: (int(scen[s, 0]), s)) if ok2 else None
                assert (p2.found, p2.scenario if p2.found else -1) == ((1, b2) if b2 is not None else (0, -1)), cap
                if b2 is not None:
                    assert (p2.cpu_pct, p2.mem_pct) == (one[b2].cpu_pct, one[b2].mem_pct)
            found.append(best)
    assert len(set(found)) >= 3 and None in found       # the caps move the answer, and the tightest finds none


# ---- 8. explain -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", [("spread_hard", 0), ("static", 0), ("gpu", 2), ("anti_aff_ports", 0)])
def test_explain_own_batch_takes_a_wide_routed_batch(family, shape, monkeypatch):
    _env(monkeypatch, shape)
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, shape)
    listed = [5, 0, 7, 2, 1, 6, 3, 4, 1]
    with _ctx(on=False) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        with pytest.raises(capi.SimonError) as e:
            ctx.explain_own_batch(listed, 64, 32)
        assert e.value.code == capi.ESTATE and "explain each scenario's own problem" in str(e.value)
        ctx.set_own_nodes_all_feature(True)
        eb = ctx.explain_own_batch(listed, 64, 32, rows=True)
        res = _fetch(ctx, prob)
    seen = {}
    for k, s in enumerate(listed):
        seen[s] = OU.assert_explained(eb, k, prob, mask[s], orders[scen[s, 1]], ranks[s], 64, 32, True)
    assert res.unscheduled.tolist() == [seen[s][0] for s in range(len(mask))]       # the replay counts what the run counted
    assert sum(1 for s in seen if seen[s][0]) >= 2


def test_an_open_local_batch_still_refuses_to_explain(monkeypatch):
    _env(monkeypatch, 0)
    prob, mask, zone, scen, orders, ranks, rows = subset_case("local", 0)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
        with pytest.raises(capi.SimonError) as e:
            ctx.explain_own_batch([0, 1], 8, 8)
        assert e.value.code == capi.ESTATE
        assert "explain_own_batch: node-subset batch on a problem the score-table kernel does not take; explain each scenario's own problem" in str(e.value)
        _same(ctx.fetch(True), res, prob)                              # the results are undisturbed
    assert res.unscheduled[1] > 0


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------------------------
class _Recording(sim.HipEngine):
    """Keeps the arguments and the result of the own-nodes batch (not of the replays a sweep with reasons runs after it)."""

    def run(self, prob, scen, orders, **kw):
        out = super().run(prob, scen, orders, **kw)
        if kw.get("segments") is not None or kw.get("present") is not None:
            self.seen, self.out = (prob, capi.scenarios_array(scen), np.asarray(orders), kw), out
        return out


GRID = [range(0, 4), range(0, 2)]


def test_sweep_mix_batches_an_open_local_cluster(monkeypatch):
    monkeypatch.delenv("SIMON_FORCE_WIDE", raising=False)
    cluster, apps, types = MU.example_open_local()
    eng = _Recording(own_nodes_all_feature=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                 # no fallback warning, nor any other
        hip = sim.sweep_mix(cluster, apps, types, GRID, engine=eng, reasons=True)
    assert hip.batched and hip.fallback is None
    assert (eng.last_stats.kernel_variant, eng.last_stats.kernel_generation) == (capi.KERNEL_WIDE, 0)
    with pytest.warns(sim.MixFallbackWarning):
        ref = sim.sweep_mix(cluster, apps, types, GRID, engine=MU.OracleEngine(), reasons=True)
    assert hip.counts == ref.counts == list(itertools.product(*GRID))
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.vg_pct, hip.best, hip.cost) == (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.vg_pct, ref.best, ref.cost)
    names = lambda lists: [sorted((u["pod"]["metadata"]["name"], u["reason"]) for u in lst) for lst in lists]   # noqa: E731
    assert names(hip.unscheduled_pods) == names(ref.unscheduled_pods)        # (Open-Local: the failing mixes take their own replay)
    import fuzz_mix
    flat = fuzz_mix.pool_flat(SimpleNamespace(cluster=cluster, apps=apps, types=types, grid=[list(g) for g in GRID]))
    for s, mix in enumerate(hip.counts):                               # every mix by object names against Simulate() of that mix alone
        res, where, _ = MU.mix_answer(cluster, apps, types, mix)
        assert fuzz_mix.names_of_row(flat, eng.out.placement[s]) == where, mix
        assert hip.unscheduled[s] == len(res.unscheduled_pods), mix
    assert any(hip.unscheduled) and hip.best is not None


@pytest.mark.parametrize("reschedule", [False, "owned"])
def test_sweep_failures_batches_an_open_local_cluster(reschedule, monkeypatch):
    monkeypatch.delenv("SIMON_FORCE_WIDE", raising=False)
    cluster, apps, _ = MU.example_open_local()
    eng = sim.HipEngine(own_nodes_all_feature=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hip = sim.sweep_failures(cluster, apps, "node", engine=eng, reschedule=reschedule)
    assert hip.batched and hip.fallback is None
    assert (eng.last_stats.kernel_variant, eng.last_stats.kernel_generation) == (capi.KERNEL_WIDE, 0)
    answers = EU.evicted_answers(cluster, apps, hip.domains, reschedule) if reschedule else SU.reduced_answers(cluster, apps, hip.domains)
    assert [w for w, _ in answers] == hip.placements
    assert [n for _, n in answers[1:]] == hip.unscheduled               # (answers[0]: the whole cluster)
    with pytest.warns(sim.FailureFallbackWarning):
        ref = sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine(), reschedule=reschedule)
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.vg_pct, hip.baseline) == (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.vg_pct, ref.baseline)


def _usage_against_the_host_twins(eng, held, probes):
    prob, scen, orders, kw = eng.seen
    out = eng.out
    assert out.local_usage is not None and out.node_usage is not None and out.headroom is not None
    lu = sim.host_local_usage(prob, out.placement, held, orders, scen)
    assert (out.local_usage.vg_req == lu.vg_req).all() and (out.local_usage.dev_alloc == lu.dev_alloc).all()
    nu = sim.host_node_usage(prob, out.placement, held)
    assert (out.node_usage.req_cpu == nu.req_cpu).all() and (out.node_usage.req_mem == nu.req_mem).all() and (out.node_usage.npods == nu.npods).all()
    fit, _, exact = sim.host_headroom(prob, out.placement, held, probes, out.gpu_slices, storage=True, orders=orders, scen=scen)
    assert np.asarray(out.headroom).tolist() == fit.tolist() and np.asarray(out.headroom_exact).tolist() == exact.tolist()
    assert (nu.npods[~held] == -1).all() and (lu.dev_alloc[~held] == -1).all() and (~held).any()
    return fit


def test_storage_and_headroom_of_the_new_batches_equal_the_host_twins(monkeypatch):
    monkeypatch.delenv("SIMON_FORCE_WIDE", raising=False)
    cluster, apps, types = MU.example_open_local()
    eng = _Recording(own_nodes_all_feature=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hip = sim.sweep_mix(cluster, apps, types, GRID, engine=eng, headroom=[0, 1], node_table=True, storage=True)
    assert hip.batched and hip.storage_table is not None and hip.node_table is not None
    prob, scen, orders, kw = eng.seen
    starts, cnt = kw["segments"]
    held = np.stack([MU.present_mask(prob.n_nodes, starts, cnt[s]) for s in range(len(scen))])
    fit = _usage_against_the_host_twins(eng, held, np.array(kw["headroom_pods"], np.int32))
    assert np.asarray(hip.headroom).tolist() == fit.tolist()
    eng = _Recording(own_nodes_all_feature=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fail = sim.sweep_failures(cluster, apps, "node", engine=eng, headroom=[0, 1], node_table=True, storage=True)
    assert fail.batched and fail.storage_table is not None
    prob, scen, orders, kw = eng.seen
    held = np.asarray(kw["present"][0], bool)
    _usage_against_the_host_twins(eng, held, np.array(kw["headroom_pods"], np.int32))


# ---- 10. GPU-share devices of the new batches against the host twins ---------------------------------------------------------------------------
def _gpu_usage_against_the_host_twins(prob, placement, slices, held, usage, headroom, exact, probes):
    want = sim.host_gpu_usage(prob, placement, slices, held)
    assert (usage.dev_used == want.dev_used).all() and (usage.dev_pods == want.dev_pods).all()
    assert (want.dev_pods[~held] == -1).all() and (~held).any() and (want.dev_used > 0).any()
    fit, _, ex = sim.host_headroom(prob, placement, held, probes, slices, devices=True)
    assert np.asarray(headroom).tolist() == fit.tolist() and np.asarray(exact).tolist() == ex.tolist()
    return fit


@pytest.mark.parametrize("shape", [0, 2])
def test_gpu_usage_and_device_headroom_of_a_node_subset_batch(shape, monkeypatch):
    """simon_fetch_gpu_usage, simon_fetch_headroom_gpu and simon_fetch_node_usage after an own-nodes run on the all-feature kernel, against
    simulate.host_gpu_usage / host_headroom(devices=True) / host_node_usage of the placements and recorded devices the run itself gave
    (which test_arbitrary_subsets_match_the_oracle_pod_by_pod holds to the oracle)."""
    _env(monkeypatch, shape)
    prob, mask, zone, scen, orders, ranks, rows = subset_case("gpu", shape)
    gm = np.asarray(prob.gpu_mem)
    probes = np.concatenate([np.flatnonzero(gm > 0)[:4], np.flatnonzero(gm == 0)[:2]]).astype(np.int32)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
        usage = ctx.fetch_gpu_usage(pods=True)
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, devices=True)
        plain, _, _ = ctx.fetch_headroom(probes)
        nu = ctx.fetch_node_usage()
    for s in range(len(mask)):
        _against_oracle(res, s, prob, *rows[s])
    want = _gpu_usage_against_the_host_twins(prob, res.placement, res.gpu_slices, mask, usage, fit, exact, probes)
    _, want_nodes, _ = sim.host_headroom(prob, res.placement, mask, probes, res.gpu_slices, devices=True)
    assert nodes.tolist() == want_nodes.tolist()
    assert plain.tolist() == sim.host_headroom(prob, res.placement, mask, probes)[0].tolist()
    assert (want <= plain).all() and (want[:, :4] < plain[:, :4]).any() and exact[:4].all()      # the devices bind somewhere
    hn = sim.host_node_usage(prob, res.placement, mask)
    assert (nu.req_cpu == hn.req_cpu).all() and (nu.req_mem == hn.req_mem).all() and (nu.npods == hn.npods).all()


@pytest.mark.parametrize("sweep", ["failures", "mix"])
def test_devices_and_headroom_of_the_sweeps_on_a_gpu_share_cluster(sweep, monkeypatch):
    """devices=True, headroom= and node_table=True through sweep_failures / sweep_mix on the reference's GPU-share example, forced onto the
    all-feature kernel with the opt-in engine: what the engine reduced on the device against the host twins."""
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    cluster, apps, types = MU.example_gpushare()
    eng = _Recording(own_nodes_all_feature=True)
    probe_kw = dict(headroom=[0, 1, 2, 3], node_table=True, devices=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if sweep == "failures":
            hip = sim.sweep_failures(cluster, apps, "node", engine=eng, **probe_kw)
        else:
            hip = sim.sweep_mix(cluster, apps, types, [range(0, 3), range(0, 2)], engine=eng, **probe_kw)
    assert hip.batched and hip.fallback is None and hip.gpu_table is not None and hip.node_table is not None
    assert (eng.last_stats.kernel_variant, eng.last_stats.kernel_generation) == (capi.KERNEL_WIDE, 0)
    prob, scen, orders, kw = eng.seen
    if sweep == "failures":
        held = np.asarray(kw["present"][0], bool)
    else:
        held = np.stack([MU.present_mask(prob.n_nodes, kw["segments"][0], kw["segments"][1][s]) for s in range(len(scen))])
    out = eng.out
    assert out.gpu_usage is not None and out.gpu_slices is not None and kw.get("headroom_devices")
    fit = _gpu_usage_against_the_host_twins(prob, out.placement, out.gpu_slices, held, out.gpu_usage, out.headroom, out.headroom_exact,
                                            np.array(kw["headroom_pods"], np.int32))
    assert np.asarray(hip.headroom).tolist() == fit.tolist()
    nu = sim.host_node_usage(prob, out.placement, held)
    assert (out.node_usage.req_cpu == nu.req_cpu).all() and (out.node_usage.npods == nu.npods).all()


# ---- 11. the full evaluation of stage A (no signature table) and the 1 024-thread forms ------------------------------------------------------------
@pytest.mark.parametrize("family,shape", [("spread_hard", 0), ("spread_hard", 2), ("local", 0), ("static", 0), ("gpu", 0), ("soft_ipa", 1)])
def test_the_full_evaluation_branch_honours_presence(family, shape, monkeypatch):
    """SIMON_WIDE_NO_TABLE=1: no (signature, node) table, so stage A evaluates every node of every pod through filter_code -- presence
    from the lane's mask word, the registered flags through head_code."""
    _env(monkeypatch, shape, SIMON_WIDE_NO_TABLE="1")
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, shape)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
    for s in range(len(mask)):
        _against_oracle(res, s, prob, *rows[s])


@pytest.mark.parametrize("family", ["local", "spread_hard", "gpu"])
def test_the_1024_thread_forms(family, monkeypatch):
    """SIMON_WG=1024: the instantiations a pool beyond 16 384 nodes would take (128 VGPRs, most spills of the unit), on 330 nodes."""
    _env(monkeypatch, 1, SIMON_WG="1024")
    prob, mask, zone, scen, orders, ranks, rows = subset_case(family, 1)
    with _ctx() as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        res = _fetch(ctx, prob)
        assert ctx.stats().workgroup_size == 1024
    for s in range(len(mask)):
        _against_oracle(res, s, prob, *rows[s])

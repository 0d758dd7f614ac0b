"""simon_explain_own_batch on the device: every plugin family on arbitrary node subsets against the CPU oracle on each scenario's own
problem (explain_own_util), word and lane edges, presence rows that spell prefixes against simon_explain_batch, segmented batches,
pods flagged for eviction, refusals and state, and the two sweeps with reasons end to end.  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest

import evict_util as EU
import explain_own_util as OU
import mix_util as MU
import randprob
import subset_util as SU
from open_simulator_amd import capi, simulate as sim
from test_gpu_mix import _route_case
from test_gpu_subsets import _random_rows, _scen_of

pytestmark = pytest.mark.gpu

FIT, STATIC, REST, GPU, PORTS = capi.FAIL_FIT, capi.FAIL_STATIC, 0x2000, 0x1000, 0x0800


def _rand(seed, **kw):
    return lambda: (randprob.rand_problem(seed, **kw), None)


# case -> (problem and its orders (None: identity + one permutation), the name that seeds its rows, families the oracle must see)
CASES = {
    "a": (lambda: _route_case("gpu")[::2], "gpu", {GPU, FIT}),
    "b": (lambda: _route_case("anti")[::2], "anti", {REST, FIT}),
    "c": (_rand(21, N=48, P=240, static_mask=True, pins=True, gates=True, tight_pods=True), "static+pins", {STATIC, FIT}),
    "d": (_rand(7421, N=40, P=500, ports=True, anti_host=True, tight_pods=True, static_mask=True), "ports+anti_host", {PORTS, REST, FIT, STATIC}),
    # (scalars=4, P=600 makes 109 distinct (ephemeral storage, extended resource) requests; the score table holds 32 (kTableMaxXres) and the
    # batch would be the all-feature kernel's, which takes no own-nodes batch.  Two extended resources and 590 pods make 31.)
    "e": (_rand(11, N=70, P=590, tight_pods=True, scalars=2, eph=True), "scalars+eph", {FIT}),
    "f": (_rand(1, N=48, P=300, spread_soft=True, hard_simple=True, tight_pods=True, n_node_classes=3), 1, {REST}),
    "g": (lambda: _route_case("service_wave")[::2], "service_wave", set()),
}
LISTED = [5, 0, 7, 2, 1, 6, 3, 4, 1]          # every scenario, permuted, one repeat


@functools.lru_cache(maxsize=None)
def subset_case(name):
    """(problem, mask, zone, scen, orders, ranks) of a case: eight seeded rows over three zones."""
    make, seed, _ = CASES[name]
    prob, orders = make()
    prob, _ = MU.segmentable(prob, fixed=0)
    N = prob.n_nodes
    rng = np.random.default_rng(seed if isinstance(seed, int) else sum(map(ord, seed)))
    mask = _random_rows(rng, N)
    zone = rng.integers(0, 3, N).astype(np.int32)
    if orders is None:
        orders = np.stack([np.arange(prob.n_pods), rng.permutation(prob.n_pods)]).astype(np.int32)
    scen = _scen_of(mask, rng.integers(0, len(orders), len(mask)))
    return prob, mask, zone, scen, np.asarray(orders, np.int32), SU.zone_ranks(mask, zone)


def _loaded(ctx, prob, scen, orders, mask, zone):
    ctx.load_problem(prob)
    ctx.load_scenarios(scen, orders)
    ctx.set_scenario_nodes(mask, zone)


def _check_listed(ctx, listed, prob, mask, scen, orders, ranks, max_failed=64, max_bins=32):
    """explain_own_batch of `listed` with and without rows against the oracle; returns per listed scenario (n_failed, oracle rows)."""
    N = prob.n_nodes
    eb = ctx.explain_own_batch(listed, max_failed, max_bins, rows=True)
    assert eb.scenarios.tolist() == list(listed) and eb.rows.shape == (len(listed), max_failed, N)
    seen = {}
    for k, s in enumerate(listed):
        if s not in seen:
            seen[s] = OU.assert_explained(eb, k, prob, mask[s], orders[scen[s, 1]], None if ranks is None else ranks[s], max_failed, max_bins, True)
        else:                                                         # a repeat: the same answer once more
            k0 = list(listed).index(s)
            for f in ("n_failed", "failed_pods", "n_bins", "bins", "rows"):
                assert getattr(eb, f)[k].tobytes() == getattr(eb, f)[k0].tobytes(), (f, s)
    eb2 = ctx.explain_own_batch(listed, max_failed, max_bins)
    assert eb2.rows is None
    for f in ("n_failed", "failed_pods", "n_bins", "bins"):
        assert getattr(eb2, f).tobytes() == getattr(eb, f).tobytes(), f
    return seen


# ---- 1. every plugin family on arbitrary subsets -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [(n, {}) for n in sorted(CASES)] + [("e", {"SIMON_WG": "64"})], ids=sorted(CASES) + ["e_wg64"])
def test_every_plugin_family_on_arbitrary_subsets(name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name == "g":
        monkeypatch.setenv("SIMON_TEAM", "0")
    prob, mask, zone, scen, orders, ranks = subset_case(name)
    with capi.Context(0) as ctx:
        _loaded(ctx, prob, scen, orders, mask, zone)
        seen = _check_listed(ctx, LISTED, prob, mask, scen, orders, ranks)              # (before any run: the call needs none)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
    assert res.unscheduled.tolist() == [seen[s][0] for s in range(len(mask))]           # the replay counts what the run counted
    fams = set().union(*[OU.families(rows) for _, rows in seen.values()])
    print(name, "failed pods per scenario:", [seen[s][0] for s in range(len(mask))], "families:", sorted(hex(f) for f in fams))
    assert CASES[name][2] <= fams, sorted(hex(f) for f in fams)
    if name == "f":                                                                    # the per-scenario `registered` rule is exercised
        assert any((rows == capi.FAIL_SPREAD).any() for _, rows in seen.values())
    if name == "g":                                                                    # absent nodes in a lane's second iteration at T = 256
        assert prob.n_nodes == 512 and [s for s in range(len(mask)) if seen[s][0]] == [1] and seen[1][0] == 1178
    else:
        assert sum(1 for s in seen if seen[s][0]) >= 7


# ---- 2. word and lane edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [1, 3])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 65, 131])
def test_word_and_lane_edges(N, Z):
    prob, _ = MU.segmentable(randprob.rand_problem(N, N=N, P=40 + 4 * N, tight_pods=True, static_mask=True, n_node_classes=min(5, N)), fixed=0)
    zone = None if Z == 1 else (np.arange(N) * 7 % Z).astype(np.int32)
    mask = SU.staging_masks(N, zone, seed=N)
    assert mask.shape == (12, N)
    ranks = SU.zone_ranks(mask, zone)
    orders = np.arange(prob.n_pods, dtype=np.int32)[None]
    scen = _scen_of(mask)
    with capi.Context(0) as ctx:
        _loaded(ctx, prob, scen, orders, mask, zone)
        seen = _check_listed(ctx, list(range(12)), prob, mask, scen, orders, ranks, max_failed=16)
    failing = sum(1 for s in seen if seen[s][0] > 0)
    print(N, Z, [seen[s][0] for s in range(12)])
    assert failing >= 7 and (N != 1 or failing == 12)


# ---- 3. rows that spell prefixes ---------------------------------------------------------------------------------------------------------------
def test_rows_that_spell_prefixes_equal_explain_batch():
    prob, scen, orders = _route_case("gpu")
    prob, _ = MU.segmentable(prob, fixed=0)
    N = prob.n_nodes
    mask = np.arange(N)[None, :] < scen[:, :1]
    listed = [3, 0, 7, 1, 2, 6, 5, 4, 0]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        want = ctx.explain_batch(listed, 64, 32, rows=True, code_stride=N)
        ctx.set_scenario_nodes(mask)
        got = ctx.explain_own_batch(listed, 64, 32, rows=True)
    assert want.n_failed.any()
    for f in ("n_failed", "failed_pods", "n_bins", "bins"):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    for k, s in enumerate(listed):
        n = int(scen[s, 0])
        assert (got.rows[k, :, :n] == want.rows[k, :, :n]).all() and not got.rows[k, :, n:].any(), s


# ---- 4. segments ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gpu", "anti"])
def test_three_random_segments_against_the_oracle(case):
    prob, scen, orders = _route_case(case)
    prob, F = MU.segmentable(prob, scen)
    N, n_seg, S = prob.n_nodes, 3, 10
    rng = np.random.default_rng(n_seg)
    starts = np.sort(np.concatenate([[F], rng.choice(np.arange(F + 1, N), n_seg - 1, replace=False)])).astype(np.int32)
    ends = np.append(starts[1:], N)
    cnt = np.stack([rng.integers(0, ends[g] - starts[g] + 1, S) for g in range(n_seg)], 1).astype(np.int32)
    sc = np.stack([F + cnt.sum(1), rng.integers(0, len(orders), S)], 1).astype(np.int32)
    mask = np.stack([MU.present_mask(N, starts, cnt[s]) for s in range(S)])
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(sc, orders)
        ctx.set_scenario_segments(starts, cnt)
        seen = _check_listed(ctx, list(range(S - 1, -1, -1)), prob, mask, sc, orders, None)
        ctx.run_loaded(True)
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
        assert ctx.fetch(True).unscheduled.tolist() == [seen[s][0] for s in range(S)]
    assert any(seen[s][0] for s in seen)


# ---- 5. evicted pods ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gates", "gpu"])
def test_evicted_pods_are_explained_like_fresh_pods(case):
    prob, evict, mask, zone, scen, orders, ranks, rows = EU.route_case(case)
    N, S = prob.n_nodes, len(mask)
    huge = int(np.flatnonzero(evict & (np.asarray(prob.req_cpu) == np.asarray(prob.req_cpu)[evict].max()))[0])
    assert int(np.asarray(prob.req_cpu)[huge]) == 2 * int(np.asarray(prob.alloc_cpu).max())
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        eb = ctx.explain_own_batch(list(range(S)), 64, 32, rows=True)
    for s in range(S):
        ps, gone = EU.scenario_problem(prob, evict, mask[s])
        nf, _ = OU.assert_explained(eb, s, ps, mask[s], orders[scen[s, 1]], ranks[s], 64, 32, True)
        assert nf == int(rows[s][1].unscheduled[0])
        if s in (2, 4):
            assert gone[huge]
            failed = eb.failed_pods[s, :eb.recorded(s)].tolist()
            assert huge in failed
            row = eb.rows[s, failed.index(huge)]
            assert ((row[mask[s]] & FIT) != 0).all() and not row[~mask[s]].any()


# ---- 6. refusals and state ----------------------------------------------------------------------------------------------------------------------
def _rc(ctx, idx, max_failed=4, max_bins=8, stride=None):
    N = ctx.problem.n_nodes
    idx = np.ascontiguousarray(idx, np.int32)
    k = len(idx)
    stride = N if stride is None else stride
    bufs = [np.zeros(k, np.int32), np.zeros((k, max_failed), np.int32), np.zeros((k, max_failed), np.int32)]
    bins = np.zeros((k, max_failed, max_bins), capi.FAIL_BIN_DTYPE)
    codes = np.zeros((k, max_failed, max(stride, 1)), np.uint16)
    rc = ctx.lib.simon_explain_own_batch(ctx.h, capi._ptr(idx, capi.C.c_int32), k, max_failed, max_bins, *[capi._ptr(b, capi.C.c_int32) for b in bufs],
                                         bins.ctypes.data_as(capi.C.c_void_p), capi._ptr(codes, capi.C.c_uint16), stride)
    return rc, ctx.lib.simon_last_error(ctx.h).decode()


def test_refusals_and_state(monkeypatch):
    prob, mask, zone, scen, orders, ranks = subset_case("a")
    N = prob.n_nodes
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        ctx.run_loaded(True)
        fresh = ctx.fetch(True)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        assert _rc(ctx, [0])[0] == capi.ESTATE                                       # nothing loaded
        ctx.load_scenarios(scen, orders)
        rc, msg = _rc(ctx, [0])
        assert rc == capi.ESTATE and "use simon_explain_batch" in msg               # a prefix batch
        ctx.set_scenario_nodes(mask, zone)
        assert _rc(ctx, [0, len(mask)])[0] == capi.EINVAL and _rc(ctx, [-1])[0] == capi.EINVAL
        assert _rc(ctx, [0], stride=N - 1)[0] == capi.EINVAL
        assert _rc(ctx, [0], max_bins=capi.EXPLAIN_BINS + 1)[0] == capi.EINVAL and _rc(ctx, [0], max_failed=0)[0] == capi.EINVAL
        assert _rc(ctx, [0, 1])[0] == 0
        ctx.explain_own_batch([2, 1], 8, 8, rows=True)
        ctx.run_loaded(True)                                                          # the batch and its results are undisturbed
        after = ctx.fetch(True)
        assert (after.placement == fresh.placement).all() and after.unscheduled.tolist() == fresh.unscheduled.tolist()
        assert after.used_cpu.tolist() == fresh.used_cpu.tolist() and after.used_mem.tolist() == fresh.used_mem.tolist()
        ctx.explain_own_batch([0], 8, 8)
        again = ctx.fetch(True)                                                       # ... also without a run in between
        assert (again.placement == fresh.placement).all()
        ctx.set_scenario_nodes(None)
        ctx.load_scenarios(np.stack([np.sort(scen[:, 0]), scen[:, 1]], 1), orders)
        eb = ctx.explain_batch([0, 1], 8, 8)                                          # a prefix batch explains as before
        assert eb.n_failed.shape == (2,)
        assert _rc(ctx, [0])[0] == capi.ESTATE
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        rc, msg = _rc(ctx, [0])
        assert rc == capi.ESTATE and "node-subset batch" in msg


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------
def _no_replay(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("_failure_replay called")
    monkeypatch.setattr(sim, "_failure_replay", boom)


@pytest.mark.parametrize("reschedule", [False, "owned"])
def test_sweep_failures_reasons_on_the_device(reschedule, monkeypatch):
    if reschedule:
        cluster, apps = EU.live_cluster()
    else:
        cluster, apps, _ = MU.example_simple()
        apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    _no_replay(monkeypatch)
    ref = sim.sweep_failures(cluster, apps, "node", engine=OU.OwnSubsetOracleEngine(), reasons=True, reschedule=reschedule)
    eng = sim.HipEngine()
    hip = sim.sweep_failures(cluster, apps, "node", engine=eng, reasons=True, reschedule=reschedule)
    assert hip.batched and ref.batched and hip.fallback is None and eng.last_stats.kernel_variant == capi.KERNEL_NARROW_CACHE
    assert hip.unscheduled == ref.unscheduled and hip.placements == ref.placements and any(hip.unscheduled)
    assert hip.unscheduled_pods == ref.unscheduled_pods
    assert [len(lst) for lst in hip.unscheduled_pods] == hip.unscheduled


@pytest.mark.parametrize("daemonset", [True, False])
def test_sweep_mix_reasons_on_the_device(daemonset):
    """With the app's DaemonSet most failing mixes are listed from their own simulate() (simulate._same_stream); without it every failing
    mix is explained in the batch."""
    cluster, apps, types = MU.example_simple()
    if not daemonset:
        apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    counts = [[0, 1, 2], [0, 1, 3]]
    ref = sim.sweep_mix(cluster, apps, types, counts, engine=OU.OwnSegmentOracleEngine(), reasons=True)
    hip = sim.sweep_mix(cluster, apps, types, counts, engine=sim.HipEngine(), reasons=True)
    assert hip.batched and ref.batched and any(hip.unscheduled)
    assert (hip.unscheduled, hip.best, hip.cost) == (ref.unscheduled, ref.best, ref.cost)
    assert hip.unscheduled_pods == ref.unscheduled_pods

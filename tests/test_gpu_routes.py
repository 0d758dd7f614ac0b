"""One small problem per route of route_batch (simon_hip.hip): the result against the CPU oracle and the whole simon_stats tuple
(kernel_variant, kernel_generation, workgroup_size, slots_per_lane, lds_bytes, n_launches) against a literal.  The literals are what
the library of the commit before simon_run_loaded was split into route_batch and its launchers reports for these batches (every
figure of the tuple is decided on the host; the batches hold 6 scenarios, at most one per CU of any device with 6 CUs or more);
the ones that follow from the code: 256 threads and one slot for 70 nodes, 64 threads under SIMON_WG=64 (generation 1:
generation 2 starts at 128 threads), 64 * kTeamWaves = 256 threads in team mode, one wave and one 64-entry round otherwise.
A fresh context per case: the library reads its knobs once per context.  Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import randprob
from open_simulator_amd import capi

pytestmark = pytest.mark.gpu

N, P, S = 70, 200, 6
KNOBS = ("SIMON_NARROW_V1", "SIMON_NO_CACHE", "SIMON_WG", "SIMON_LDS_WS", "SIMON_TABLE_COARSE", "SIMON_TEAM", "SIMON_FORCE_WIDE")
PROBLEMS = {"plain": dict(), "gpu": dict(gpu=True, eph=True), "spread": dict(spread_soft=True), "local": dict(local=True),
            "static": dict(static_scores=True), "zero_cpu": dict()}
NARROW, WIDE, FAST, TABLE = capi.KERNEL_NARROW, capi.KERNEL_WIDE, capi.KERNEL_NARROW_FAST, capi.KERNEL_NARROW_CACHE


@functools.lru_cache(maxsize=None)
def _inputs(name, ranked=False):
    """(problem, 6 prefix scenarios of 40 .. 70 nodes over 2 orders, per-scenario node ranks or None, the oracle's result): once per
    problem, shared by its cases and left unchanged"""
    prob = randprob.rand_problem(23, N, P, **PROBLEMS[name])
    if name == "zero_cpu":                      # a node without allocatable CPU: no score table for the problem (its rows divide by the capacity)
        prob.alloc_cpu[5] = 0
    scen, orders = randprob.rand_scenarios(23, prob, S=S, n_orders=2, min_n=40)
    ranks = None
    if ranked:
        ranks = np.tile(np.arange(N, dtype=np.int32), (S, 1))
        for s in range(S):
            ranks[s, :scen[s, 0]] = np.random.default_rng(s).permutation(scen[s, 0])
    gpu = prob.gpu_mem is not None
    return prob, scen, orders, ranks, O.run(prob, scen, orders, node_ranks=ranks, want_gpu_slices=gpu)


# (id, problem, environment, node ranks, simon_stats)
CASES = [
    ("generation1", "plain", {"SIMON_NARROW_V1": "1", "SIMON_NO_CACHE": "1"}, False, (NARROW, 1, 256, 1, 128, 1)),
    ("generation2", "plain", {"SIMON_NO_CACHE": "1"}, False, (FAST, 2, 256, 1, 240, 1)),
    ("wg64", "plain", {"SIMON_WG": "64", "SIMON_NO_CACHE": "1"}, False, (NARROW, 1, 64, 2, 128, 1)),
    ("generation4_hbm", "plain", {"SIMON_LDS_WS": "0"}, False, (TABLE, 4, 64, 1, 592, 1)),
    ("generation4_ldsws", "plain", {}, False, (TABLE, 4, 64, 1, 2816, 1)),
    ("generation5", "plain", {"SIMON_TABLE_COARSE": "1"}, False, (TABLE, 5, 64, 1, 432, 1)),
    ("generation6_ldsx", "gpu", {}, False, (TABLE, 6, 64, 1, 4480, 1)),
    ("generation6_hbm", "gpu", {"SIMON_LDS_WS": "0"}, False, (TABLE, 6, 64, 1, 1072, 1)),
    ("generation7_wave", "spread", {"SIMON_TEAM": "0"}, False, (TABLE, 7, 64, 1, 7312, 1)),
    ("generation7_team", "spread", {"SIMON_TEAM": "1"}, False, (TABLE, 7, 256, 1, 9744, 1)),
    ("wide_forced", "plain", {"SIMON_FORCE_WIDE": "1"}, False, (WIDE, 0, 256, 0, 0, 1)),
    ("wide_local_storage", "local", {}, False, (WIDE, 0, 256, 0, 0, 1)),
    ("wide_ranks_without_table", "zero_cpu", {}, True, (WIDE, 0, 256, 0, 0, 1)),
]


def _set_env(monkeypatch, env):
    for k in KNOBS:                             # (the suite alternates SIMON_LDS_WS by test id: a case's environment is its own)
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_same(res, ref, gpu):
    assert (res.placement == ref.placement).all()
    assert res.unscheduled.tolist() == ref.unscheduled.tolist()
    assert res.used_cpu.tolist() == ref.used_cpu.tolist() and res.used_mem.tolist() == ref.used_mem.tolist()
    if gpu:
        assert (res.gpu_slices == ref.gpu_slices).all()


def _stats(ctx):
    st = ctx.stats()
    return (st.kernel_variant, st.kernel_generation, st.workgroup_size, st.slots_per_lane, st.lds_bytes, st.n_launches)


@pytest.mark.parametrize("name,problem,env,ranked,stats", CASES, ids=[c[0] for c in CASES])
def test_route(name, problem, env, ranked, stats, monkeypatch):
    prob, scen, orders, ranks, ref = _inputs(problem, ranked)
    gpu = prob.gpu_mem is not None
    _set_env(monkeypatch, env)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        if ranks is not None:
            ctx.set_node_ranks(ranks)
        ctx.run_loaded(True, gpu)
        got = _stats(ctx)
        print(name, got)
        res = ctx.fetch(True, gpu)
    assert got == stats
    _assert_same(res, ref, gpu)


def test_segmented_batch_is_refused_on_the_all_feature_kernel_and_the_context_lives_on(monkeypatch):
    """A problem only the all-feature kernel takes (NodePreferAvoidPods-sized additions): a segmented batch is refused before anything
    is launched, and a prefix batch on the same context then runs."""
    prob, scen, orders, _, ref = _inputs("static")
    _set_env(monkeypatch, {})
    F = N - 16
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 9, (S, 2)).astype(np.int32)
    seg = np.stack([F + cnt.sum(1), scen[:, 1]], 1).astype(np.int32)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(seg, orders)
        ctx.set_scenario_segments([F, F + 8], cnt)
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE
        assert "run_loaded: segmented batch on a problem the score-table kernel does not take; run each scenario's own problem" in str(e.value)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True)
        got = _stats(ctx)
        print("after the refusal", got)
        res = ctx.fetch(True)
    assert got == (WIDE, 0, 256, 0, 0, 1)
    _assert_same(res, ref, False)

"""Pod eviction on the device (simon_set_pod_eviction): a node-subset batch with flagged pods -- bound where their node is present,
scheduled like fresh pods where it is not -- against the unmodified CPU oracle on every scenario's OWN problem (evict_util), pod by
pod, on every score-table route; flagged pods on the edges of the 64-pod chunks and of the 32-node presence words; the refusals and
the state machine; preempt-risk flags; sweep_failures(reschedule=...) against the oracle engine.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import evict_util as EU
import mix_util as MU
import randprob
import subset_util as SU
from open_simulator_amd import capi, simulate as sim

pytestmark = pytest.mark.gpu


def _run(prob, evict, mask, zone, scen, orders, want_gpu=False):
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        if evict is not None:
            ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(mask, zone)
        ctx.run_loaded(True, want_gpu)
        res = ctx.fetch(True, want_gpu)
        if prob.priority is not None:
            res.preempt_risk = ctx.fetch_preempt_risk()
        return res, ctx.stats()


def _compare(res, rows, mask, want_gpu=False):
    """Device rows against the oracle's, pod by pod; returns (evicted pods placed, evicted pods unscheduled) as the DEVICE has them."""
    placed = failed = 0
    for s, (row, ref, gone) in enumerate(rows):
        got = res.placement[s]
        assert got.tolist() == row.tolist(), (s, np.flatnonzero(got != row)[:8].tolist())
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), s
        if want_gpu:
            assert (res.gpu_slices[s] == ref.gpu_slices[0]).all(), s
        assert mask[s][got[got >= 0]].all(), s                        # nobody lands on an absent node
        assert (got[gone] != capi.GATED).all(), s                     # an evicted pod is part of the scenario
        placed += int((got[gone] >= 0).sum())
        failed += int((got[gone] == capi.UNSCHEDULED).sum())
    return placed, failed


# (case, environment, generation, threads per scenario): the score-table routes of test_gpu_mix.ROUTES plus a problem with more than 64
# request signatures; the LDS homes of generations 4 and 6 by name and through conftest's alternation of SIMON_LDS_WS
ROUTES = [("gates_fine", {"SIMON_TABLE_COARSE": "0"}, 4, 64),
          ("gates_coarse", {"SIMON_TABLE_COARSE": "1"}, 5, 64),
          ("config3_fine_lds", {"SIMON_TABLE_COARSE": "0", "SIMON_LDS_WS": "1"}, 4, 64),
          ("many_sigs", {"SIMON_TABLE_COARSE": "0"}, 4, 64),
          ("classes160", {}, 4, 64),
          ("gpu_fold", {}, 5, 64),
          ("gpu_lds", {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "1"}, 6, 64),
          ("gpu_hbm", {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "0"}, 6, 64),
          ("anti", {}, 6, 64),
          ("service_wave", {"SIMON_TEAM": "0"}, 7, 64),
          ("service_team", {"SIMON_TEAM": "1"}, 7, 256)]


@pytest.mark.parametrize("case,env,gen,wg", ROUTES, ids=[r[0] for r in ROUTES])
def test_flagged_pods_match_the_oracle_on_every_route(case, env, gen, wg, monkeypatch):
    """evict_util.route_case: flagged pods from as many pod classes as there are (REST descriptors in `anti`, soft-spread descriptors in
    `service_*`, GPU requests in `gpu_*`) on three nodes, one of them over-committed by a bound pod that fits nowhere once evicted; eight
    scenarios over three zones with per-scenario orders: every node (its rows equal the batch without flags), without one flagged node,
    without all of them, three other nodes alone, four random rows."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, evict, mask, zone, scen, orders, ranks, rows = EU.route_case(case)
    want_gpu = prob.gpu_mem is not None
    pre = np.asarray(prob.preset_node)
    huge = int(np.flatnonzero(evict)[np.argmax(np.asarray(prob.req_cpu)[evict])])
    assert prob.req_cpu[huge] > prob.alloc_cpu.max() and mask[0].all() and not mask[2][pre[evict]].any() and mask[3].sum() == 3
    if case == "anti":
        assert any(prob.anti_off[c + 1] > prob.anti_off[c] for c in np.asarray(prob.pod_class)[evict])
    if case.startswith("service"):
        assert any(prob.spread_soft_off[c + 1] > prob.spread_soft_off[c] for c in np.asarray(prob.pod_class)[evict])
    if case == "many_sigs":
        assert len({(int(prob.req_cpu[p]), int(prob.req_mem[p]), int(prob.pod_class[p])) for p in range(prob.n_pods)}) > 64
    want = EU.evicted_counts(rows)
    assert want[0] > 0 and want[1] > 0                                # the oracle alone: evicted pods placed, evicted pods unscheduled
    res, st = _run(prob, evict, mask, zone, scen, orders, want_gpu)
    assert (st.kernel_variant, st.kernel_generation, st.workgroup_size) == (capi.KERNEL_NARROW_CACHE, gen, wg)
    assert _compare(res, rows, mask, want_gpu) == want
    assert int(res.placement[0][huge]) == pre[huge] and (res.placement[2][huge], res.placement[1][huge]) == (capi.UNSCHEDULED, pre[huge])
    # the scenario that loses no node, without flags: the same rows
    plain, _ = _run(prob, None, mask[:1], zone, scen[:1], orders, want_gpu)
    assert (plain.placement[0] == res.placement[0]).all() and int(plain.unscheduled[0]) == int(res.unscheduled[0])
    assert (int(plain.used_cpu[0]), int(plain.used_mem[0])) == (int(res.used_cpu[0]), int(res.used_mem[0]))


def _edge_case(N, P):
    """Flagged pods at stream positions 0, 63, 64 and P - 1 of the identity order (63 | 64: neighbours across a chunk boundary; P = 65: 64
    is the only pod of the last chunk), preset to the nodes of presence bits 31 and 32 where the pool has them (else its last two
    nodes); a reversed and a shuffled order move them; pod 64 fits nowhere once evicted."""
    prob, _ = MU.segmentable(randprob.rand_problem(100 * N + P, N=N, P=P, n_node_classes=min(5, N), nz_differs=True), fixed=0)
    a = min(31, N - 1)
    b = 32 if N > 32 else a - 1
    where = {0: a, 63: a, 64: b, P - 1: b}
    if N > 64:
        where[1] = 64
    prob, evict = EU.flag(prob, where, huge=64)
    rng = np.random.default_rng(N + P)
    orders = np.stack([np.arange(P), np.arange(P)[::-1], rng.permutation(P)]).astype(np.int32)
    full = np.ones(N, bool)
    rnd = rng.random(N) < 0.6
    rnd[[a, 0]] = [False, True]
    mask = np.stack([full, full, full, full, full, full, full, rnd])
    for s, lost in enumerate(([], [a], [b], [a, b], [a], [b], [a, b])):
        mask[s, lost] = False
    if N > 64:
        mask[3, 64] = False
    scen = np.stack([mask.sum(1), [0, 0, 0, 0, 1, 2, 2, 1]], 1).astype(np.int32)
    zone = (np.arange(N) % 2).astype(np.int32) if N >= 32 else None
    ranks = SU.zone_ranks(mask, zone)
    return prob, evict, mask, zone, scen, orders, ranks, EU.oracle_rows(prob, evict, mask, scen, orders, ranks, restricted=(3, 7))


@pytest.mark.parametrize("P", [65, 130])
@pytest.mark.parametrize("N", [31, 32, 33, 65])
def test_flagged_pods_on_chunk_and_word_edges(N, P):
    prob, evict, mask, zone, scen, orders, ranks, rows = _edge_case(N, P)
    want = EU.evicted_counts(rows)
    assert want[0] > 0 and want[1] > 0
    res, st = _run(prob, evict, mask, zone, scen, orders)
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation in (4, 5)
    assert _compare(res, rows, mask) == want
    plain, _ = _run(prob, None, mask[:1], zone, scen[:1], orders)
    assert (plain.placement[0] == res.placement[0]).all()


def _expect(rc, code, ctx, match):
    assert rc == code, (rc, ctx.lib.simon_last_error(ctx.h))
    assert match in ctx.lib.simon_last_error(ctx.h).decode()


def test_refusals_and_the_state_machine():
    """SIMON_EINVAL: a flag on a pod without preset, a flag on a gated pod; SIMON_ESTATE: the call while a subset or segmented batch is
    loaded.  After each the context still runs a prefix batch.  Without flags the ungated absent preset is refused in the old words;
    simon_load_pods clears the flags; a prefix batch that lacks a flagged pod's node waits for its node rows."""
    prob, evict, mask, zone, scen, orders, ranks, rows = EU.route_case("gates_fine")
    N, P = prob.n_nodes, prob.n_pods
    u8 = lambda a: capi._ptr(np.ascontiguousarray(a, np.uint8), capi.C.c_uint8)   # noqa: E731
    pre, gate = np.asarray(prob.preset_node), np.asarray(prob.gate_node)
    free = int(np.flatnonzero((pre < 0) & (gate < 0))[0])
    gated = int(np.flatnonzero(gate >= 0)[0])
    top = int(pre[evict].max())
    prefix = np.array([[N, 0], [top + 1, 1]], np.int32)               # prefix scenarios that hold every preset target
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ref = ctx.run_batch(prefix, orders)

        def still_runs():
            ctx.load_scenarios(prefix, orders)
            ctx.run_loaded(True)
            out = ctx.fetch(True)
            assert (out.placement == ref.placement).all() and out.unscheduled.tolist() == ref.unscheduled.tolist()

        bad = np.zeros(P, np.uint8)
        bad[free] = 1
        _expect(ctx.lib.simon_set_pod_eviction(ctx.h, u8(bad)), capi.EINVAL, ctx, "not preset")
        still_runs()
        gated_prob = EU.replaced(prob, preset_node=np.where(np.arange(P) == gated, gate[gated], pre).astype(np.int32))
        ctx.load_problem(gated_prob)
        bad = np.zeros(P, np.uint8)
        bad[gated] = 1
        _expect(ctx.lib.simon_set_pod_eviction(ctx.h, u8(bad)), capi.EINVAL, ctx, "gated")
        ctx.load_problem(prob)
        still_runs()
        # without flags: the old refusal, word for word; the batch stays a prefix batch
        ctx.load_scenarios(scen[:3], orders)
        with pytest.raises(capi.SimonError, match="absent from some scenario, and not gated on it") as e:
            ctx.set_scenario_nodes(mask[:3], zone)
        assert e.value.code == capi.EINVAL
        still_runs()
        # with flags: accepted; while the subset batch is loaded the flags cannot change
        ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen[:3], orders)
        ctx.set_scenario_nodes(mask[:3], zone)
        _expect(ctx.lib.simon_set_pod_eviction(ctx.h, u8(evict)), capi.ESTATE, ctx, "node-subset")
        _expect(ctx.lib.simon_set_pod_eviction(ctx.h, None), capi.ESTATE, ctx, "node-subset")
        ctx.run_loaded(True)
        assert _compare(ctx.fetch(True), rows[:3], mask[:3])[0] > 0
        ctx.set_scenario_nodes(None)
        still_runs()                                                  # (the flags are inert in a prefix batch that holds every target)
        ctx.load_scenarios(prefix, orders)
        ctx.set_scenario_segments([top + 1], (prefix[:, :1] - (top + 1)).astype(np.int32))
        _expect(ctx.lib.simon_set_pod_eviction(ctx.h, None), capi.ESTATE, ctx, "segmented")
        ctx.run_loaded(True)
        seg = ctx.fetch(True)
        assert (seg.placement == ref.placement).all()
        # a prefix batch that lacks a flagged pod's node loads, but runs only once its node rows have arrived
        short = np.array([[top, 0]], np.int32)
        ctx.load_scenarios(short, orders)
        with pytest.raises(capi.SimonError, match="flagged for eviction") as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE
        still_runs()
        ctx.set_pod_eviction(None)                                    # detached: the prefix rule refuses at load time again
        with pytest.raises(capi.SimonError, match="gate it") as e:
            ctx.load_scenarios(short, orders)
        assert e.value.code == capi.EINVAL
        ctx.set_pod_eviction(evict)
        ctx.load_problem(prob)                                        # simon_load_pods clears the flags
        ctx.load_scenarios(scen[:3], orders)
        with pytest.raises(capi.SimonError, match="not gated on it"):
            ctx.set_scenario_nodes(mask[:3], zone)
        still_runs()
        with pytest.raises(ValueError, match="shape"):
            ctx.set_pod_eviction(np.ones(P + 1, bool))


def test_preempt_risk_of_an_evicted_pod_that_fails():
    prob, evict, mask, zone, scen, orders, ranks, _ = EU.route_case("gates_fine")
    rng = np.random.default_rng(5)
    prio = rng.integers(0, 3, prob.n_pods).astype(np.int32)
    huge = int(np.flatnonzero(evict)[np.argmax(np.asarray(prob.req_cpu)[evict])])
    prio[huge] = 10
    prob = EU.replaced(prob, priority=prio)
    rows = EU.oracle_rows(prob, evict, mask, scen, orders, ranks)
    want = [int(ref.preempt_risk[0]) for _, ref, _ in rows]
    assert want[2] == 1 and rows[2][0][huge] == capi.UNSCHEDULED and want[0] == 0      # evicted, failed, lower priorities placed before it
    res, _ = _run(prob, evict, mask, zone, scen, orders)
    _compare(res, rows, mask)
    assert res.preempt_risk.tolist() == want


@pytest.mark.parametrize("which", ["owned", "all"])
def test_rescheduling_sweep_on_the_device_equals_the_oracle_engine(which):
    cluster, apps = EU.live_cluster()
    eng = sim.HipEngine()
    hip = sim.sweep_failures(cluster, apps, "node", engine=eng, reschedule=which, reasons=True)
    ref = sim.sweep_failures(cluster, apps, "node", engine=EU.EvictOracleEngine(), reschedule=which, reasons=True)
    assert hip.batched and ref.batched and hip.fallback is None
    assert eng.last_stats.kernel_variant == capi.KERNEL_NARROW_CACHE
    assert hip.placements == ref.placements and hip.domains == ref.domains
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.vg_pct, hip.survives, hip.needs_reference, hip.baseline, hip.critical, hip.removable,
            hip.evicted, hip.evicted_unscheduled) == \
           (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.vg_pct, ref.survives, ref.needs_reference, ref.baseline, ref.critical, ref.removable,
            ref.evicted, ref.evicted_unscheduled)
    assert sum(hip.evicted) > sum(hip.evicted_unscheduled) > 0
    names = lambda lists: [[(u["pod"]["metadata"]["name"], u["reason"]) for u in lst] for lst in lists]   # noqa: E731
    assert names(hip.unscheduled_pods) == names(ref.unscheduled_pods)
    assert [w for w, _ in EU.evicted_answers(cluster, apps, hip.domains, which)] == hip.placements

"""GPU parity tests of the score-table step's memory waits (round 10): the winner's node state loaded ahead of its table row, the pod
stream's chunk boundaries (a chunk of 64 steps is loaded ahead of the chunk that runs; a two-stage form of the stream was built against these
tests, measured slower and not kept: profiles/experiments/r10_step_waits.md), the placement flush, and the one read-back per plan.  The CPU
oracle is the expected result everywhere; the plan tests recompute the parent's values from the fetched results."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import randprob
from open_simulator_amd import capi
from test_gpu_cycle_paths import HBM_WS, run_on_table, tie_problem, ties_in_oracle
from test_gpu_parity import assert_same, run_gpu

pytestmark = pytest.mark.gpu

ONE_LEVEL = dict(HBM_WS, SIMON_TABLE_COARSE="0")          # the base unit's one-level straight-line instantiations
N_NODES = 40
EDGES = (0, -1, 63, 64, 127, 128)                          # first step, last step, the chunk edges
KINDS = ("gated", "preset", "pinned")


def chunk_problem(P, **feat):
    """P pods of six requests on 40 nodes of three shapes (node j: class j % 3).  The first min(P, 6) pod ids are special, kind i % 3: gated
    on node 39 (part of the 40-node scenarios only), preset to a node, pinned to a node."""
    N = N_NODES
    rng = np.random.default_rng(1000 + P)
    shape_cpu, shape_mem = np.array([8000, 16000, 32000]), np.array([16, 32, 64]) << 30
    ncls = (np.arange(N) % 3).astype(np.int32)
    sig = rng.integers(0, 6, P)
    preset, gate, pin = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    for i in range(min(P, 6)):
        kind = KINDS[i % 3]
        if kind == "gated":
            gate[i] = N - 1
        elif kind == "preset":
            preset[i] = gate[i] = 1 + i                    # (a preset pod is gated on its own node)
        else:
            pin[i] = 4 + i
    prob = capi.Problem(alloc_cpu=shape_cpu[ncls].astype(np.int64), alloc_mem=shape_mem[ncls].astype(np.int64), alloc_pods=np.full(N, 6, np.int32),
                        node_class=ncls, req_cpu=(500 + 250 * sig).astype(np.int64), req_mem=((256 + 128 * sig) << 20).astype(np.int64),
                        pod_class=np.zeros(P, np.int32), n_pod_classes=1, n_node_classes=3,
                        simon_raw=np.array([[30, 60, 10]], np.int64), const_score=np.full(1, 1000300, np.int64))
    prob.preset_node, prob.gate_node, prob.pin_node = preset, gate, pin
    return prob.normalise()


def chunk_orders(P):
    """Four orders -- ascending, descending and two random permutations of the plain pods -- with the special pods at the first, the last and
    the chunk-edge steps; order o rotates the kinds over those steps, so that every kind meets every edge the stream is long enough for."""
    n_special = min(P, 6)
    steps = sorted({e % P for e in EDGES if -P <= e < P})[:n_special]
    plain = np.arange(n_special, P)
    fills = [plain, plain[::-1], np.random.default_rng(P).permutation(plain), np.random.default_rng(P + 1).permutation(plain)]
    orders = []
    for o, fill in enumerate(fills):
        order = np.full(P, -1, np.int64)
        special = list(np.roll(np.arange(n_special), o))
        at = list(steps)
        while len(at) < n_special:                         # (a stream too short for every edge: the spare special pods go anywhere free)
            at.append(next(i for i in range(P) if i not in at))
        order[at] = special
        order[order < 0] = fill
        assert sorted(order.tolist()) == list(range(P))
        orders.append(order)
    return np.array(orders, np.int32), steps


CHUNK_REF = {}


def chunk_case(P):
    """problem, scenarios, orders and the oracle's result, computed once per P"""
    if P not in CHUNK_REF:
        prob = chunk_problem(P)
        orders, steps = chunk_orders(P)
        scen = np.array([[n, o] for o in range(4) for n in (20, 39, 40)], np.int32)
        CHUNK_REF[P] = (prob, scen, orders, steps, O.run(prob, scen, orders))
    return CHUNK_REF[P]


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 128, 129, 191, 193])
def test_pod_chunk_boundaries(P):
    """Stream lengths around the 64-step chunk, rare pods on the first, the last and the chunk-edge steps, four orders."""
    prob, scen, orders, steps, ref = chunk_case(P)
    # the special pods do sit on the edges, and they take their paths in the oracle's result
    special = set(range(min(P, 6)))
    for order in orders:
        assert all(int(order[s]) in special for s in steps)
    if P >= 6:
        gated = [i for i in range(6) if KINDS[i % 3] == "gated"]
        preset = [i for i in range(6) if KINDS[i % 3] == "preset"]
        small = scen[:, 0] < N_NODES
        assert (ref.placement[small][:, gated] == -2).all() and (ref.placement[~small][:, gated] > -2).all()
        assert (ref.placement[:, preset] == np.asarray(prob.preset_node)[preset]).all()
    if P >= 127:
        assert (ref.unscheduled[scen[:, 0] == 20] > 0).all()          # 20 nodes x 6 pods: the tail of the stream finds a full cluster
    res = run_on_table(prob, scen, orders, env=ONE_LEVEL)
    assert_same(res, ref)


ROUTES = {                                                 # features -> generation of the kernel that must run
    "rest": (dict(gpu=True, anti_host=True, presets=True, gates=True, pins=True), 6, {"SIMON_NO_FOLD": "1", "SIMON_NO_GPU_FOLD": "1"}),
    "spread": (dict(spread_soft=True, presets=True, gates=True, pins=True), 7, {}),
}


@pytest.mark.parametrize("P", [65, 129])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_pod_chunks_on_the_rest_and_spread_routes(route, P, monkeypatch):
    """The same stream lengths, rare pods included, through the per-node filters (generation 6) and the spread walks (generation 7)."""
    feat, generation, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = randprob.rand_problem(8800 + P, N=N_NODES, P=P, **feat)
    scen, orders = randprob.rand_scenarios(P, prob, S=6)
    ref = O.run(prob, scen, orders)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders)
        st = ctx.stats()
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation == generation, (st.kernel_variant, st.kernel_generation)
    assert_same(res, ref)


@pytest.mark.parametrize("P", [129, 193])
def test_pod_chunks_with_more_than_128_signatures(P):
    """The MANY instantiations (further signature groups) take more than 128 signatures, so a stream of at least 129 pods with a request each:
    65 pods cannot reach them.  P = 129 is the shortest; 193 ends one step behind a chunk edge as well."""
    N = N_NODES
    rng = np.random.default_rng(P)
    prob = capi.Problem(alloc_cpu=np.full(N, 64000, np.int64), alloc_mem=np.full(N, 256 << 30, np.int64), alloc_pods=np.full(N, 4, np.int32),
                        node_class=(np.arange(N) % 3).astype(np.int32), req_cpu=(100 + 7 * rng.permutation(P)).astype(np.int64),
                        req_mem=np.full(P, 64 << 20, np.int64), pod_class=np.zeros(P, np.int32), n_pod_classes=1, n_node_classes=3,
                        simon_raw=np.array([[30, 60, 10]], np.int64), const_score=np.full(1, 1000300, np.int64))
    preset = np.full(P, -1, np.int32)
    preset[[0, P - 1]] = [3, 5]
    prob.preset_node = preset
    prob.gate_node = np.where(preset >= 0, preset, -1).astype(np.int32)
    prob.gate_node[[1, P - 2]] = N - 1
    prob.normalise()
    orders = np.stack([np.arange(P), np.arange(P)[::-1], np.roll(np.arange(P), 64)]).astype(np.int32)
    scen = np.array([[n, o] for o in range(3) for n in (20, N)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.unscheduled[scen[:, 0] == 20] > 0).all() and (ref.placement[scen[:, 0] == 20][:, [1, P - 2]] == -2).all()
    assert_same(run_on_table(prob, scen, orders, env=HBM_WS), ref)


@pytest.mark.parametrize("last", [1, 64])
def test_every_step_is_recorded(last):
    """A stream whose last chunk holds `last` steps: every step's record reaches the placement row, and the count of unscheduled pods is the
    number of -1 entries of the fetched row."""
    P = 128 + last
    prob, scen, orders, _, ref = chunk_case(P)
    res, _ = run_gpu(prob, scen, orders, env=ONE_LEVEL)
    assert_same(res, ref)
    assert (res.placement >= -2).all() and (res.placement < N_NODES).all()
    assert ((res.placement == -1).sum(axis=1) == res.unscheduled).all()
    assert (res.unscheduled > 0).any()
    with capi.Context(0) as ctx:                           # the row as simon_fetch_placement hands it out
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True)
        counts = ctx.fetch(False).unscheduled
        for s in range(len(scen)):
            row = ctx.fetch_placement(s)
            assert (row == ref.placement[s]).all() and int((row == -1).sum()) == int(counts[s])


# ---- the state ahead of the row -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n_classes", [(2, 1), (17, 1), (17, 2)])
def test_consecutive_pods_on_one_node_and_one_block(N, n_classes):
    """200 pods on 2 nodes, or on 17 nodes of one shape: consecutive pods land on the same node and on nodes of the same 16-position block,
    so a cycle loads the state and the row its predecessor has just stored.  Two caller classes of one shape tie across classes: the
    speculated winner loses to the canonical order and state, row and byte are loaded a second time."""
    P = 200
    prob = tie_problem(N, P, n_classes, 6)
    prob.alloc_pods = np.full(N, 110, np.int32)
    prob.normalise()
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(N).permutation(P).astype(np.int32)])
    scen = np.array([[n, o] for n in sorted({1, N - 1, N}) for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    for s, (n, o) in enumerate(scen.tolist()):
        row = ref.placement[s][orders[o]]
        placed = row[row >= 0]
        assert (placed[1:] == placed[:-1]).any() or n > 2, (n, o)          # the same node twice in a row
        assert ((placed[1:] >> 4) == (placed[:-1] >> 4)).mean() > 0.5           # ... and the same block, most of the time
        if n_classes == 2 and n > 2:
            assert ties_in_oracle(prob, n, orders[o], ref.placement[s])[1] > 0   # the canonical cross-class tie-break fires
    assert_same(run_on_table(prob, scen, orders, env=ONE_LEVEL), ref)


# ---- one read-back per plan ---------------------------------------------------------------------------------------------------------
def parent_plan(prob, scen, res, present=None, caps=(100, 100)):
    """simon_min_plan as the parent computed it, from the fetched counts and sums: the smallest feasible scenario (node count, then index),
    its sums, and the percentages over the allocatable of its own nodes."""
    ac_all, am_all = np.asarray(prob.alloc_cpu, np.int64), np.asarray(prob.alloc_mem, np.int64)
    best = None
    for s, (n, o) in enumerate(np.asarray(scen).tolist()):
        if res.unscheduled[s] != 0:
            continue
        mask = np.arange(prob.n_nodes) < n if present is None else np.asarray(present[s], bool)
        ac, am = int(ac_all[mask].sum()), int(am_all[mask].sum())
        uc, um = int(res.used_cpu[s]), int(res.used_mem[s])
        cpu, mem = int(float(uc) / float(ac) * 100.0), int(float(um * 1000) / float(am * 1000) * 100.0)
        if cpu > caps[0] or mem > caps[1]:
            continue
        if best is None or (n, s) < (best["n_nodes"], best["scenario"]):
            best = dict(found=1, scenario=s, n_nodes=n, order_id=o, cpu_pct=cpu, mem_pct=mem, used_cpu=uc, used_mem=um)
    return best


def device_key(ctx, caps=(100, 100)):
    import torch
    d_key, stream = C.c_void_p(), C.c_void_p()
    assert ctx.lib.simon_min_plan_device(ctx.h, caps[0], caps[1], 100, C.byref(d_key), C.byref(stream)) == 0 and d_key.value
    torch.cuda.synchronize()
    key = torch.empty(1, dtype=torch.int64)
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(key.data_ptr()), d_key, C.c_size_t(8), C.c_int(2)) == 0        # hipMemcpyDeviceToHost
    return int(key.item())


def check_plans(ctx, prob, scen, res, present=None, caps_list=((100, 100),)):
    found = set()
    for caps in caps_list:
        want = parent_plan(prob, scen, res, present, caps)
        plan = ctx.min_plan(*caps)
        plan_vg, vg = ctx.min_plan_vg(caps[0], caps[1], 100)
        key = device_key(ctx, caps)
        found.add(want is not None)
        if want is None:
            assert plan.found == 0 and plan.scenario == -1 and plan_vg.found == 0 and key == -1, caps      # (the key: all ones)
            continue
        for got in (plan, plan_vg):
            d = got.as_dict()
            assert {k: d[k] for k in want} == want, (caps, d, want)
        assert vg == 0 and key == (want["n_nodes"] << 32 | want["scenario"])
    return found


def test_plan_record_found_none_and_ties():
    """Plan found; ties on the node count across orders (the lower scenario index wins); caps that leave no plan; a batch in which every
    scenario leaves pods unscheduled."""
    from open_simulator_amd import synth
    prob, scen, orders = synth.config3(n_counts=8, n_orders=3, n_pods=600, n_het=40)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders)
        feasible = np.flatnonzero(res.unscheduled == 0)
        n_best = scen[feasible, 0].min()
        assert (scen[feasible, 0] == n_best).sum() >= 2, "the batch must tie on the node count across orders"
        found = check_plans(ctx, prob, scen, res, caps_list=((100, 100), (60, 100), (100, 50), (1, 1)))
        assert found == {True, False}
        assert O.min_plan(prob, scen, res).as_dict() == ctx.min_plan().as_dict()
    prob = chunk_problem(193)                               # 40 nodes x 6 pods hold at most 240, but the requests fill them earlier
    orders, _ = chunk_orders(193)
    scen = np.array([[n, o] for o in range(4) for n in (5, 10)], np.int32)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders)
        assert (res.unscheduled > 0).all()
        assert check_plans(ctx, prob, scen, res) == {False}


def test_plan_record_on_an_own_nodes_batch():
    """Node-subset scenarios: the allocatable sums come from each scenario's own nodes."""
    prob = chunk_problem(65)
    prob.preset_node = prob.gate_node = prob.pin_node = None   # (plain pods: every subset may hold them)
    prob.normalise()
    N = prob.n_nodes
    rng = np.random.default_rng(5)
    present = rng.random((6, N)) < 0.7
    present[0] = True
    present[1, : N // 2] = False
    orders = np.stack([np.arange(65), np.arange(65)[::-1]]).astype(np.int32)
    scen = np.array([[int(present[s].sum()), s % 2] for s in range(6)], np.int32)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(present)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        assert (res.unscheduled == 0).any()
        assert check_plans(ctx, prob, scen, res, present=present, caps_list=((100, 100), (30, 100))) >= {True}

"""GPU parity tests of the plain pod's scheduling cycle in the score-table kernel (round 13): in the straight-line kernels whose workspace is in
HBM every lane stores the touched node's state (no EXEC region around one lane's store, and no wait for that store in front of the refresh);
the round also tried other address forms for the selector table, the state and the winner's class, which were not kept.  What those touch is
what the cases aim at: both bodies of the fused kernel in one launch, the 64-step chunk edges, cross-class ties, classes emptying, pods that
fit nowhere, the cold branch next to plain pods, both homes of the workspace and two signatures per lane.  Every case compares every placement
row, the unscheduled count and the used cpu / memory of every scenario with the CPU oracle, and first counts, in the oracle's own result, the
events it aims at."""
import re

import numpy as np
import pytest

import oracle_lib as O
from open_simulator_amd import synth
from test_gpu_cycle_paths import HBM_WS, rejoin_orders, rejoin_problem, run_on_table, tie_problem, ties_in_oracle
from test_gpu_eager_rebase import SIZES, batch, check_events, emptying_problem
from test_gpu_parity import assert_same
from test_gpu_step_waits import KINDS, N_NODES, chunk_case

pytestmark = pytest.mark.gpu

ENV = dict(HBM_WS, SIMON_TABLE_COARSE="0", SIMON_DEBUG_ROUTE="1")          # the base unit's one-level kernels, workspace in HBM
ROUTE = re.compile(r"\[route\] unit (\S+) .*? entries/lane (\d) \(own size: ([^)]*)\)")
_CASES = {}


def routed(prob, scen, orders, capfd, env):
    """run_on_table and (unit, entries per lane, own-size note) of the launch's route line"""
    capfd.readouterr()
    res = run_on_table(prob, scen, orders, env=env)
    route = ROUTE.findall(capfd.readouterr().err)
    assert len(route) == 1, route
    return res, route[0]


# ---- both bodies of the fused kernel in one launch ----------------------------------------------------------------------------------------
def config3_pool():
    """Config 3's pool (488 existing nodes in four shapes + new nodes of the template) with 400 pods; cluster sizes around 1 000 and 1 040
    nodes, two orders each: some scenarios pad to at most 1 024 positions, some to more."""
    if "c3" not in _CASES:
        prob, scen, orders = synth.config3(n_counts=600, n_orders=2, n_pods=400)
        sizes = (600, 985, 1000, 1005, 1038, 1040, 1045, 1087)
        scen = np.ascontiguousarray(scen[np.isin(scen[:, 0], sizes)])
        assert len(scen) == 2 * len(sizes)
        _CASES["c3"] = (prob, scen, orders, O.run(prob, scen, orders))
    return _CASES["c3"]


@pytest.mark.parametrize("dispatch", ["own-size", "off"])
def test_config3_pool_on_both_bodies(dispatch, capfd):
    prob, scen, orders, ref = config3_pool()
    assert (ref.placement >= 0).sum() > 0.9 * ref.placement.size
    res, (unit, entries, own) = routed(prob, scen, orders, capfd, dict(ENV, **({"SIMON_NO_SIZE_DISPATCH": "1"} if dispatch == "off" else {})))
    assert unit == "simon_table" and entries == "2", (unit, entries)
    if dispatch == "off":
        assert own == "off", own
    else:
        m = re.fullmatch(r"(\d+) of (\d+) scenarios at 1", own)
        assert m and 0 < int(m.group(1)) < int(m.group(2)) == len(scen), own      # both bodies run in this launch
    assert_same(res, ref)


# ---- chunk edges, the cold branch next to plain pods, a cluster that fills up ------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_chunk_edges(P):
    """Stream lengths around the 64-step chunk: the record of the last step of a chunk and of the first of the next, with gated, preset and
    pinned pods on those steps (four orders rotate the kinds) between plain ones."""
    prob, scen, orders, steps, ref = chunk_case(P)
    special = set(range(min(P, 6)))
    assert all(int(order[s]) in special for order in orders for s in steps)
    if P >= 6:
        preset = [i for i in range(6) if KINDS[i % 3] == "preset"]
        gated = [i for i in range(6) if KINDS[i % 3] == "gated"]
        assert (ref.placement[:, preset] == np.asarray(prob.preset_node)[preset]).all()
        assert (ref.placement[scen[:, 0] < N_NODES][:, gated] == -2).all()
        assert (ref.placement[:, 6:] >= 0).any()
    if P >= 129:
        assert (ref.unscheduled[scen[:, 0] == 20] > 0).all()                      # 20 nodes x 6 pod slots: free slots reach 0, the tail fits nowhere
    assert_same(run_on_table(prob, scen, orders, env=dict(HBM_WS, SIMON_TABLE_COARSE="0")), ref)


@pytest.mark.parametrize("pins", [False, True], ids=["preset+gated", "preset+gated+pinned"])
def test_unschedulable_pods_in_mid_stream(pins):
    """Pods that fit no node (a FitError between plain pods, the state unchanged), presets, gates and pins at the head of the stream and on the
    chunk edge; pods behind an unschedulable one are placed as if it had not been there."""
    prob, kinds = rejoin_problem(9100 + pins, pins)
    P = prob.n_pods
    orders, _ = rejoin_orders(kinds, P, pins)
    scen = np.array([[n, o] for o in range(len(orders)) for n in (40, 62, 70)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.placement[:, kinds["huge"]] == -1).all() and all(0 < u < P for u in ref.unscheduled.tolist())
    assert (ref.placement[scen[:, 0] <= 62][:, kinds["gated"]] == -2).all()
    for s, (n, o) in enumerate(scen.tolist()):
        row = ref.placement[s, orders[o]]
        first = int(np.flatnonzero(row == -1)[0])
        assert (row[first + 1:] >= 0).sum() > 20, s                                  # plain pods land behind the first FitError
    assert_same(run_on_table(prob, scen, orders, env=dict(HBM_WS, SIMON_TABLE_COARSE="0")), ref)


# ---- cross-class ties --------------------------------------------------------------------------------------------------------------------------
def test_cross_class_ties_on_many_cycles(capfd):
    """Two caller classes of one shape, interleaved in canonical order and kept apart (SIMON_TABLE_NO_CLASS_CONTENT): untouched nodes tie on
    the total across the classes, and while both classes hold one the tie check sends the cycle to the canonical tie-break -- on a third of
    the cycles and more in the scenarios with more nodes than pods (config 3: 0.2 %).  Scenarios on each body of the fused kernel."""
    N, P = 1100, 150
    prob = tie_problem(N, P, 2, 6)
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(N).permutation(P).astype(np.int32)])
    scen = np.array([[n, o] for n in (33, 1009, N) for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.unscheduled == 0).all()
    for s, (n, o) in enumerate(scen.tolist()):
        by_position, cross_class = ties_in_oracle(prob, n, orders[o], ref.placement[s])
        assert by_position > 0 and cross_class > 0, (n, o)                           # ... and position order would have chosen otherwise
        # cycles whose winner is an untouched node while the OTHER class still holds one: its entries reach the same total, the tie check fires
        ncls, used, fired = np.asarray(prob.node_class)[:n], np.zeros(n, bool), 0
        for pod in orders[o]:
            j = ref.placement[s, pod]
            fired += bool(not used[j] and (~used & (ncls != ncls[j])).any())
            used[j] = True
        if n > 2 * P:
            assert fired >= P // 3, (n, o, fired)                                    # (config 3: 0.2 % of the cycles)
    res, (unit, entries, own) = routed(prob, scen, orders, capfd, dict(ENV, SIMON_TABLE_NO_CLASS_CONTENT="1"))
    assert unit == "simon_table" and entries == "2" and own == "4 of 6 scenarios at 1", (unit, entries, own)
    assert_same(res, ref)


# ---- class emptying ------------------------------------------------------------------------------------------------------------------------
# (seed: the first of 0, 1, 2, ... for which check_events' three conditions hold in every scenario and an event falls on the last step of a chunk)
EMPTY_SEED = {(4, 8): 21, (4, 5): 9, (4, 12): 1}


def emptying_case(n_classes, n_sigs, seed, **feat):
    key = (n_classes, n_sigs, seed, tuple(sorted(feat.items())))
    if key not in _CASES:
        sizes, slots = SIZES[n_classes], (1, 2, 1, 3)[:n_classes]
        prob, sig = emptying_problem(seed, sizes, n_sigs, max(n_sigs, int(np.dot(sizes, slots))) + 40, slots, **feat)
        scen, orders = batch(prob)
        _CASES[key] = (prob, sig, scen, orders, O.run(prob, scen, orders))
    return _CASES[key]


def on_chunk_end(events):
    return any(step % 64 == 63 for ev in events for step, _, _ in ev)


@pytest.mark.parametrize("n_classes,n_sigs", list(EMPTY_SEED))
def test_classes_emptying(n_classes, n_sigs, capfd):
    """Few small nodes per class, Simon raw scores that differ per class (a missed re-base moves a placement): counters of several (signature,
    class) pairs reach 0 mid-stream, two rows in one cycle among them, one on the last step of a chunk; pods of a signature that lost every class
    are unschedulable."""
    prob, sig, scen, orders, ref = emptying_case(n_classes, n_sigs, EMPTY_SEED[n_classes, n_sigs])
    events = check_events(prob, sig, scen, orders, ref)                              # (asserts the three conditions per scenario)
    assert on_chunk_end(events) and (ref.unscheduled > 0).all()
    assert len({tuple(r) for r in np.asarray(prob.simon_raw).T.tolist()}) == n_classes
    res, (unit, _, _) = routed(prob, scen, orders, capfd, ENV)
    assert unit == "simon_table"
    assert_same(res, ref)


# ---- more than 64 signatures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sigs,n_pod_classes,no_twins", [(70, 1, False), (128, 2, False), (128, 2, True)], ids=["K70", "K128-twins", "K128-twins-off"])
def test_two_signatures_per_lane(n_sigs, n_pod_classes, no_twins, capfd):
    """KQ = 2: the refresh runs per register; every signature meets an emptied class."""
    prob, sig, scen, orders, ref = emptying_case(4, n_sigs, 100 + n_sigs, n_pod_classes=n_pod_classes)
    for events in check_events(prob, sig, scen, orders, ref, all_three=False):
        assert {k for _, k, _ in events} == set(range(n_sigs))
    assert (ref.unscheduled > 0).all()
    res, (unit, _, _) = routed(prob, scen, orders, capfd, dict(ENV, **({"SIMON_TABLE_NO_TWINS": "1"} if no_twins else {})))
    assert unit == "simon_table"
    assert_same(res, ref)


# ---- both workspace homes ----------------------------------------------------------------------------------------------------------------------
def test_workspace_in_lds_and_in_hbm(capfd, monkeypatch):
    """One small scenario: table and state in LDS by default (simon_table_lds.hip, where lane 0 keeps the store), in HBM with SIMON_LDS_WS=0."""
    prob, sig, scen, orders, _ = emptying_case(4, 8, EMPTY_SEED[4, 8])
    one = scen[:1]
    ref = O.run(prob, one, orders)
    assert check_events(prob, sig, one, orders, ref) and ref.unscheduled[0] > 0
    monkeypatch.delenv("SIMON_LDS_WS", raising=False)
    res, (unit, _, _) = routed(prob, one, orders, capfd, {"SIMON_DEBUG_ROUTE": "1", "SIMON_TABLE_COARSE": "0"})
    assert unit == "simon_table_lds"
    assert_same(res, ref)
    res, (unit, _, _) = routed(prob, one, orders, capfd, ENV)
    assert unit == "simon_table"
    assert_same(res, ref)

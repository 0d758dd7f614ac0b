"""GPU parity tests of what the score-table kernel's cycle records and scans: the placement record is written one lane per step into a
register that is flushed every 64 steps, so pods the cycle does not place (unschedulable: -1, not part of the scenario: -2) are put on the
chunk's edges; and the scan key is built from 1, 2 or 4 summary entries per lane, so the same pod stream runs on clusters of every entry
count with an initial state that makes totals tie inside a lane's entries and across lanes.  Generations 4 / 5 only, the oracle is the
expected result, and every test first checks on the oracle's result that the case it aims at occurs."""
import numpy as np
import pytest

import oracle_lib as O
from open_simulator_amd import capi
from test_gpu_cycle_paths import HBM_WS, run_on_table
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

HUGE_CPU = 10_000_000                    # milli-cores: fits no node
GATE = 62                                # a gated pod is part of the scenarios of more than 62 nodes only


def two_class_problem(N, P, req_cpu, req_mem, init_cpu=None, init_mem=None):
    """N nodes in two node classes of different shapes (node j: class j % 2), one pod class."""
    ncls = (np.arange(N) % 2).astype(np.int32)
    prob = capi.Problem(alloc_cpu=np.where(ncls == 0, 32000, 48000).astype(np.int64),
                        alloc_mem=np.where(ncls == 0, 64 << 30, 96 << 30).astype(np.int64), alloc_pods=np.full(N, 250, np.int32),
                        node_class=ncls, req_cpu=np.asarray(req_cpu, np.int64), req_mem=np.asarray(req_mem, np.int64),
                        pod_class=np.zeros(P, np.int32), n_pod_classes=1, n_node_classes=2,
                        simon_raw=np.full((1, 2), 50, np.int64), const_score=np.full(1, 1000300, np.int64))
    if init_cpu is not None:
        prob.init_req_cpu = np.asarray(init_cpu, np.int64)
        prob.init_req_mem = np.asarray(init_mem, np.int64)
        prob.init_nz_cpu = prob.init_req_cpu.copy()
        prob.init_nz_mem = prob.init_req_mem.copy()
        prob.init_npods = np.ones(N, np.int32)
    return prob


# ---- chunk edges of the placement record ------------------------------------------------------------------------------------------------
KINDS = ("huge", "gated", "both")        # -1 everywhere | -2 up to GATE nodes, placed beyond | -2 up to GATE nodes, -1 beyond


def edge_steps(P):
    return sorted({s for s in (0, 63, 64, P - 1) if 0 <= s < P})


def edge_case(P):
    """P pods whose first ones are of the rare kinds (four of each; the single pod of P = 1 is huge AND gated), and three orders that rotate
    the kinds over the steps 0, 63, 64 and P - 1; every other pod is drawn at random into the steps between."""
    cpu = 100 + 10 * (np.arange(P) % 6)
    mem = (64 + (np.arange(P) % 6)) << 20
    gate = np.full(P, -1, np.int32)
    if P == 1:
        pods = {"both": [0]}
    else:
        pods = {k: list(range(4 * i, 4 * i + 4)) for i, k in enumerate(KINDS)}
    for k, ids in pods.items():
        if k in ("huge", "both"):
            cpu[ids] = HUGE_CPU
        if k in ("gated", "both"):
            gate[ids] = GATE
    prob = two_class_problem(70, P, cpu, mem)
    prob.gate_node = gate
    prob.normalise()
    steps = edge_steps(P)
    orders, kinds_at = [], []
    for o in range(1 if P == 1 else 3):
        pool = {k: list(v) for k, v in pods.items()}
        order = [None] * P
        kinds = {}
        for i, step in enumerate(steps):
            kinds[step] = "both" if P == 1 else KINDS[(i + o) % 3]
            order[step] = pool[kinds[step]].pop()
        placed = {p for p in order if p is not None}
        rest = list(np.random.default_rng(100 * P + o).permutation([p for p in range(P) if p not in placed]))
        for step in range(P):
            if order[step] is None:
                order[step] = rest.pop()
        assert sorted(order) == list(range(P))
        orders.append(order)
        kinds_at.append(kinds)
    return prob, np.array(orders, np.int32), kinds_at


@pytest.mark.parametrize("coarse", ["0", "1"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 128, 130])
def test_unplaced_pods_on_the_edges_of_the_record(P, coarse):
    prob, orders, kinds_at = edge_case(P)
    scen = np.array([[n, o] for o in range(len(orders)) for n in (40, 62, 63, 70)], np.int32)
    ref = O.run(prob, scen, orders)
    seen = set()
    for s, (n, o) in enumerate(scen.tolist()):                    # the oracle's result holds -1 and -2 at those steps
        for step, kind in kinds_at[o].items():
            got = int(ref.placement[s, orders[o][step]])
            want = -1 if kind == "huge" else (-2 if n <= GATE else (-1 if kind == "both" else None))
            assert got == want if want is not None else got >= 0, (P, n, o, step, kind, got)
            seen.add(got if got < 0 else 0)
        if P > 12:
            assert (ref.placement[s] >= 0).sum() >= P - 12           # every plain pod lands
    assert {-1, -2} <= seen
    assert_same(run_on_table(prob, scen, orders, env=dict(HBM_WS, SIMON_TABLE_COARSE=coarse)), ref)


# ---- the scan key at 1, 2 and 4 entries per lane ----------------------------------------------------------------------------------------
def entries(n):
    """summary entries of 16 positions of an n-node prefix of the two interleaved classes (each padded to 16)"""
    return (((n + 1) // 2 + 15) // 16) + ((n // 2 + 15) // 16)


def scan_case(N):
    """The 130-pod stream of six small requests on N nodes whose initial state repeats with period 6 over the nodes -- three levels per
    node class: nodes 6 apart tie, in one summary entry (16 positions of a class are 32 nodes), in the entries of one lane (64 entries
    apart) and across lanes.  The least loaded level is what the pods fill first, so its ties are the ones the scan decides."""
    P = 130
    cpu = 100 + 10 * (np.arange(P) % 6)
    mem = (64 + (np.arange(P) % 6)) << 20
    level = (np.arange(N) // 2) % 3
    prob = two_class_problem(N, P, cpu, mem, init_cpu=1000 + 4000 * level, init_mem=(2 + 8 * level).astype(np.int64) << 30)
    return prob.normalise()


def position_ties(prob, n, order, row):
    """Steps at which the chosen node still held its initial state while a LATER node of the same class and initial level did as well: the
    totals tie and the position decides -- counted per distance of the two nodes in summary entries of 16 positions: same entry, another
    entry, an entry of the SAME lane (lane l scans entries l, l + 64, l + 128, ...: a multiple of 64 entries apart inside the class's
    segment) and an entry of another lane."""
    ncls = np.asarray(prob.node_class)[:n]
    init = np.asarray(prob.init_req_cpu)[:n]
    used = np.zeros(n, bool)
    same_entry = other_entry = same_lane = other_lane = 0
    for pod in order:
        j = int(row[pod])
        if j < 0:
            continue
        if not used[j]:
            later = np.flatnonzero(~used[j + 1:] & (ncls[j + 1:] == ncls[j]) & (init[j + 1:] == init[j])) + j + 1
            same_entry += bool((later // 32 == j // 32).any())
            other_entry += bool((later // 32 != j // 32).any())
            apart = later // 32 - j // 32                       # node j is index j // 2 of its class: 32 nodes per entry
            same_lane += bool(((apart > 0) & (apart % 64 == 0)).any())
            other_lane += bool((apart % 64 != 0).any())
        used[j] = True
    return same_entry, other_entry, same_lane, other_lane


@pytest.mark.parametrize("coarse", ["0", "1"])
@pytest.mark.parametrize("N,per_lane", [(70, 1), (1100, 2), (2100, 4)])
def test_scan_key_with_tied_totals_at_every_entry_count(N, per_lane, coarse):
    assert (entries(N) + 63) // 64 == {1: 1, 2: 2, 4: 3}[per_lane]       # 65 .. 128 entries: two per lane; 129 .. 256: four
    prob = scan_case(N)
    P = prob.n_pods
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(N).permutation(P).astype(np.int32)])
    counts = [N, N - 7, max(48, N // 2 + 1)]
    scen = np.array([[n, o] for n in counts for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.unscheduled == 0).all()
    for s, (n, o) in enumerate(scen.tolist()):
        same_entry, other_entry, same_lane, other_lane = position_ties(prob, n, orders[o], ref.placement[s])
        assert same_entry > 0 and other_entry > 0 and other_lane > 0, (n, o, same_entry, other_entry, other_lane)
        if n > 2 * 64 * 16:                                          # a class of more than 64 entries: ties between entries b and b + 64 of one lane
            assert same_lane > 0, (n, o)
    assert per_lane < 4 or counts[0] > 2 * 64 * 16
    assert_same(run_on_table(prob, scen, orders, env=dict(HBM_WS, SIMON_TABLE_COARSE=coarse)), ref)

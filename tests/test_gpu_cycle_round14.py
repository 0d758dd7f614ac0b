"""GPU parity tests of the score-table kernel's refresh (round 14): in the one-level straight-line kernels the evaluation hands out its fit as a
mask of the wave apart from its value -- the new byte is one select on `fit & (old byte != 0)`, every lane whose old byte is not 0 refreshes,
and "a byte dropped to 0" is `(old != 0) & ~fit` -- and the LeastAllocated terms are saturating converts instead of a convert behind a select
on `requested >= capacity`.  The cases aim at what that touches: nodes requested far beyond their capacity, (signature, node) pairs the static
mask excludes while the evaluation fits, classes emptying for several signatures at once and for signatures 0 and 63, two signatures per lane
with and without twins, both bodies of the fused kernel in one launch, and the 64-step chunk edges.  Every case compares every placement row,
the unscheduled count and the used cpu / memory of every scenario with the CPU oracle, and first finds, in the oracle's own result, the
events it aims at."""
import numpy as np
import pytest

import oracle_lib as O
import randprob
from open_simulator_amd import capi, synth
from test_gpu_cycle_paths import HBM_WS
from test_gpu_cycle_round13 import ENV, emptying_case, routed
from test_gpu_eager_rebase import check_events
from test_gpu_parity import assert_same
from test_gpu_step_waits import KINDS, N_NODES, chunk_case

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
ONE_LEVEL = {"SIMON_TABLE_COARSE": "0"}
WORKSPACES = {"hbm": dict(HBM_WS, **ONE_LEVEL), "lds": ONE_LEVEL}                 # (small batches default to the LDS-resident workspace)
_CASES = {}


# ---- nodes requested far beyond their capacity ----------------------------------------------------------------------------------------------
def overcommitted_case():
    """48 nodes of three shapes with coprime capacities, 160 pods.  The first 36 pods are bound by Spec.NodeName, two to each of nodes 0 .. 17,
    each asking 1.3 x the node's cpu (nodes 0 .. 5), memory (6 .. 11) or both (12 .. 17): Requested ends at 2.6 x allocatable, r - cap > cap.
    A third of the others ask nothing (NonZeroRequested counts 100m / 200 MiB for them): they pass NodeResourcesFit on those nodes, and in the
    scenarios of 8 and 18 nodes they have nowhere else to go."""
    if "over" not in _CASES:
        N, P, B = 48, 160, 36
        shape = np.arange(N) % 3
        alloc_cpu = np.array([3989, 7993, 16001], np.int64)[shape]
        alloc_mem = (np.array([8, 16, 32], np.int64) * GiB + np.array([3, 7, 11], np.int64) * MiB)[shape]
        rng = np.random.default_rng(14)
        req_cpu = rng.choice([100, 250, 330], P).astype(np.int64)
        req_mem = (rng.choice([64, 100, 257], P) * MiB).astype(np.int64)
        zero = np.arange(P) % 3 == 0
        req_cpu[zero] = 0
        req_mem[zero] = 0
        preset = np.full(P, -1, np.int32)
        for i in range(B):
            j = i // 2
            preset[i] = j
            req_cpu[i] = alloc_cpu[j] * 13 // 10 if j < 6 or j >= 12 else 100
            req_mem[i] = alloc_mem[j] * 13 // 10 // MiB * MiB if j >= 6 else 64 * MiB
        prob = capi.Problem(alloc_cpu=alloc_cpu, alloc_mem=alloc_mem, alloc_pods=np.full(N, 30, np.int32), node_class=shape.astype(np.int32),
                            req_cpu=req_cpu, req_mem=req_mem, nz_cpu=np.where(req_cpu == 0, 100, req_cpu).astype(np.int64),
                            nz_mem=np.where(req_mem == 0, 200 * MiB, req_mem).astype(np.int64), pod_class=np.zeros(P, np.int32),
                            preset_node=preset, gate_node=preset.copy(), n_pod_classes=1, n_node_classes=3,
                            simon_raw=np.array([[10, 50, 90]], np.int64), const_score=np.full(1, 1000300, np.int64)).normalise()
        head = np.arange(B, dtype=np.int32)
        orders = np.stack([np.arange(P, dtype=np.int32), np.concatenate([head, B + np.random.default_rng(3).permutation(P - B).astype(np.int32)])])
        scen = np.array([[8, 0], [18, 1], [30, 0], [48, 1]], np.int32)
        _CASES["over"] = (prob, scen, orders, O.run(prob, scen, orders), B)
    return _CASES["over"]


UNIT = {"hbm": ("simon_table",), "lds": ("simon_table", "simon_table_lds")}     # (a problem the LDS-resident kernels do not take stays in the base unit)


def on_one_level(prob, scen, orders, capfd, ws):
    """the run, after asserting that the launch went to the one-level kernels of the base unit or of its LDS-resident twin"""
    res, (unit, _, _) = routed(prob, scen, orders, capfd, dict(WORKSPACES[ws], SIMON_DEBUG_ROUTE="1"))
    assert unit in UNIT[ws], (ws, unit)
    return res


@pytest.mark.parametrize("ws", list(WORKSPACES))
def test_overcommitted_nodes(ws, capfd):
    prob, scen, orders, ref, B = overcommitted_case()
    ac, am = np.asarray(prob.alloc_cpu), np.asarray(prob.alloc_mem)
    rc, rm = np.asarray(prob.req_cpu), np.asarray(prob.req_mem)
    for s, (n, o) in enumerate(scen.tolist()):
        row = ref.placement[s]
        bound = np.flatnonzero((np.asarray(prob.preset_node) >= 0) & (np.asarray(prob.preset_node) < n))
        assert (row[bound] == np.asarray(prob.preset_node)[bound]).all()
        uc, um = np.zeros(n, np.int64), np.zeros(n, np.int64)
        np.add.at(uc, row[bound], rc[bound])
        np.add.at(um, row[bound], rm[bound])
        over_c, over_m = uc - ac[:n] > ac[:n], um - am[:n] > am[:n]                  # r - cap > cap before the first scheduled pod
        assert over_c.any() and (over_m.any() or n <= 6), (n, over_c.sum(), over_m.sum())
        zero_pods = np.flatnonzero((rc == 0) & (rm == 0) & (row >= 0))
        landed = row[zero_pods]
        if n <= 18:                                                                   # every node of the scenario is over-committed
            assert (over_c | over_m).all() and len(landed) > 10, n                    # ... and pods that ask nothing land there
    assert (over_c & over_m).any()                                                    # (the largest scenario holds nodes 12 .. 17: both at once)
    assert_same(on_one_level(prob, scen, orders, capfd, ws), ref)


# ---- the static mask: the evaluation fits, the byte stays 0 ---------------------------------------------------------------------------------------
def masked_case():
    """60 nodes with three to eleven pod slots and a static mask that excludes a fifth of the (pod class, node) pairs; 200 pods."""
    if "mask" not in _CASES:
        prob = randprob.rand_problem(1414, N=60, P=200, static_mask=True, tight_pods=True, n_node_classes=3, n_pod_classes=6).normalise()
        P = prob.n_pods
        orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(5).permutation(P).astype(np.int32)])
        scen = np.array([[60, 0], [60, 1], [41, 0], [17, 1]], np.int32)
        _CASES["mask"] = (prob, scen, orders, O.run(prob, scen, orders))
    return _CASES["mask"]


@pytest.mark.parametrize("ws", list(WORKSPACES))
def test_static_mask_keeps_the_byte_at_zero(ws, capfd):
    prob, scen, orders, ref = masked_case()
    mask = np.asarray(prob.static_mask)
    allowed = lambda c, j: bool((int(mask[c, j >> 6]) >> (j & 63)) & 1)              # noqa: E731
    pcls, rc, rm = np.asarray(prob.pod_class), np.asarray(prob.req_cpu), np.asarray(prob.req_mem)
    ac, am, ap = np.asarray(prob.alloc_cpu), np.asarray(prob.alloc_mem), np.asarray(prob.alloc_pods)
    for s, (n, o) in enumerate(scen.tolist()):
        uc, um, up, hits, full = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), 0, 0
        for pod in orders[o]:
            j = int(ref.placement[s, pod])
            if j < 0:
                continue
            assert allowed(int(pcls[pod]), j)
            uc[j] += rc[pod]; um[j] += rm[pod]; up[j] += 1
            # the touched node is re-evaluated for every signature: pod classes the mask excludes from it while their request still fits ...
            for c in range(prob.n_pod_classes):
                if not allowed(c, j):
                    k = np.flatnonzero(pcls == c)[0]
                    hits += bool(up[j] < ap[j] and uc[j] + rc[k] <= ac[j] and um[j] + rm[k] <= am[j])
            full += bool(up[j] == ap[j])                                              # ... and nodes that leave every signature at once
        assert hits > 10 and full > 0, (n, o, hits, full)
    assert (ref.unscheduled > 0).any()
    assert_same(on_one_level(prob, scen, orders, capfd, ws), ref)


# ---- classes emptying ---------------------------------------------------------------------------------------------------------------------------
def test_classes_emptying_for_signatures_0_and_63(capfd):
    """64 signatures, one per lane: counters of (signature, class) pairs reach 0, several in one cycle, those of the first and the last lane among them."""
    prob, sig, scen, orders, ref = emptying_case(4, 64, 1464)
    per_scen = check_events(prob, sig, scen, orders, ref, all_three=False)
    for events in per_scen:
        assert {0, 63} <= {k for _, k, _ in events}
        assert max(np.bincount([step for step, _, _ in events])) >= 2                 # one cycle empties a class for several signatures
    assert (ref.unscheduled > 0).all()
    res, (unit, _, _) = routed(prob, scen, orders, capfd, ENV)
    assert unit == "simon_table"
    assert_same(res, ref)


@pytest.mark.parametrize("no_twins", [False, True], ids=["twins", "twins-off"])
def test_classes_emptying_with_two_signatures_per_lane(no_twins, capfd):
    """KQ = 2: with twins the upper slot takes the lower slot's value AND fit mask; without them it evaluates its own."""
    prob, sig, scen, orders, ref = emptying_case(4, 128, 228, n_pod_classes=2)
    for events in check_events(prob, sig, scen, orders, ref, all_three=False):
        assert {k for _, k, _ in events} == set(range(128))
        assert max(np.bincount([step for step, _, _ in events])) >= 2
    assert (ref.unscheduled > 0).all()
    res, (unit, _, _) = routed(prob, scen, orders, capfd, dict(ENV, **({"SIMON_TABLE_NO_TWINS": "1"} if no_twins else {})))
    assert unit == "simon_table"
    assert_same(res, ref)


# ---- both bodies of the fused kernel in one launch --------------------------------------------------------------------------------------------
def blocks_of(prob, n):
    """summary entries of 16 positions of the prefix scenario of n nodes: every internal node class (caller class x shape) padded to 16"""
    key = np.stack([np.asarray(prob.node_class)[:n], np.asarray(prob.alloc_cpu)[:n], np.asarray(prob.alloc_mem)[:n]], 1)
    _, counts = np.unique(key, axis=0, return_counts=True)
    return int(((counts + 15) // 16).sum())


def two_body_case():
    """Config 3's pool with 400 pods; cluster sizes that pad to 65, 66, 96 and 97 entries (two per lane, the last two around the pitch of the
    full benchmark batch) and to 64 and fewer (one per lane), two orders each."""
    if "c3" not in _CASES:
        prob, scen, orders = synth.config3(n_counts=1064, n_orders=2, n_pods=400)
        sizes = np.unique(scen[:, 0])
        by_blocks = {}
        for n in sizes.tolist():
            by_blocks.setdefault(blocks_of(prob, n), n)                                # the smallest size of every entry count
        want = (40, 63, 64, 65, 66, 96, 97)
        picked = [by_blocks[b] for b in want if b in by_blocks]
        assert {65, 66, 96, 97} <= set(by_blocks) and 64 in by_blocks, sorted(by_blocks)
        scen = np.ascontiguousarray(scen[np.isin(scen[:, 0], picked)])
        assert len(scen) == 2 * len(picked)
        _CASES["c3"] = (prob, scen, orders, O.run(prob, scen, orders), len(picked))
    return _CASES["c3"]


@pytest.mark.parametrize("dispatch", ["own-size", "off"])
def test_both_bodies_in_one_launch(dispatch, capfd):
    import re
    prob, scen, orders, ref, n_sizes = two_body_case()
    assert (ref.placement >= 0).sum() > 0.9 * ref.placement.size
    res, (unit, entries, own) = routed(prob, scen, orders, capfd, dict(ENV, **({"SIMON_NO_SIZE_DISPATCH": "1"} if dispatch == "off" else {})))
    assert unit == "simon_table" and entries == "2", (unit, entries)
    if dispatch == "off":
        assert own == "off", own
    else:
        m = re.fullmatch(r"(\d+) of (\d+) scenarios at 1", own)
        assert m and int(m.group(1)) == 2 * (n_sizes - 4) and int(m.group(2)) == len(scen), own      # sizes of 64 entries and fewer on the one-entry body
    assert_same(res, ref)


# ---- chunk edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 64, 65])
def test_chunk_edges(P, capfd):
    """Stream lengths 63 / 64 / 65: gated, preset and pinned pods on the first steps, the last step of a chunk and the first of the next."""
    prob, scen, orders, steps, ref = chunk_case(P)
    preset = [i for i in range(6) if KINDS[i % 3] == "preset"]
    gated = [i for i in range(6) if KINDS[i % 3] == "gated"]
    assert all(int(order[s]) in set(range(6)) for order in orders for s in steps)
    assert (ref.placement[:, preset] == np.asarray(prob.preset_node)[preset]).all()
    assert (ref.placement[scen[:, 0] < N_NODES][:, gated] == -2).all()
    assert (ref.placement[:, 6:] >= 0).any()
    assert_same(on_one_level(prob, scen, orders, capfd, "hbm"), ref)

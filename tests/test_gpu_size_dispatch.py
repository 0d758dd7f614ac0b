"""GPU parity tests of the score table's entries-per-lane by scenario size (round 11): in a one-level, unranked launch whose largest scenario
needs two summary entries per lane, a scenario of at most 1 024 padded positions runs the kernel's one-entry body (simon_table.hip:
table_kernel, LO).  Every batch runs three ways -- each scenario by its own size, SIMON_NO_SIZE_DISPATCH=1 (every scenario scans the launch's
two entries, as before round 11) and its own size behind the per-scenario prologue -- and the CPU oracle is the expected result of all three.
The padded sizes are computed here, from the class counts of a prefix, and the library's route line (SIMON_DEBUG_ROUTE) must count the same
scenarios on the one-entry body."""
import re

import numpy as np
import pytest

import oracle_lib as O
from open_simulator_amd import capi
from test_gpu_cycle_paths import HBM_WS, run_on_table, tie_problem, ties_in_oracle
from test_gpu_parity import assert_same
from test_gpu_step_waits import KINDS, chunk_orders

pytestmark = pytest.mark.gpu

ENV = dict(HBM_WS, SIMON_TABLE_COARSE="0", SIMON_DEBUG_ROUTE="1")          # the base unit's one-level kernels, workspace in HBM
WAYS = {"own": {}, "off": {"SIMON_NO_SIZE_DISPATCH": "1"}, "own, per-scenario prologue": {"SIMON_NO_SHARED_PROLOGUE": "1"}}
MiB, GiB = 1 << 20, 1 << 30
N_POOL = 1100
N_LOADED = 962               # nodes below it start half full: the emptiest nodes of every large scenario are its last ones
ONE_ENTRY = 1024             # padded positions one entry per lane covers (64 lanes x 16 positions)
N_CLS = 3


def padded(ncls, n, n_classes=N_CLS):
    """padded class-major size of the prefix scenario of n nodes: every class segment is rounded up to a summary entry of 16 positions"""
    return int((((np.bincount(ncls[:n], minlength=n_classes) + 15) // 16) * 16).sum())


def positions(ncls, n, n_classes=N_CLS):
    """class-major position of every node of the prefix (classes in the order of their first node, as the library numbers them)"""
    counts = np.bincount(ncls[:n], minlength=n_classes)
    seg = np.concatenate([[0], np.cumsum((counts + 15) // 16 * 16)])
    rank = np.zeros(n, np.int64)
    for c in range(n_classes):
        rank[ncls[:n] == c] = np.arange(counts[c])
    return seg[ncls[:n]] + rank


def size_with(ncls, want, n_classes=N_CLS):
    """the smallest prefix whose padded size is `want`"""
    hits = [n for n in range(1, len(ncls) + 1) if padded(ncls, n, n_classes) == want]
    assert hits, want
    return hits[0]


def pool_problem(P, n_sigs=7, special=False, nz=False):
    """1 100 nodes in three shapes (node j: class j % 3, so no class count of the sizes below is a multiple of 16 by design), the largest shape
    last in class-major order; the nodes below N_LOADED start half full, so pods prefer the last nodes of a large scenario -- the largest
    shape's among them sit at positions >= 1 024.  P pods of n_sigs requests, every one used.  special: the first six pod ids are gated,
    preset and pinned pods (kind i % 3), one of each on a node every scenario but the smallest holds and one on a node of the last class
    beyond position 1 024.  nz: NonZeroRequested differs from Requested, for nodes and pods."""
    N = N_POOL
    rng = np.random.default_rng(11 * P + n_sigs)
    ncls = (np.arange(N) % N_CLS).astype(np.int32)
    shape_cpu, shape_mem = np.array([8000, 16000, 64000]), np.array([16, 32, 128]) * GiB
    sig = np.concatenate([np.arange(n_sigs), rng.integers(0, n_sigs, P - n_sigs)])
    sig = sig[rng.permutation(P)]
    req_cpu, req_mem = (200 + 10 * sig).astype(np.int64), ((128 + 8 * sig) * MiB).astype(np.int64)
    alloc_cpu, alloc_mem = shape_cpu[ncls].astype(np.int64), shape_mem[ncls].astype(np.int64)
    loaded = np.arange(N) < N_LOADED
    kw = dict(alloc_cpu=alloc_cpu, alloc_mem=alloc_mem, alloc_pods=np.full(N, 3, np.int32), node_class=ncls,
              init_req_cpu=np.where(loaded, alloc_cpu // 2, 0).astype(np.int64), init_req_mem=np.where(loaded, alloc_mem // 2, 0).astype(np.int64),
              req_cpu=req_cpu, req_mem=req_mem, pod_class=np.zeros(P, np.int32), n_pod_classes=1, n_node_classes=N_CLS,
              simon_raw=np.array([[10, 30, 60]], np.int64), const_score=np.full(1, 1000300, np.int64))
    kw["init_nz_cpu"], kw["init_nz_mem"] = kw["init_req_cpu"], kw["init_req_mem"]     # (the scores read NonZeroRequested)
    if nz:
        kw["init_nz_cpu"] = kw["init_req_cpu"] + (np.arange(N) // 3 % 3) * 100
        kw["init_nz_mem"] = kw["init_req_mem"] + (np.arange(N) // 3 % 3) * 200 * MiB
        kw["nz_cpu"], kw["nz_mem"] = req_cpu + (sig % 2) * 100, req_mem + (sig % 2) * 200 * MiB
    if special:
        preset, gate, pin = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.full(P, -1, np.int32)
        nodes = {0: N - 1, 1: 4, 2: 8, 3: 1009, 4: 1001, 5: 1049}            # (1 001 and 1 049: class 2, ranks 333 and 349)
        for i in range(6):
            kind = KINDS[i % 3]
            if kind == "gated":
                gate[i] = nodes[i]
            elif kind == "preset":
                preset[i] = gate[i] = nodes[i]                                 # (a preset pod is gated on its own node)
            else:
                pin[i] = nodes[i]
        kw.update(preset_node=preset, gate_node=gate, pin_node=pin)
    return capi.Problem(**kw).normalise()


def run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, expect, env=ENV):
    """the batch by its own sizes, with the dispatch off, and behind the per-scenario prologue: all equal to the oracle; `expect` = (entries
    per lane, scenarios on the one-entry body or None where the kernel holds one body) is what the route line must say"""
    for k in ("SIMON_NO_SIZE_DISPATCH", "SIMON_NO_SHARED_PROLOGUE"):
        monkeypatch.delenv(k, raising=False)
    entries, fits = expect
    for way, extra in WAYS.items():
        capfd.readouterr()
        res = run_on_table(prob, scen, orders, env=dict(env, **extra))
        route = re.findall(r"\[route\] unit (\S+) .*? prologue (\S+) entries/lane (\d) \(own size: ([^)]*)\)", capfd.readouterr().err)
        assert len(route) == 1, (way, route)
        unit, prologue, lane_entries, own = route[0]
        assert unit == "simon_table" and int(lane_entries) == entries, (way, route)
        assert prologue == ("per-scenario" if "SIMON_NO_SHARED_PROLOGUE" in extra else "shared-image"), (way, route)
        want = "none" if fits is None else "off" if "SIMON_NO_SIZE_DISPATCH" in extra else f"{fits} of {len(scen)} scenarios at 1"
        assert own == want, (way, own, want)
        assert_same(res, ref)


_POOL = {}


def pool_case(name, **feat):
    """(problem, scenarios, orders, sizes, oracle result) of a pool batch over the boundary sizes, computed once"""
    if name not in _POOL:
        P = 300
        prob = pool_problem(P, **feat)
        ncls = np.asarray(prob.node_class)
        sizes = [size_with(ncls, w) for w in (32, 1008, 1024, 1040)] + [N_POOL]
        if feat.get("special"):
            orders, steps = chunk_orders(P)
            for order in orders:
                assert all(int(order[s]) < 6 for s in steps) and {0, P - 1, 63, 64} <= set(steps)
        else:
            orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(P).permutation(P).astype(np.int32)])
        scen = np.array([[n, o] for n in sizes for o in range(len(orders))], np.int32)
        _POOL[name] = (prob, scen, orders, sizes, O.run(prob, scen, orders))
    return _POOL[name]


def check_sizes_and_upper_half(prob, scen, sizes, ref):
    """the padded sizes are the boundary's, and in the two-entry scenarios the oracle places pods at positions >= 1 024: a kernel that ran the
    one-entry body there could not find them"""
    ncls = np.asarray(prob.node_class)
    pad = [padded(ncls, n) for n in sizes]
    assert pad == [32, 1008, 1024, 1040, 1104], pad
    assert all((np.bincount(ncls[:n], minlength=N_CLS) % 16 != 0).any() for n in sizes)      # (class counts that are no multiples of 16)
    for s, (n, _) in enumerate(scen.tolist()):
        row = ref.placement[s]
        pos = positions(ncls, n)[row[row >= 0]]
        if padded(ncls, n) > ONE_ENTRY:
            assert (pos >= ONE_ENTRY).sum() >= 10, (n, int((pos >= ONE_ENTRY).sum()))
        else:
            assert pos.max() < ONE_ENTRY
    return sum(p <= ONE_ENTRY for p in pad)


def test_scenarios_on_both_sides_of_the_boundary(capfd, monkeypatch):
    """Padded sizes 32, 1 008, 1 024 (the last one-entry size), 1 040 (the first two-entry size) and the pool's 1 104, two orders each."""
    prob, scen, orders, sizes, ref = pool_case("plain")
    small = check_sizes_and_upper_half(prob, scen, sizes, ref)
    assert small == 3 and (ref.unscheduled[scen[:, 0] == sizes[0]] > 0).all() and (ref.unscheduled[scen[:, 0] == N_POOL] == 0).all()
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (2, small * len(orders)))


def test_preset_pinned_and_gated_pods_on_both_sides(capfd, monkeypatch):
    """The HAS_PIN instantiations: gated, preset and pinned pods on the first and the last step and on the 64-step chunk edges, four orders
    that rotate the kinds over those steps; one pod of each kind on a node beyond position 1 024 of the large scenarios."""
    prob, scen, orders, sizes, ref = pool_case("special", special=True)
    small = check_sizes_and_upper_half(prob, scen, sizes, ref)
    ncls = np.asarray(prob.node_class)
    n_of = scen[:, 0]
    large, row = n_of == N_POOL, ref.placement
    assert (row[n_of > 1001][:, [1, 4]] == [4, 1001]).all() and (row[n_of <= 1001][:, 4] == -2).all()                         # preset
    assert (row[~large][:, 0] == -2).all() and (row[large][:, 0] >= 0).all()                                                   # gated on the last node
    assert (row[n_of <= 1009][:, 3] == -2).all() and (row[n_of > 1009][:, 3] >= 0).all()                                       # ... on node 1 009
    assert (row[~large][:, 5] == -1).all() and (row[large][:, 5] == 1049).any()                                                # pinned beyond the small scenarios
    assert set(row[n_of > 8][:, 2].tolist()) == {8, -1}                                                                        # ... to a node that may be full by then
    assert positions(ncls, N_POOL)[[1001, 1049]].min() >= ONE_ENTRY
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (2, small * len(orders)))


def test_70_signatures(capfd, monkeypatch):
    """65 .. 128 signatures: two per lane (KQ = 2)."""
    prob, scen, orders, sizes, ref = pool_case("sigs70", n_sigs=70)
    small = check_sizes_and_upper_half(prob, scen, sizes, ref)
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (2, small * len(orders)))


def test_nonzero_requested_differs_from_requested(capfd, monkeypatch):
    """NonZeroRequested of nodes and pods above Requested (the NZEQ = false instantiations)."""
    prob, scen, orders, sizes, ref = pool_case("nz", nz=True)
    small = check_sizes_and_upper_half(prob, scen, sizes, ref)
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (2, small * len(orders)))


def test_cross_class_ties_in_both_bodies(capfd, monkeypatch):
    """Two caller classes of one shape, kept apart (SIMON_TABLE_NO_CLASS_CONTENT): every total ties across the classes, and the canonical order
    decides -- at 1 009 nodes (2 x 512 positions: one entry per lane) and at 1 025 and 1 100 nodes (two) in one batch."""
    P = 150
    prob = tie_problem(N_POOL, P, 2, 6)
    ncls = np.asarray(prob.node_class)
    counts = [1009, 1025, N_POOL]
    assert [padded(ncls, n, 2) for n in counts] == [1024, 1040, 1120]
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(N_POOL).permutation(P).astype(np.int32)])
    scen = np.array([[n, o] for n in counts for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.unscheduled == 0).all()
    for s, (n, o) in enumerate(scen.tolist()):
        by_position, cross_class = ties_in_oracle(prob, n, orders[o], ref.placement[s])
        assert by_position > 0 and cross_class > 0, (n, o)
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (2, 2), env=dict(ENV, SIMON_TABLE_NO_CLASS_CONTENT="1"))


def test_a_batch_that_fits_one_entry_keeps_the_one_entry_kernel(capfd, monkeypatch):
    """Every scenario at or below 1 024 padded positions: the host picks one entry per lane as before, and no second body is in play."""
    prob, _, orders, sizes, _ = pool_case("plain")
    scen = np.array([[n, o] for n in (sizes[0], 500, sizes[1], sizes[2]) for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    assert max(padded(np.asarray(prob.node_class), n) for n in scen[:, 0]) == ONE_ENTRY
    run_three_ways(prob, scen, orders, ref, capfd, monkeypatch, (1, None))

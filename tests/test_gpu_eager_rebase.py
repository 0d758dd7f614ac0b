"""GPU parity tests of the class terms' re-base at the event (round 12): where the score-table kernel's cycle is straight-line code, the
summary row of a signature is re-based in the cycle that takes the last feasible node of a node class from it -- inside the assume -- and
once behind the prologue; the plain pod no longer asks whether its row is current.  What can go wrong is the event, so the inputs are small
and built around it: every test first replays the oracle's own placements on the host and checks that the events it aims at occur, then
compares the whole placement matrix, the unscheduled counts and the used cpu / memory of every scenario with the oracle, exactly.  The
route of every launch (SIMON_DEBUG_ROUTE) must name the unit and the scheme (`re-base at-event` / `at-use`) the test is about."""
import re

import numpy as np
import pytest

import image_util as IU
import mix_util as MU
import oracle_lib as O
import randprob
from open_simulator_amd import capi
from test_gpu_cycle_paths import HBM_WS, run_on_table
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
BASE = dict(HBM_WS, SIMON_TABLE_COARSE="0", SIMON_DEBUG_ROUTE="1")      # the base unit's one-level kernels, workspace in HBM
SIZES = {2: (1, 17), 3: (1, 16, 17), 4: (1, 15, 16, 17)}                 # nodes per class: 1, and 15 / 16 / 17 around a block of 16 positions
ROUTE = re.compile(r"\[route\] unit (\S+) .*? prologue (\S+) entries/lane (\d) \(own size: ([^)]*)\) re-base (\S+) twins (\d)")


def emptying_problem(seed, sizes, n_sigs, P, slots, n_pod_classes=1, tables=False, images=False, node_order=None):
    """Node classes of `sizes` nodes in random pool order, class c with 4 000 (c + 1) milli-cores and slots[c] pod slots per node (small: a
    node's last slot takes the node from EVERY signature at once; the larger requests run out of cpu on the small shapes first).  Signature
    k = request k // n_pod_classes under pod class k % n_pod_classes; pod k < n_sigs carries signature k (the library numbers signatures by
    first appearance), the others a random one.  tables: preferred node affinity and PreferNoSchedule tables (with them every leave
    re-bases); images: ImageLocality per cluster size.  Returns (problem, signature of every pod)."""
    rng = np.random.default_rng(seed)
    Cn, N, Cp = len(sizes), int(sum(sizes)), n_pod_classes
    ncls = np.repeat(np.arange(Cn), sizes)
    ncls = (ncls[rng.permutation(N)] if node_order is None else ncls[node_order]).astype(np.int32)
    sig = np.concatenate([np.arange(n_sigs), rng.integers(0, n_sigs, P - n_sigs)])
    req = sig // Cp
    kw = dict(alloc_cpu=(4000 * (1 + ncls)).astype(np.int64), alloc_mem=(8 * GiB) * (1 + ncls.astype(np.int64)),
              alloc_pods=np.asarray(slots, np.int32)[ncls], node_class=ncls,
              req_cpu=(100 + 10 * req).astype(np.int64), req_mem=((64 + req) * MiB).astype(np.int64), pod_class=(sig % Cp).astype(np.int32),
              n_pod_classes=Cp, n_node_classes=Cn, simon_raw=rng.permutation(Cp * Cn).reshape(Cp, Cn).astype(np.int64) * 7,
              const_score=np.full(Cp, 1000300, np.int64))
    if tables:
        kw["node_affinity_raw"] = rng.integers(0, 50, (Cp, Cn)).astype(np.int64)
        kw["taint_prefer_raw"] = rng.integers(0, 4, (Cp, Cn)).astype(np.int64)
    if images:
        lists = [[i for i in (0, 1) if rng.random() < 0.5] for _ in range(N)]
        off = np.cumsum([0] + [len(x) for x in lists])
        img = np.array([i for x in lists for i in x], np.int32)
        holders = np.bincount(img, minlength=2)
        coff = np.arange(Cp + 1) * 2                                        # every pod class runs both images
        kw["image_locality"] = capi.ImageLocality(size=np.array([300 * MiB, 1900 * MiB], np.int64), node_off=off, node_image=img,
                                                  node_count=holders[img], class_off=coff, class_image=np.tile([0, 1], Cp))
    return capi.Problem(**kw).normalise(), sig.astype(np.int64)


def replay(prob, sig, nodes, order, row):
    """The oracle's placements of one scenario (`nodes`: its pool nodes), replayed: NodeResourcesFit of every signature on the touched node
    after every step, and the feasible-node counter of every (signature, caller node class).  Returns the events [(step, signature, class)]
    at which a counter reaches 0 and the steps of pods left unschedulable after their signature had lost every class.  The replay checks
    itself against the oracle: a placed pod fitted its node (unless bound by Spec.NodeName), an unschedulable one fitted none."""
    nodes = np.asarray(nodes)
    K = int(sig.max()) + 1
    first = np.array([np.flatnonzero(sig == k)[0] for k in range(K)])
    rc, rm = np.asarray(prob.req_cpu)[first], np.asarray(prob.req_mem)[first]
    ac, am, ap = (np.asarray(a)[nodes].astype(np.int64) for a in (prob.alloc_cpu, prob.alloc_mem, prob.alloc_pods))
    cls = np.asarray(prob.node_class)[nodes]
    where = {int(j): i for i, j in enumerate(nodes)}
    uc, um, up = np.zeros(len(nodes), np.int64), np.zeros(len(nodes), np.int64), np.zeros(len(nodes), np.int64)
    fits = lambda i: (up[i] < ap[i]) & (uc[i] + rc <= ac[i]) & (um[i] + rm <= am[i])          # noqa: E731  [K]
    feas = np.stack([fits(i) for i in range(len(nodes))], 1)                                   # [K][n]
    count = np.stack([feas[:, cls == c].sum(1) for c in range(prob.n_node_classes)], 1)        # [K][Cn]
    preset = np.asarray(prob.preset_node) if prob.preset_node is not None else np.full(prob.n_pods, -1)
    events, lost = [], []
    for step, pod in enumerate(np.asarray(order).tolist()):
        j, k = int(row[pod]), int(sig[pod])
        if j == -1:
            assert count[k].sum() == 0, (step, pod)
            lost.append(step)
        if j < 0:
            continue
        i = where[j]
        assert feas[k, i] or preset[pod] >= 0, (step, pod, j)
        uc[i] += rc[k]; um[i] += rm[k]; up[i] += 1
        now = feas[:, i] & fits(i)
        gone = feas[:, i] & ~now
        feas[:, i] = now
        count[gone, cls[i]] -= 1
        events += [(step, int(q), int(cls[i])) for q in np.flatnonzero(gone & (count[:, cls[i]] == 0))]
    return events, lost


def check_events(prob, sig, scen, orders, ref, all_three=True, at_once=True):
    """The events of every scenario of a prefix batch; with all_three the three conditions of the classes-emptying cases on each of them:
    some signature loses at least Cn - 1 classes, some cycle empties a class for two or more signatures at once, and some signature loses
    every class and has a later pod (which the replay has seen to be unschedulable)."""
    out = []
    for s, (n, o) in enumerate(np.asarray(scen).tolist()):
        events, lost = replay(prob, sig, np.arange(n), orders[o], ref.placement[s])
        assert events, s
        if all_three:
            per_sig = np.bincount([k for _, k, _ in events], minlength=int(sig.max()) + 1)
            present = len(set(np.asarray(prob.node_class)[:n].tolist()))
            assert per_sig.max() >= present - 1, (s, per_sig)
            steps = [st for st, _, _ in events]
            assert not at_once or max(np.bincount(steps)) >= 2, s
            assert lost and ref.unscheduled[s] >= len(lost) > 0, s
        out.append(events)
    return out


def batch(prob, n_orders=2, smaller=(2,)):
    """the pool and some smaller prefixes, under the identity order and random ones"""
    P, N = prob.n_pods, prob.n_nodes
    orders = np.stack([np.arange(P, dtype=np.int32)] + [np.random.default_rng(P + i).permutation(P).astype(np.int32) for i in range(1, n_orders)])
    sizes = [N] + [N - d for d in smaller if N - d >= 1]
    return np.array([[n, o] for n in sizes for o in range(n_orders)], np.int32), orders


def run_routed(prob, scen, orders, capfd, env, unit="simon_table", prologue=None, scheme="at-event"):
    """run_on_table, and the launch's route line: unit, prologue and re-base scheme as expected"""
    capfd.readouterr()
    res = run_on_table(prob, scen, orders, env=env)
    err = capfd.readouterr().err
    route = ROUTE.findall(err)
    assert len(route) == 1, err
    assert route[0][0] == unit and route[0][4] == scheme, route
    if prologue is not None:
        assert route[0][1] == prologue, route
    return res, route[0], err


# ---- classes emptying -----------------------------------------------------------------------------------------------------------------
# (seeds: the first of 0, 1, 2, ... for which the oracle's result meets check_events' three conditions in every scenario of the batch)
EMPTYING = {(2, 3): 0, (3, 5): 0, (4, 8): 0}


@pytest.mark.parametrize("n_classes,n_sigs", list(EMPTYING))
def test_classes_emptying(n_classes, n_sigs, capfd):
    sizes = SIZES[n_classes]
    slots = (1, 2, 1, 3)[:n_classes]
    cap = int(np.dot(sizes, slots))
    prob, sig = emptying_problem(EMPTYING[n_classes, n_sigs], sizes, n_sigs, cap + 12, slots)
    scen, orders = batch(prob)
    ref = O.run(prob, scen, orders)
    check_events(prob, sig, scen, orders, ref)
    res, _, _ = run_routed(prob, scen, orders, capfd, BASE)
    assert_same(res, ref)


# ---- lane edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sigs,n_pod_classes,no_twins", [(1, 1, False), (64, 1, False), (65, 1, False), (128, 1, False), (128, 2, False), (128, 2, True)],
                         ids=["K1", "K64", "K65", "K128", "K128-twins", "K128-twins-off"])
def test_lane_edges(n_sigs, n_pod_classes, no_twins, capfd):
    """One signature, a full register (64), one signature in the upper register (65) and two full registers (128; with two pod classes over
    64 requests every upper signature has a twin 64 slots below it, kStTwins, unless SIMON_TABLE_NO_TWINS keeps them apart).  A node's last
    pod slot takes the node from every signature: the event must reach all of them -- signature 0, signature 63 and the upper register."""
    sizes, slots = SIZES[4], (1, 3, 4, 5)
    cap = int(np.dot(sizes, slots))
    prob, sig = emptying_problem(100 + n_sigs, sizes, n_sigs, max(n_sigs, cap) + 12, slots, n_pod_classes=n_pod_classes)
    scen, orders = batch(prob)
    ref = O.run(prob, scen, orders)
    for events in check_events(prob, sig, scen, orders, ref, at_once=n_sigs > 1):     # (one signature: nothing to empty at once)
        assert {k for _, k, _ in events} == set(range(n_sigs))
    res, route, _ = run_routed(prob, scen, orders, capfd, dict(BASE, **({"SIMON_TABLE_NO_TWINS": "1"} if no_twins else {})))
    assert route[5] == ("1" if n_pod_classes == 2 and not no_twins else "0"), route        # the launch paired the signatures (kStTwins), or did not
    assert_same(res, ref)


# ---- every class-term source ----------------------------------------------------------------------------------------------------------
def test_static_score_tables(capfd):
    """Preferred node affinity and PreferNoSchedule: tables with maxima of their own over the classes that hold a feasible node."""
    sizes, slots = SIZES[4], (1, 2, 1, 3)
    prob, sig = emptying_problem(7, sizes, 6, int(np.dot(sizes, slots)) + 12, slots, n_pod_classes=2, tables=True)
    scen, orders = batch(prob)
    ref = O.run(prob, scen, orders)
    check_events(prob, sig, scen, orders, ref)
    res, _, _ = run_routed(prob, scen, orders, capfd, BASE)
    assert_same(res, ref)


def test_image_locality_sizes(capfd):
    """ImageLocality per cluster size: the class term reads the scenario's size slot.  The oracle runs every scenario's one-size problem."""
    sizes, slots = SIZES[3], (1, 2, 2)
    prob, sig = emptying_problem(9, sizes, 4, int(np.dot(sizes, slots)) + 12, slots, n_pod_classes=2, images=True)
    scen, orders = batch(prob, smaller=(2, 9))
    ref = IU.oracle_per_size(prob, scen, orders)
    check_events(prob, sig, scen, orders, ref)
    res, _, _ = run_routed(prob, scen, orders, capfd, BASE)
    assert_same(res, ref)


# ---- the cold assume ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["preset", "preset+pinned"])
def test_a_preset_and_a_pinned_pod_take_a_class_s_last_node(pinned, capfd):
    """Classes 0 and 1 are one node with one pod slot each, and no plain pod wants them while the others have room (lowest Simon scores): a
    pod bound by Spec.NodeName fills class 0 at step 3, and a pinned pod class 1 at step 6 -- the counters reach 0 in the cold expansion of
    the assume, and the plain pods behind them are scored over the classes that are left."""
    N, P = 30, 90
    ncls = np.array([0, 1] + [2] * 10 + [3] * (N - 12), np.int32)
    req = np.arange(P) % 5
    prob = capi.Problem(alloc_cpu=(4000 * (1 + ncls)).astype(np.int64), alloc_mem=(8 * GiB) * (1 + ncls.astype(np.int64)),
                        alloc_pods=np.array([1, 1, 2, 3], np.int32)[ncls], node_class=ncls,
                        req_cpu=(100 + 10 * req).astype(np.int64), req_mem=((64 + req) * MiB).astype(np.int64), pod_class=np.zeros(P, np.int32),
                        n_pod_classes=1, n_node_classes=4, simon_raw=np.array([[0, 20, 60, 100]], np.int64), const_score=np.full(1, 1000300, np.int64))
    preset, pin = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    preset[3] = 0
    if pinned:
        pin[6] = 1
    else:
        preset[6] = 1
    prob.preset_node = preset
    prob.gate_node = np.where(preset >= 0, preset, -1).astype(np.int32)
    if pinned:
        prob.pin_node = pin
    prob.normalise()
    orders = np.arange(P, dtype=np.int32)[None]
    scen = np.array([[N, 0], [N - 3, 0]], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.placement[:, 3] == 0).all() and (ref.placement[:, 6] == 1).all()
    for s, (n, o) in enumerate(scen.tolist()):
        events, _ = replay(prob, req.astype(np.int64), np.arange(n), orders[o], ref.placement[s])
        assert {(st, c) for st, _, c in events} >= {(3, 0), (6, 1)}, events               # the bound pods' own steps empty classes 0 and 1
        assert {c for _, _, c in events} >= {0, 1, 2}                                     # ... and plain pods a third one later
    res, _, _ = run_routed(prob, scen, orders, capfd, BASE)
    assert_same(res, ref)


# ---- routes ---------------------------------------------------------------------------------------------------------------------------
def route_case():
    sizes, slots = SIZES[4], (1, 2, 1, 3)
    prob, sig = emptying_problem(21, sizes, 7, int(np.dot(sizes, slots)) + 12, slots)
    scen, orders = batch(prob)
    ref = O.run(prob, scen, orders)
    check_events(prob, sig, scen, orders, ref)
    return prob, scen, orders, ref


@pytest.mark.parametrize("prologue", ["shared-image", "per-scenario"])
def test_both_prologues(prologue, capfd):
    prob, scen, orders, ref = route_case()
    env = dict(BASE, **({"SIMON_NO_SHARED_PROLOGUE": "1"} if prologue == "per-scenario" else {}))
    res, _, _ = run_routed(prob, scen, orders, capfd, env, prologue=prologue)
    assert_same(res, ref)


def test_workspace_in_lds_and_in_hbm(capfd, monkeypatch):
    """A single small scenario: its workspace lives in LDS by default (simon_table_lds.hip), and in HBM with SIMON_LDS_WS=0."""
    prob, scen, orders, ref = route_case()
    one = scen[:1]
    ref1 = O.run(prob, one, orders)
    monkeypatch.delenv("SIMON_LDS_WS", raising=False)
    res, _, _ = run_routed(prob, one, orders, capfd, {"SIMON_DEBUG_ROUTE": "1", "SIMON_TABLE_COARSE": "0"}, unit="simon_table_lds")
    assert_same(res, ref1)
    res, _, _ = run_routed(prob, one, orders, capfd, BASE, unit="simon_table")
    assert_same(res, ref1)


def test_two_level_layout(capfd):
    """COARSE without REST rows: summary entries of 64 positions, per-16 entries and counters in the workspace.  It keeps the lazy scheme
    (simon_table.hip, kEager: the layout of the problems with many node classes, where re-basing once per use is the cheaper way)."""
    prob, scen, orders, ref = route_case()
    res, _, err = run_routed(prob, scen, orders, capfd, dict(BASE, SIMON_TABLE_COARSE="1"), scheme="at-use")
    assert re.search(r"\[route\] variant \d+ rest 0 spread 0 .* coarse 1 ", err), err
    assert_same(res, ref)


def test_segmented_batch_on_the_ranked_kernels(capfd, monkeypatch):
    """Fixed nodes and prefixes of two pool segments (simon_set_scenario_segments): the ranked instantiations, per-scenario class lists."""
    sizes, slots = SIZES[4], (1, 2, 1, 3)
    N = int(sum(sizes))
    F = N - 16
    prob, sig = emptying_problem(33, sizes, 6, int(np.dot(sizes, slots)) + 12, slots)
    starts = [F, F + 8]
    cnt = np.array([[8, 8], [3, 8], [8, 0], [1, 5]], np.int32)
    P = prob.n_pods
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(5).permutation(P).astype(np.int32)])
    scen = np.stack([F + cnt.sum(1), np.arange(len(cnt)) % 2], 1).astype(np.int32)
    rows, refs = [], []
    for s in range(len(cnt)):
        present = MU.present_mask(N, starts, cnt[s])
        row, r = MU.oracle_of_scenario(prob, present, orders[scen[s, 1]])
        events, lost = replay(prob, sig, np.flatnonzero(present), orders[scen[s, 1]], row)
        assert events and lost, s
        rows.append(row); refs.append(r)
    for k, v in BASE.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(starts, cnt)
        ctx.run_loaded(True)
        st = ctx.stats()
        res = ctx.fetch(True)
    err = capfd.readouterr().err
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation in (4, 5)
    assert "score-table kernel, ranked instantiation" in err, err
    route = ROUTE.findall(err)
    assert len(route) == 1 and route[0][0] == "simon_table" and route[0][4] == "at-event", err
    assert (res.placement == np.stack(rows)).all()
    for s, r in enumerate(refs):
        assert (res.unscheduled[s], res.used_cpu[s], res.used_mem[s]) == (r.unscheduled[0], r.used_cpu[0], r.used_mem[0]), s


def test_both_bodies_of_the_fused_kernel(capfd):
    """1 100 nodes in three classes; the 18 nodes of the class the pods like best hold one pod each.  Scenarios on both sides of 1 024
    padded positions in one launch: the one-entry body and the two-entry body both meet the event."""
    N, P = 1100, 260
    ncls = np.where(np.arange(N) % 61 == 7, 2, np.arange(N) % 2).astype(np.int32)
    sig = np.arange(P) % 6
    prob = capi.Problem(alloc_cpu=(8000 * (1 + ncls)).astype(np.int64), alloc_mem=(16 * GiB) * (1 + ncls.astype(np.int64)),
                        alloc_pods=np.where(ncls == 2, 1, 3).astype(np.int32), node_class=ncls,
                        req_cpu=(200 + 10 * sig).astype(np.int64), req_mem=((128 + 8 * sig) * MiB).astype(np.int64), pod_class=np.zeros(P, np.int32),
                        n_pod_classes=1, n_node_classes=3, simon_raw=np.array([[10, 30, 90]], np.int64), const_score=np.full(1, 1000300, np.int64)).normalise()
    pad = lambda n: int((((np.bincount(ncls[:n], minlength=3) + 15) // 16) * 16).sum())         # noqa: E731
    sizes = [600, 990, N]
    assert [pad(n) <= 1024 for n in sizes] == [True, True, False]
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(8).permutation(P).astype(np.int32)])
    scen = np.array([[n, o] for n in sizes for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    for events in check_events(prob, sig.astype(np.int64), scen, orders, ref, all_three=False):
        assert {(k, c) for _, k, c in events} >= {(k, 2) for k in range(6)}                       # class 2 empties for every signature
    res, route, _ = run_routed(prob, scen, orders, capfd, BASE, prologue="shared-image")
    assert route[2] == "2" and route[3] == "4 of 6 scenarios at 1", route
    assert_same(res, ref)


# ---- one lazy family ------------------------------------------------------------------------------------------------------------------
def test_a_spread_problem_still_re_bases_at_use(capfd, monkeypatch):
    """Soft spread constraints: generation 7 keeps the dirty rows and re-bases at the row's next use.  Two pod slots per node: whole
    node classes fill up while pods keep arriving."""
    prob = randprob.rand_problem(7300, N=40, P=300, spread_soft=True, n_node_classes=4, n_pod_classes=9)
    prob.alloc_pods = np.full(prob.n_nodes, 2, np.int32)
    prob.normalise()
    scen, orders = randprob.rand_scenarios(170, prob, S=4)
    ref = O.run(prob, scen, orders)
    ncls = np.asarray(prob.node_class)
    for s, (n, _) in enumerate(np.asarray(scen).tolist()):
        row = ref.placement[s]
        held = np.bincount(row[row >= 0], minlength=n)[:n]
        assert any((held[ncls[:n] == c] == 2).all() for c in set(ncls[:n].tolist())), s          # some class is full: it left every signature
        assert ref.unscheduled[s] > 0
    monkeypatch.setenv("SIMON_DEBUG_ROUTE", "1")
    capfd.readouterr()
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch(scen, orders)
        st = ctx.stats()
    err = capfd.readouterr().err
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation == 7, (st.kernel_variant, st.kernel_generation)
    route = ROUTE.findall(err)
    assert len(route) == 1 and route[0][4] == "at-use", err
    assert_same(res, ref)

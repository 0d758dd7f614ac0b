"""GPU parity tests of the score-table kernel's scheduling cycle, path by path: the rare pods (preset, pinned, gated out, unschedulable)
and the class-term re-base leave the plain pod's straight-line path and rejoin it, and the summary scan decides ties by position inside
a lane's entries and across lanes.  Generations 4 / 5 only, the oracle is the expected result, and every test first checks that the
path it aims at occurs in the oracle's result."""
import numpy as np
import pytest

import oracle_lib as O
import randprob
from open_simulator_amd import capi
from test_gpu_parity import assert_same, run_gpu

pytestmark = pytest.mark.gpu

HBM_WS = {"SIMON_LDS_WS": "0"}          # small batches default to the LDS-resident workspace (simon_table_lds.hip): the base unit needs this


def run_on_table(prob, scen, orders, env=None):
    """run_gpu, and the generation of the kernel that ran: a fall-through to another kernel must not pass silently."""
    seen = []
    stats = capi.Context.stats

    def spy(self):
        st = stats(self)
        seen.append(st.kernel_generation)
        run_on_table.lds_bytes = st.lds_bytes
        return st
    capi.Context.stats = spy
    try:
        res, variant = run_gpu(prob, scen, orders, env=env)
    finally:
        capi.Context.stats = stats
    assert variant == capi.KERNEL_NARROW_CACHE and seen and seen[-1] in (4, 5), (variant, seen)
    return res


# ---- rejoin paths -----------------------------------------------------------------------------------------------------------------
HUGE_CPU = 10_000_000                    # milli-cores: fits no node


def rejoin_problem(seed, pins):
    """200 pods x 70 nodes with presets, gates, a static mask, initial state (and pins), plus pods no node can hold."""
    N, P = 70, 200
    prob = randprob.rand_problem(seed, N=N, P=P, presets=True, gates=True, static_mask=True, init_state=True, pins=pins)
    preset = np.asarray(prob.preset_node)
    gate = np.asarray(prob.gate_node)
    pin = np.asarray(prob.pin_node) if pins else np.full(P, -1)
    plain = np.flatnonzero((preset < 0) & (gate < 0) & (pin < 0))
    huge, gated = plain[:12], plain[12:24]
    prob.req_cpu = np.asarray(prob.req_cpu).copy()
    prob.req_cpu[huge] = HUGE_CPU
    prob.gate_node = gate.copy()
    prob.gate_node[gated] = 62                               # out of every scenario of at most 62 nodes
    kinds = {"preset": np.flatnonzero(preset >= 0), "pinned": np.flatnonzero(pin >= 0), "gated": gated, "huge": huge, "plain": plain[24:]}
    kinds["other"] = np.setdiff1d(np.arange(P), np.concatenate(list(kinds.values())))      # (pods the generator gated itself)
    return prob.normalise(), kinds


def rejoin_orders(kinds, P, pins):
    """Pod orders whose steps 62 .. 66 (the 64-step chunk edge) and whose first steps alternate rare pods with plain ones."""
    rare = ["preset", "huge", "gated"] + (["pinned"] if pins else [])
    edge_patterns = [                                       # steps 62, 63, 64, 65, 66
        ["plain", rare[0], rare[1], rare[2], "plain"],
        ["plain", rare[-1], "plain", rare[0], "plain"],
        [rare[1], "plain", rare[2], "plain", rare[-1]],
        [rare[2], rare[1], rare[0], rare[-1], rare[1]],
    ]
    orders = []
    for pat in edge_patterns:
        pool = {k: list(v) for k, v in kinds.items()}
        order = [None] * P
        for step, kind in zip(range(62, 67), pat):
            order[step] = pool[kind].pop()
        # the head of the stream: plain, rare, plain, rare, ... through every rare kind twice, then two rare pods in a row
        head = []
        for kind in rare * 2:
            head += [pool["plain"].pop(), pool[kind].pop()]
        head += [pool[rare[0]].pop(), pool[rare[1]].pop(), pool["plain"].pop()]
        rest = [p for v in pool.values() for p in v]
        rest = list(np.random.default_rng(len(orders)).permutation(rest))
        for step in range(P):
            if order[step] is None:
                order[step] = head.pop(0) if head else rest.pop()
        assert sorted(order) == list(range(P))
        orders.append(order)
    return np.array(orders, np.int32), edge_patterns


@pytest.mark.parametrize("pins", [False, True])
@pytest.mark.parametrize("coarse", ["0", "1"])
def test_rare_pods_leave_and_rejoin_the_plain_path(pins, coarse):
    prob, kinds = rejoin_problem(9100 + pins, pins)
    P = prob.n_pods
    orders, patterns = rejoin_orders(kinds, P, pins)
    scen = np.array([[n, o] for o in range(len(orders)) for n in (40, 55, 60, 70)], np.int32)
    ref = O.run(prob, scen, orders)
    # the paths occur in the oracle's result
    preset = np.asarray(prob.preset_node)
    assert len(kinds["preset"]) > 0 and (ref.placement[:, kinds["preset"]] == preset[kinds["preset"]]).sum() > 0
    assert all(0 < u < P for u in ref.unscheduled.tolist())
    assert (ref.placement[:, kinds["huge"]] == -1).all()
    small = scen[:, 0] <= 62
    assert (ref.placement[small][:, kinds["gated"]] == -2).all() and (ref.placement[~small][:, kinds["gated"]] > -2).all()
    if pins:
        pl = ref.placement[:, kinds["pinned"]]
        assert (pl >= 0).any() and (pl == -1).any()                                             # pinned pods that land and that do not
    for s, (n, o) in enumerate(scen.tolist()):
        for step, kind in zip(range(62, 67), patterns[o]):
            got = ref.placement[s, orders[o][step]]
            if kind == "plain":
                assert got >= -1
            elif kind == "huge":
                assert got == -1
            elif kind == "preset":
                assert got in (preset[orders[o][step]], -2)
            elif kind == "gated":
                assert (got == -2) == (n <= 62)
        assert (ref.placement[s, orders[o][:20]] >= 0).sum() >= 5                              # plain pods between the rare ones do land
    env = dict(HBM_WS, SIMON_TABLE_COARSE=coarse)
    assert_same(run_on_table(prob, scen, orders, env=env), ref)


# ---- pair boundaries ----------------------------------------------------------------------------------------------------------------
def tie_problem(N, P, n_classes, n_sigs):
    """N nodes of ONE allocatable shape in `n_classes` caller classes with identical score columns (node j: class j % n_classes): every
    total ties, inside a node class and across classes; P pods of `n_sigs` distinct small requests."""
    rng = np.random.default_rng(N * 7 + n_classes)
    cpu = 100 + 10 * (np.arange(P) % n_sigs)
    mem = (64 + (np.arange(P) % n_sigs)) << 20
    perm = rng.permutation(P)
    prob = capi.Problem(alloc_cpu=np.full(N, 32000, np.int64), alloc_mem=np.full(N, 64 << 30, np.int64), alloc_pods=np.full(N, 250, np.int32),
                        node_class=(np.arange(N) % n_classes).astype(np.int32), req_cpu=cpu[perm].astype(np.int64), req_mem=mem[perm].astype(np.int64),
                        pod_class=np.zeros(P, np.int32), n_pod_classes=1, n_node_classes=n_classes,
                        simon_raw=np.full((1, n_classes), 50, np.int64), const_score=np.full(1, 1000300, np.int64))
    return prob.normalise()


def ties_in_oracle(prob, n, order, row):
    """(steps at which the chosen node was untouched while a later node was untouched as well -- a tie decided by position --, and among them
    those where such a later node belongs to a LOWER caller class: position order would have taken it, the canonical order decides)."""
    used = np.zeros(n, bool)
    ncls = np.asarray(prob.node_class)[:n]
    by_position = cross_class = 0
    for pod in order:
        j = row[pod]
        if j < 0:
            continue
        if not used[j]:
            later = np.flatnonzero(~used[j + 1:]) + j + 1
            by_position += len(later) > 0
            cross_class += bool((ncls[later] < ncls[j]).any())
        used[j] = True
    return by_position, cross_class


# node counts -> summary entries of 16 positions: one class  16 -> 1, 17 -> 2, 33 -> 3, 1008 -> 63, 1024 -> 64, 1025 -> 65, 2032 -> 127, 2048 -> 128,
# 2049 -> 129; two classes (each padded to 16)  1 -> 1, 2 -> 2, 33 -> 3, 993 -> 63, 1009 -> 64, 1025 -> 65, 2017 -> 127, 2048 -> 128, 2049 -> 129.
# One batch per pool size: the largest scenario of a batch picks the entries per lane (1, 2 or 4).
POOLS = {1: [(33, [16, 17, 33]), (1024, [1008, 1024]), (2048, [1025, 2032, 2048]), (2049, [17, 1025, 2049])],
         2: [(33, [1, 2, 33]), (1009, [993, 1009]), (2048, [1025, 2017, 2048]), (2049, [2, 1025, 2049])]}


def entries(n, n_classes):
    return sum((len(range(c, n, n_classes)) + 15) // 16 for c in range(n_classes))


def run_tie_batch(n_classes, N, counts, env, n_sigs=6, P=150):
    prob = tie_problem(N, P, n_classes, n_sigs)
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(N).permutation(P).astype(np.int32)])
    scen = np.array([[n, o] for n in counts for o in (0, 1)], np.int32)
    ref = O.run(prob, scen, orders)
    assert (ref.unscheduled == 0).all()
    for s, (n, o) in enumerate(scen.tolist()):
        by_position, cross_class = ties_in_oracle(prob, n, orders[o], ref.placement[s])
        if n > 1:
            assert by_position > 0, (n, o)
        if n_classes == 2 and n > 2:
            assert cross_class > 0, (n, o)               # the canonical cross-class tie-break fires
    assert_same(run_on_table(prob, scen, orders, env=env), ref)


def test_entry_counts_name_the_boundaries():
    assert [entries(n, 1) for n in (16, 17, 33, 1008, 1024, 1025, 2032, 2048, 2049)] == [1, 2, 3, 63, 64, 65, 127, 128, 129]
    assert [entries(n, 2) for n in (1, 2, 33, 993, 1009, 1025, 2017, 2048, 2049)] == [1, 2, 3, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("n_classes", [1, 2])
@pytest.mark.parametrize("pool", range(4))
def test_ties_at_the_summary_entry_boundaries(n_classes, pool):
    N, counts = POOLS[n_classes][pool]
    run_tie_batch(n_classes, N, counts, HBM_WS)


@pytest.mark.parametrize("n_classes", [1, 2])
def test_ties_on_the_two_level_summary(n_classes):
    run_tie_batch(n_classes, 2049, [130, 1025, 2049], dict(HBM_WS, SIMON_TABLE_COARSE="1"))


@pytest.mark.parametrize("n_classes", [1, 2])
def test_ties_with_70_signatures(n_classes):
    N, counts = POOLS[n_classes][2]
    run_tie_batch(n_classes, N, counts, HBM_WS, n_sigs=70)


def test_ties_with_the_workspace_in_lds(monkeypatch):
    """SIMON_LDS_WS at its default: a single small scenario keeps table and state in LDS (simon_table_lds.hip)."""
    monkeypatch.delenv("SIMON_LDS_WS", raising=False)      # (conftest alternates the home by test id: this test is about the default)
    prob = tie_problem(33, 150, 2, 6)
    orders = np.arange(150, dtype=np.int32)[None]
    scen = np.array([[33, 0]], np.int32)
    ref = O.run(prob, scen, orders)
    by_position, cross_class = ties_in_oracle(prob, 33, orders[0], ref.placement[0])
    assert by_position > 0 and cross_class > 0
    assert_same(run_on_table(prob, scen, orders, env=HBM_WS), ref)
    lds_hbm = run_on_table.lds_bytes
    assert_same(run_on_table(prob, scen, orders), ref)
    assert run_on_table.lds_bytes > lds_hbm                # table and state did move into LDS


# ---- re-base next to a rare pod -----------------------------------------------------------------------------------------------------
def test_rebase_right_before_and_after_a_preset_pod(monkeypatch):
    """Two two-node classes the pods prefer (Simon score) hold two pods per node: the class's last feasible node disappears -- the row of the
    signature goes dirty and is re-based at its next use -- in the step right before a preset pod (class 0) and right after one (class 1)."""
    N, P = 24, 16
    ncls = np.array([0, 0, 1, 1] + [2] * (N - 4), np.int32)
    prob = capi.Problem(alloc_cpu=np.full(N, 32000, np.int64), alloc_mem=np.full(N, 64 << 30, np.int64),
                        alloc_pods=np.where(ncls < 2, 2, 110).astype(np.int32), node_class=ncls,
                        req_cpu=np.full(P, 100, np.int64), req_mem=np.full(P, 64 << 20, np.int64), pod_class=np.zeros(P, np.int32),
                        n_pod_classes=1, n_node_classes=3, simon_raw=np.array([[100, 60, 0]], np.int64), const_score=np.full(1, 1000300, np.int64))
    preset = np.full(P, -1, np.int32)
    preset[[4, 8]] = [10, 11]                             # steps 4 and 8 of the identity order, onto nodes of the large class
    prob.preset_node = preset
    prob.gate_node = np.where(preset >= 0, preset, -1).astype(np.int32)
    prob.normalise()
    orders = np.arange(P, dtype=np.int32)[None]
    scen = np.array([[N, 0], [20, 0]], np.int32)
    ref = O.run(prob, scen, orders)
    for row in ref.placement:
        cls_of = ncls[row]
        assert cls_of[:4].tolist() == [0, 0, 0, 0]         # class 0 is full after step 3: its last feasible node leaves right BEFORE the preset pod of step 4
        assert row[4] == 10 and row[8] == 11
        assert cls_of[5:8].tolist() == [1, 1, 1] and cls_of[9] == 1   # step 5 re-bases; class 1's last slot goes at step 9, right AFTER the preset pod of step 8
        assert (cls_of[10:] == 2).all()                     # step 10 re-bases again
    assert (ref.unscheduled == 0).all()
    for coarse in ("0", "1"):
        assert_same(run_on_table(prob, scen, orders, env=dict(HBM_WS, SIMON_TABLE_COARSE=coarse)), ref)
    monkeypatch.delenv("SIMON_LDS_WS", raising=False)
    assert_same(run_on_table(prob, scen, orders), ref)     # and with the workspace in LDS (the default for a batch this small)

"""GPU tests of the score-table kernel's shared initial image ("prologue by copy", simon_table.hip: table_image_kernel, kSharedPro): a prefix
scenario in canonical order copies its initial table, node state and block summaries from an image of the batch's largest scenario instead of
evaluating them.  Every case runs three ways -- the default, SIMON_NO_SHARED_PROLOGUE=1 (every scenario evaluates its own table, the code every
other route keeps) and the C oracle -- and all three must agree on every placement row, unscheduled count and used cpu / memory; the route line
(SIMON_DEBUG_ROUTE) must name the prologue that ran.

The cases sit where the copy can go wrong: a node class that grows with the scenario through 0, 1, 15, 16, 17, 32 and 33 nodes (absent class,
cut last block, exact block ends), first / in the middle / last in class order (later class segments shift by whole blocks), 64 and 65 summary
entries (one and two per lane), 1 / 64 / 65 / 128 request signatures (one and two per lane), a static mask inside the last block, initial
Requested with NonZeroRequested != Requested, nodes without a free pod slot, preset / pinned / gated pods, more than 64 node classes; a ranked and
a segmented batch must keep the per-scenario prologue.  All runs keep the workspace in HBM on the one-level layout (SIMON_LDS_WS=0,
SIMON_TABLE_COARSE=0): batches this small would otherwise take the LDS-resident unit, which has no copy path."""
import re

import numpy as np
import pytest

import mix_util as MU
import oracle_lib as O
from open_simulator_amd import capi

pytestmark = pytest.mark.gpu
MiB, GiB = 1 << 20, 1 << 30
P = 300
SHAPE = {"A": (8000, 16 * GiB), "B": (16000, 32 * GiB), "T": (4000, 8 * GiB), "U": (6000, 8 * GiB)}
BASE = {"last": list("ABABABABABABABABA"),                 # no template-shaped node in the cluster: the growing class is the last one, from 0 nodes
        "first": list("TABABABABABABABABA"),               # one template-shaped node first / second: the growing class is class 0 / class 1
        "middle": list("ATBABABABABABABABA")}
ENV = {"SIMON_DEBUG_ROUTE": "1", "SIMON_LDS_WS": "0", "SIMON_TABLE_COARSE": "0"}


def _problem(seed, kinds, shapes, K, *, mask=False, init=False, full=False, presets=False, pins=False, gates=False):
    """Nodes of the given kinds (a kind = a shape = a node class, numbered by first appearance as the library numbers them), P pods of K + 1 request
    signatures (every one used; K = 1: that one alone, the pod slots run out instead), three pod classes with their own Simon row."""
    rng = np.random.default_rng(seed)
    N = len(kinds)
    names = list(dict.fromkeys(kinds))
    ncls = np.array([names.index(k) for k in kinds], np.int32)
    sig = np.concatenate([np.arange(K), rng.integers(0, K, P - K)])
    if K > 1:
        sig[K:][np.arange(K, P) % 12 == 11] = K                  # signature K asks for more cpu than any node has: every scenario leaves pods unscheduled
    sig_cpu = np.append(np.full(1, 1000) if K == 1 else 200 + 20 * np.arange(K), 70000)
    sig_mem = np.append(np.full(1, 1024) if K == 1 else 128 + 16 * np.arange(K), 1024) * MiB
    req_cpu, req_mem = sig_cpu[sig].astype(np.int64), sig_mem[sig].astype(np.int64)
    pcls = (sig % 3).astype(np.int32)
    kw = dict(alloc_cpu=np.array([shapes[k][0] for k in kinds], np.int64), alloc_mem=np.array([shapes[k][1] for k in kinds], np.int64),
              alloc_pods=np.full(N, 12, np.int32), node_class=ncls, req_cpu=req_cpu, req_mem=req_mem, pod_class=pcls, n_pod_classes=3,
              n_node_classes=len(names), simon_raw=rng.integers(0, 120, (3, len(names))).astype(np.int64), const_score=np.full(3, 1000300, np.int64))
    if init:                                                       # Requested at the start, NonZeroRequested above it on some nodes
        f = rng.random(N) * 0.5
        kw["init_req_cpu"] = (kw["alloc_cpu"] * f // 100 * 100).astype(np.int64)
        kw["init_req_mem"] = (kw["alloc_mem"] * f // MiB * MiB).astype(np.int64)
        kw["init_nz_cpu"] = kw["init_req_cpu"] + rng.integers(0, 3, N) * 100
        kw["init_nz_mem"] = kw["init_req_mem"] + rng.integers(0, 3, N) * 200 * MiB
        kw["init_npods"] = rng.integers(0, 5, N).astype(np.int32)
        kw["nz_cpu"], kw["nz_mem"] = req_cpu + (sig % 2) * 100, req_mem + (sig % 2) * 200 * MiB
    if full:                                                       # no free pod slot from the start: every fourth node, new ones included
        npods = kw.get("init_npods", np.zeros(N, np.int32)).copy()
        npods[np.arange(N) % 4 == 2] = 12
        kw["init_npods"] = npods
    if mask:                                                       # pod classes 0 and 2 may not use some nodes, among them nodes of the last blocks
        ok = np.ones((3, N), bool)
        ok[0, np.arange(N) % 3 == 1] = False
        ok[2, np.arange(N) % 5 == 4] = False
        m = np.zeros((3, (N + 63) // 64), np.uint64)
        for c, j in zip(*np.nonzero(ok)):
            m[c, j // 64] |= np.uint64(1) << np.uint64(j % 64)
        kw["static_mask"], kw["static_reason"] = m, np.where(ok, 0, 2).astype(np.uint8)
    gate = np.full(P, -1, np.int32)
    if presets:                                                    # bound pods, gated on their node (cluster nodes and new ones)
        pr = np.full(P, -1, np.int32)
        idx = rng.choice(P, P // 10, replace=False)
        pr[idx] = rng.integers(0, N, len(idx))
        kw["preset_node"] = pr
        gate = np.maximum(gate, pr)
    if gates:                                                      # DaemonSet-style pods that exist only with their node
        idx = rng.choice(P, P // 8, replace=False)
        gate[idx] = np.maximum(gate[idx], rng.integers(0, N, len(idx)))
    if presets or gates:
        kw["gate_node"] = gate
    if pins:                                                       # node affinity admits ONE node, some beyond the small scenarios
        pin = np.where(rng.random(P) < 0.2, rng.integers(0, N, P), -1).astype(np.int32)
        kw["pin_node"] = np.where(kw["preset_node"] >= 0, -1, pin).astype(np.int32) if presets else pin
    return capi.Problem(**kw).normalise()


def _growing(where, K=40, seed=1, **feat):
    """The cluster of BASE[where] + 33 new template nodes; scenarios that give the template's class 0 (last only), 1, 15, 16, 17, 32 and 33 nodes, and
    three that end inside the cluster (every class cut)."""
    base = BASE[where]
    have = base.count("T")
    prob = _problem(seed, base + ["T"] * 33, SHAPE, K, **feat)
    sizes = [3, 9, len(base) - 1] + [len(base) + c - have for c in (0, 1, 15, 16, 17, 32, 33) if c >= have]
    return prob, sizes


def _entries(n_single, grow_to):
    """n_single classes of one node each (one block each) and one class of 1 .. grow_to nodes behind them: n_single + 1 and n_single + 2 summary entries."""
    shapes = {f"s{i}": (4000 + 500 * i, 16 * GiB) for i in range(n_single)}
    shapes["T"] = SHAPE["T"]
    prob = _problem(7, list(shapes)[:n_single] + ["T"] * grow_to, shapes, 40, init=True)
    return prob, [n_single // 2, n_single + 1, n_single + 15, n_single + 16] + ([n_single + 17] if grow_to > 16 else [])


CASES = {
    "last": lambda: _growing("last"),
    "first": lambda: _growing("first"),
    "middle": lambda: _growing("middle"),
    "entries64": lambda: _entries(63, 16),                         # 64 summary entries at most: one per lane
    "entries65": lambda: _entries(63, 17),                         # 64 and 65: two per lane
    "classes72": lambda: _entries(71, 17),                         # more than 64 node classes: two per lane in the prologue's scan
    "sigs1": lambda: _growing("last", K=1),
    "sigs64": lambda: _growing("middle", K=63),                    # + the signature that never fits: 64, one per lane
    "sigs65": lambda: _growing("middle", K=64),                    # 65: two per lane
    "sigs128": lambda: _growing("last", K=127),
    "mask": lambda: _growing("last", seed=3, mask=True),
    "init_nz": lambda: _growing("middle", seed=4, init=True),
    "full_nodes": lambda: _growing("last", seed=5, full=True, init=True),
    "preset_pin_gate": lambda: _growing("first", seed=6, presets=True, pins=True, gates=True, mask=True),
}
_REF = {}


def _case(name):
    """(problem, scenarios, orders, oracle result), computed once; the oracle must place some pods and refuse some, or a wrong zero byte could hide."""
    if name not in _REF:
        prob, sizes = CASES[name]()
        assert prob.n_pods <= 300 and prob.n_nodes <= 120
        rng = np.random.default_rng(99)
        orders = np.stack([np.arange(P, dtype=np.int32), rng.permutation(P).astype(np.int32)])
        scen = np.array([[n, o] for n in sizes for o in (0, 1)], np.int32)
        assert len(scen) <= 48
        ref = O.run(prob, scen, orders)
        assert (ref.placement >= 0).any() and (ref.unscheduled > 0).any(), name
        _REF[name] = (prob, scen, orders, ref)
    return _REF[name]


def _device(prob, scen, orders, monkeypatch, capfd, shared, ranks=None, segments=None):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    if shared:
        monkeypatch.delenv("SIMON_NO_SHARED_PROLOGUE", raising=False)
    else:
        monkeypatch.setenv("SIMON_NO_SHARED_PROLOGUE", "1")
    capfd.readouterr()
    with capi.Context(0) as ctx:                                   # (a fresh context: the knobs are read when it is created)
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        if segments is not None:
            ctx.set_scenario_segments(*segments)
        if ranks is not None:
            ctx.set_node_ranks(ranks)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        st = ctx.stats()
    route = capfd.readouterr().err
    assert st.kernel_generation == 4, (st.kernel_generation, st.kernel_variant, route)
    unit = re.findall(r"\[route\] unit (\S+) nzeq \d team \d+ prologue (\S+)", route)
    assert len(unit) == 1, route
    return res, unit[0], route


def _same(a, b, what):
    assert a.placement.tolist() == b.placement.tolist(), f"{what}: placements differ"
    assert a.unscheduled.tolist() == b.unscheduled.tolist(), f"{what}: unscheduled counts differ"
    assert a.used_cpu.tolist() == b.used_cpu.tolist() and a.used_mem.tolist() == b.used_mem.tolist(), f"{what}: used cpu / memory differ"


@pytest.mark.parametrize("name", list(CASES))
def test_copy_matches_evaluation_and_oracle(name, monkeypatch, capfd):
    prob, scen, orders, ref = _case(name)
    copied, unit_c, route = _device(prob, scen, orders, monkeypatch, capfd, shared=True)
    evaluated, unit_e, _ = _device(prob, scen, orders, monkeypatch, capfd, shared=False)
    assert unit_c == ("simon_table", "shared-image") and unit_e == ("simon_table", "per-scenario"), (unit_c, unit_e)
    want = {"sigs1": 1, "sigs64": 64, "sigs65": 65, "sigs128": 128}.get(name)     # (K + 1: the signature that never fits)
    if want:
        assert [int(x) for x in re.findall(r"n_sigs (\d+)", route)][-1] == want
    _same(copied, evaluated, "shared image against per-scenario prologue")
    _same(copied, ref, "shared image against the oracle")
    _same(evaluated, ref, "per-scenario prologue against the oracle")


def test_ranked_batch_keeps_the_per_scenario_prologue(monkeypatch, capfd):
    prob, scen, orders, _ = _case("middle")
    rng = np.random.default_rng(5)
    ranks = np.zeros((len(scen), prob.n_nodes), np.int32)
    for s, (n, _o) in enumerate(scen.tolist()):
        ranks[s, :n] = rng.permutation(n)
    ref = O.run(prob, scen, orders, node_ranks=ranks)
    assert (ref.placement >= 0).any() and (ref.unscheduled > 0).any()
    res, unit, _ = _device(prob, scen, orders, monkeypatch, capfd, shared=True, ranks=ranks)
    assert unit == ("simon_table", "per-scenario"), unit
    _same(res, ref, "ranked batch against the oracle")


def test_segmented_batch_keeps_the_per_scenario_prologue(monkeypatch, capfd):
    base = BASE["middle"]
    prob = _problem(8, base + ["T"] * 20 + ["U"] * 20, SHAPE, 40, mask=True)          # (a segment node may not start with pods bound to it)
    seg_start = np.array([len(base), len(base) + 20], np.int32)
    counts = np.array([[0, 0], [1, 17], [16, 0], [17, 3], [20, 20], [0, 16]], np.int32)
    scen = np.array([[len(base) + int(counts[s].sum()), s % 2] for s in range(len(counts))], np.int32)
    orders = np.stack([np.arange(P, dtype=np.int32), np.random.default_rng(3).permutation(P).astype(np.int32)])
    res, unit, route = _device(prob, scen, orders, monkeypatch, capfd, shared=True, segments=(seg_start, counts))
    assert unit == ("simon_table", "per-scenario"), unit
    assert "segmented batch" in route
    placed = unsched = 0
    for s in range(len(counts)):
        row, r = MU.oracle_of_restricted(prob, MU.present_mask(prob.n_nodes, seg_start, counts[s]), orders[scen[s, 1]])
        assert res.placement[s].tolist() == row.tolist(), f"scenario {s}: placements differ"
        assert int(res.unscheduled[s]) == int(r.unscheduled[0]) and int(res.used_cpu[s]) == int(r.used_cpu[0]) and int(res.used_mem[s]) == int(r.used_mem[0])
        placed += int((row >= 0).sum())
        unsched += int(r.unscheduled[0])
    assert placed > 0 and unsched > 0

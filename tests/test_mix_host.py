"""Node-type mixes (simon_set_scenario_segments, simulate.sweep_mix) on the host: the C-ABI surface, the mirror's per-mix answers against
hand-built Simulate() calls of every mix, the best-mix rule, and the pool layout a segmented batch is built on.  No GPU."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import mix_util as MU
from open_simulator_amd import capi, k8s, simulate as sim, workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the oracle engine has no pool segments: sweep_mix runs its mixes one by one and says so (test_fallback_is_visible)
pytestmark = pytest.mark.filterwarnings("ignore::open_simulator_amd.simulate.MixFallbackWarning")


def test_abi_declares_and_exports_the_segment_setter():
    with open(os.path.join(ROOT, "include", "simon_hip.h")) as f:
        hdr = f.read()
    assert "int simon_set_scenario_segments(simon_ctx* ctx, int32_t n_seg, const int32_t* seg_start, const int32_t* count" in hdr
    assert "#define SIMON_MAX_SEGMENTS 8" in hdr and capi.MAX_SEGMENTS == 8
    assert "simon_set_scenario_segments" in capi.EXPORTS
    assert "#define SIMON_HIP_ABI_VERSION 7 " in hdr and capi.ABI_VERSION == 7
    lib = ctypes.CDLL(capi.library_path())
    assert hasattr(lib, "simon_set_scenario_segments") and lib.simon_hip_version() == 7
    assert hasattr(sim.HipEngine, "supports_scenario_segments") and sim.HipEngine.supports_scenario_segments


@pytest.mark.parametrize("case", ["simple", "gpushare", "open_local"])
def test_sweep_mix_equals_simulate_of_every_mix_on_the_reference_examples(case):
    cluster, apps, types = {"simple": MU.example_simple, "gpushare": MU.example_gpushare, "open_local": MU.example_open_local}[case]()
    grid = [range(0, 3), range(0, 2)]
    sw = sim.sweep_mix(cluster, apps, types, grid, engine=MU.OracleEngine())
    assert sw.counts == list(itertools.product(range(0, 3), range(0, 2))) and not sw.batched
    for s, mix in enumerate(sw.counts):
        res, where, nodes = MU.mix_answer(cluster, apps, types, mix)
        assert sw.unscheduled[s] == len(res.unscheduled_pods), mix
        placed = sum(len(st["pods"]) for st in res.node_status)
        assert placed + len(res.unscheduled_pods) == len(where) and len(res.node_status) == len(nodes)
    if sw.best is not None:
        res, where, _ = MU.mix_answer(cluster, apps, types, sw.best)
        got = {(p["metadata"].get("namespace", ""), p["metadata"]["name"]): st["node"]["metadata"]["name"]
               for st in sw.result.node_status for p in st["pods"]}
        assert got == {k: v for k, v in where.items() if v is not None}


def test_sweep_mix_on_a_random_cluster_with_daemonsets_over_two_zones():
    cluster, apps, types = MU.random_zoned(7)
    sw = sim.sweep_mix(cluster, apps, types, [range(0, 3), range(0, 3)], engine=MU.OracleEngine())
    for s, mix in enumerate(sw.counts):
        res, where, nodes = MU.mix_answer(cluster, apps, types, mix)
        assert sw.unscheduled[s] == len(res.unscheduled_pods), mix
    # sweep_mix's own answer: the best mix's nodes are the cluster plus its clones, each running exactly one DaemonSet pod
    assert sw.best is not None
    _, where, nodes = MU.mix_answer(cluster, apps, types, sw.best)
    assert [st["node"]["metadata"]["name"] for st in sw.result.node_status] == [n["metadata"]["name"] for n in
                                                                               [nodes[j] for j in k8s.canonical_node_order(nodes)]]
    for st in sw.result.node_status:
        assert sum(p["metadata"]["name"].startswith("agent") for p in st["pods"]) == 1, st["node"]["metadata"]["name"]
    got = {(p["metadata"].get("namespace", ""), p["metadata"]["name"]): st["node"]["metadata"]["name"] for st in sw.result.node_status for p in st["pods"]}
    assert got == {k: v for k, v in where.items() if v is not None}


@pytest.mark.parametrize("case", ["simple", "open_local"])
def test_one_type_equals_sweep_field_by_field(case):
    cluster, apps, types = {"simple": MU.example_simple, "open_local": MU.example_open_local}[case]()
    one = sim.sweep(cluster, apps, types[0], range(0, 5), engine=MU.OracleEngine())
    mix = sim.sweep_mix(cluster, apps, types[:1], [range(0, 5)], engine=MU.OracleEngine())
    assert [m[0] for m in mix.counts] == one.counts
    assert mix.unscheduled == one.unscheduled and mix.cpu_pct == one.cpu_pct and mix.mem_pct == one.mem_pct
    assert mix.vg_pct == one.vg_pct and mix.needs_reference == one.needs_reference
    assert (None if mix.best is None else mix.best[0]) == one.best
    if one.best is not None:
        def by_name(r):
            return {st["node"]["metadata"]["name"]: sorted(p["metadata"]["name"] for p in st["pods"]) for st in r.node_status}
        assert by_name(mix.result) == by_name(one.result)


def test_best_mix_rule_costs_and_ties():
    mixes = [(0, 2), (1, 1), (2, 0), (0, 3), (3, 0), (1, 0)]
    ok = [0, 1, 2, 3, 4]
    assert sim._best_mix(mixes, ok, [1, 1]) == 0                 # cost 2 three ways: fewest nodes tie too -> smallest vector (0, 2)
    assert sim._best_mix(mixes, ok, [1, 3]) == 2                 # (2, 0) costs 2, (1, 1) 4, (0, 2) 6
    assert sim._best_mix(mixes, ok, [3, 1]) == 0
    assert sim._best_mix(mixes, ok, [2, 3]) == 2                 # (2, 0) 4 < (1, 1) 5 < (0, 2) 6
    assert sim._best_mix(mixes, [3, 4], [1.5, 1.5]) == 3         # equal cost and size: lexicographically smallest
    assert sim._best_mix(mixes, [], [1, 1]) is None


def test_best_mix_under_caps():
    cluster, apps, types = MU.example_open_local()
    free = sim.sweep_mix(cluster, apps, types, [range(0, 4), range(0, 2)], engine=MU.OracleEngine())
    capped = sim.sweep_mix(cluster, apps, types, [range(0, 4), range(0, 2)], engine=MU.OracleEngine(), max_vg=9)
    ok = [s for s in range(len(capped.counts)) if capped.unscheduled[s] == 0 and capped.vg_pct[s] <= 9]
    assert capped.best == (None if not ok else capped.counts[sim._best_mix(capped.counts, ok, [1, 1])])
    assert capped.vg_pct == free.vg_pct
    costly = sim.sweep_mix(cluster, apps, types, [range(0, 4), range(0, 2)], costs=[5, 1], engine=MU.OracleEngine())
    okc = [s for s in range(len(costly.counts)) if costly.unscheduled[s] == 0]
    if okc:
        b = sim._best_mix(costly.counts, okc, [5, 1])
        assert costly.best == costly.counts[b] and costly.cost == 5 * costly.counts[b][0] + costly.counts[b][1]


def test_mix_pool_names_gates_and_layout():
    cluster, apps, types = MU.random_zoned(3, n_types=3, zones=("za", "zb", "zc"))
    top = [2, 3, 1]
    typed = sim.mix_fake_nodes(types, top)
    assert [n["metadata"]["name"] for n in typed[0]] == [n["metadata"]["name"] for n in wl.new_fake_nodes(types[0], 2)]
    names = [n["metadata"]["name"] for nn in typed for n in nn] + [n["metadata"]["name"] for n in cluster["Node"]]
    assert len(set(names)) == len(names)
    assert [n["metadata"]["labels"][k8s.LABEL_HOSTNAME] for n in typed[1]] == [n["metadata"]["name"] for n in typed[1]]
    base = cluster["Node"]
    pool = base + [n for nn in typed for n in nn]
    pods, gates = sim.build_stream(cluster, apps, pool, len(base))
    idx = {n["metadata"]["name"]: j for j, n in enumerate(pool)}
    for p, g in zip(pods, gates):
        if p.get("_daemon_node") in idx and idx[p["_daemon_node"]] >= len(base):
            assert g == idx[p["_daemon_node"]]
        else:
            assert g == -1
    # ranks of every mix, vectorised, against nodeTree.list() of the mix's own node list
    mixes = list(itertools.product(range(3), range(4), range(2)))
    starts = np.cumsum([len(base)] + top[:-1])
    present = np.ones((len(mixes), len(pool)), bool)
    for g, st in enumerate(starts):
        present[:, st:st + top[g]] = np.arange(top[g])[None, :] < np.array(mixes)[:, g:g + 1]
    ranks = sim.mix_node_ranks(pool, present)
    for s, mix in enumerate(mixes):
        own = np.flatnonzero(present[s])
        order = k8s.canonical_node_order([pool[j] for j in own])
        want = np.full(len(pool), -1)
        want[own[order]] = np.arange(len(own))
        assert ranks[s].tolist() == want.tolist(), mix


def test_fallback_is_visible_and_arguments_are_checked():
    cluster, apps, types = MU.example_simple()
    with pytest.warns(sim.MixFallbackWarning, match="no pool segments"):
        sw = sim.sweep_mix(cluster, apps, types, [range(0, 2), range(0, 2)], engine=MU.OracleEngine())
    assert not sw.batched and sw.fallback == "the engine has no pool segments"
    for kw in ({"costs": [1]}, {"costs": [1, 2, 3]}):
        with pytest.raises(ValueError, match="costs"):
            sim.sweep_mix(cluster, apps, types, [range(0, 2), range(0, 2)], engine=MU.OracleEngine(), **kw)
    with pytest.raises(ValueError, match="at least one count"):
        sim.sweep_mix(cluster, apps, types, [range(0, 2), []], engine=MU.OracleEngine())
    with pytest.raises(ValueError, match="one count list per"):
        sim.sweep_mix(cluster, apps, types, [range(0, 2)], engine=MU.OracleEngine())


def test_permute_nodes_keeps_the_oracle_s_answer():
    """The yardstick of the GPU mix tests: moving nodes a scenario lacks behind it, in any order, changes no placement."""
    import oracle_lib as O
    import randprob
    for seed, kw in ((1, dict(gates=True, presets=True, init_state=True)), (2, dict(gpu=True, anti=True)),
                     (3, dict(spread_soft=True, static_mask=True)), (4, dict(local=True, pins=True, gates=True))):
        prob = randprob.rand_problem(seed, N=30, P=120, **kw)
        order = np.arange(prob.n_pods, dtype=np.int32)
        ref = O.run(prob, [[20, 0]], order[None]).placement[0]
        rng = np.random.default_rng(seed)
        perm = np.concatenate([np.arange(20), 20 + rng.permutation(10)])
        row = O.run(MU.permute_nodes(prob, perm), [[20, 0]], order[None]).placement[0]
        assert np.where(row >= 0, perm[np.maximum(row, 0)], row).tolist() == ref.tolist()
        present = np.arange(30) < 20
        assert MU.oracle_of_scenario(prob, present, order)[0].tolist() == ref.tolist()


# ---- the yardstick of the segmented batches and the fuzz regime's generator (fuzz_mix.py), without a GPU ---------------------------
XCHECK = [(1, dict()), (2, dict(gpu=True, anti=True)), (3, dict(spread_soft=True, static_mask=True)), (4, dict(gates=True, pins=True)),
          (5, dict(spread_soft=True, gpu=True, eph=True, scalars=2, gates=True)),
          (6, dict(anti_host=True, ports=True, pins=True, presets=True, init_state=True))]


@pytest.mark.parametrize("seed,kw", XCHECK, ids=[str(x[0]) for x in XCHECK])
def test_the_oracle_on_a_scenario_s_nodes_alone_agrees_with_the_permuted_problem(seed, kw):
    """oracle_of_scenario sees a segmented scenario as a prefix of the node-permuted problem (absent nodes behind it).  Second opinion:
    the oracle on a problem that holds the scenario's nodes ALONE (restrict_nodes: every node-indexed field sliced, built without
    permute_nodes).  Presence masks with absent nodes BETWEEN present ones: prefixes of several segments, and any subset at all; pool
    order and caller rank rows; gates and pins that name absent nodes."""
    import randprob
    rng = np.random.default_rng(seed)
    N = 70
    prob, F = MU.segmentable(randprob.rand_problem(seed, N=N, P=200, **kw), fixed=20)
    masks = []
    for _ in range(3):
        starts = np.sort(np.concatenate([[F], rng.choice(np.arange(F + 1, N), 3, replace=False)]))
        lens = np.append(starts[1:], N) - starts
        masks.append(MU.present_mask(N, starts, [int(rng.integers(0, n + 1)) for n in lens]))
    for _ in range(2):
        m = rng.random(N) < 0.6
        m[:F] = True
        masks.append(m)
    assert any((~m[:np.flatnonzero(m)[-1]]).any() for m in masks)                       # absent nodes between present ones
    for present in masks:
        order = rng.permutation(prob.n_pods).astype(np.int32)
        for ranks in (None, rng.permutation(N)):
            a, ra = MU.oracle_of_scenario(prob, present, order, ranks)
            b, rb = MU.oracle_of_restricted(prob, present, order, ranks)
            assert a.tolist() == b.tolist()
            assert (int(ra.unscheduled[0]), int(ra.used_cpu[0]), int(ra.used_mem[0])) == (int(rb.unscheduled[0]), int(rb.used_cpu[0]), int(rb.used_mem[0]))
            if prob.gpu_mem is not None:
                assert (ra.gpu_slices == rb.gpu_slices).all()
            assert not present[a[a >= 0]].size or present[a[a >= 0]].all()              # nobody lands on an absent node


def test_every_problem_field_says_how_it_depends_on_the_nodes(monkeypatch):
    """mix_util's lists name every field of capi.Problem exactly once; permute_nodes and restrict_nodes refuse a field in no list (a new
    node-indexed field passed through untouched would make the yardstick wrong in silence)."""
    import randprob
    assert MU.unclassified_fields() == ([], [], [])
    prob = randprob.rand_problem(1, N=12, P=20)
    for kind in ("node axis 0", "node-free"):
        lists = dict(MU.FIELD_LISTS, **{kind: MU.FIELD_LISTS[kind][1:]})
        monkeypatch.setattr(MU, "FIELD_LISTS", lists)
        assert len(MU.unclassified_fields()[0]) == 1
        for f in (lambda: MU.permute_nodes(prob, np.arange(12)), lambda: MU.restrict_nodes(prob, np.arange(6))):
            with pytest.raises(KeyError, match="none of mix_util's field lists"):
                f()
        monkeypatch.undo()
    assert MU.unclassified_fields() == ([], [], [])


def _valid_segments(inp):
    """simon_set_scenario_segments' rules (simon_hip.hip), restated: ascending starts inside [0, N], counts within lengths, totals equal
    n_nodes, a node at least in every scenario, no initial state of any kind and no preset pod on a segment node; rank rows
    (simon_set_node_ranks): a permutation over each scenario's own nodes."""
    pr, N, F = inp.prob, inp.prob.n_nodes, int(inp.seg_start[0])
    ends = np.append(inp.seg_start[1:], N)
    assert 1 <= len(inp.seg_start) <= capi.MAX_SEGMENTS and (inp.seg_start >= 0).all() and (inp.seg_start <= ends).all() and ends[-1] == N
    assert inp.counts.shape == (inp.S, len(inp.seg_start)) and (inp.counts >= 0).all() and (inp.counts <= (ends - inp.seg_start)[None]).all()
    assert (F + inp.counts.sum(1) == inp.scen[:, 0]).all() and (inp.scen[:, 0] >= 1).all()
    for name in ("init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem", "init_npods", "init_gpu_used", "init_vg_req",
                 "init_dev_alloc"):
        v = getattr(pr, name)
        assert v is None or not np.asarray(v)[F:].any(), name
    assert pr.init_scalar_req is None or not pr.init_scalar_req[:, F:].any()
    assert pr.preset_node is None or (pr.preset_node < F).all()
    if inp.ranks is not None:
        for s in range(inp.S):
            own = np.flatnonzero(MU.present_mask(N, inp.seg_start, inp.counts[s]))
            assert sorted(inp.ranks[s, own].tolist()) == list(range(len(own)))


def _same(a, b):
    import dataclasses
    for f in dataclasses.fields(a.prob):
        x, y = getattr(a.prob, f.name), getattr(b.prob, f.name)
        if f.name.startswith("_"):
            continue
        assert (x is None) == (y is None) and (x is None or np.array_equal(np.asarray(x), np.asarray(y))), f.name
    for name in ("scen", "orders", "seg_start", "counts", "ranks"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), name
    assert (a.env, a.runs, a.caps, a.feat) == (b.env, b.runs, b.caps, b.feat)


def _array_slice():
    import fuzz_mix
    return [c for c in fuzz_mix.SLICE if c < fuzz_mix.K8S_FIRST]


def test_the_fuzz_generator_is_deterministic_and_draws_valid_segments():
    import fuzz_mix
    for case in list(range(0, 60)) + _array_slice():
        inp = fuzz_mix.draw(case)
        _valid_segments(inp)
        if case in fuzz_mix.SLICE or case < 10:
            _same(inp, fuzz_mix.draw(case))
    shapes = [fuzz_mix.draw(c) for c in range(0, 200)]                                   # the regime reaches the shapes it promises
    seg_len = lambda i: np.append(i.seg_start[1:], i.prob.n_nodes) - i.seg_start       # noqa: E731
    assert any(i.F == 0 for i in shapes) and any((seg_len(i) == 0).any() for i in shapes) and {len(i.seg_start) for i in shapes} == set(range(1, 9))
    assert any((i.counts.sum(1) == 0).any() for i in shapes) and any((i.counts == seg_len(i)[None]).all(1).any() for i in shapes)
    assert any((i.seg_start % 16 != 0).any() for i in shapes) and any(i.ranks is not None and (i.ranks < 0).any() for i in shapes)
    assert any(i.prob.pin_node is not None and i.prob.gate_node is None and (i.prob.pin_node >= i.F).any() for i in shapes)   # pinned, no gate, segment node


def test_the_slice_of_the_fuzz_regime_offers_what_it_is_there_for():
    """Every array-level case of the slice has two or more non-empty segments of which some scenario holds a strict, non-zero prefix (a
    batch with one non-empty segment is a prefix batch in disguise); on the reference's results it places a pod on a segment node in some
    scenario, the cases with gates have a pod gated out of one scenario and placed in another; the slice holds cases with and without
    unscheduled pods, and a multi-segment case for every route family."""
    import fuzz_mix
    uns = []
    for case in _array_slice():
        inp = fuzz_mix.draw(case)
        ref = fuzz_mix.reference(inp)
        assert fuzz_mix.slice_conditions(inp, ref) == [], case
        assert fuzz_mix.n_segments(inp) >= 2, case
        uns.append(int(ref.unscheduled.sum()))
    assert any(u > 0 for u in uns) and any(u == 0 for u in uns)
    covered = {f for c in _array_slice() for f in fuzz_mix.SLICE[c][1]}
    assert covered >= set(fuzz_mix.FAMILIES) - {"multi_segment"}, set(fuzz_mix.FAMILIES) - covered
    assert {1, 2, 3} == {len(fuzz_mix.draw_k8s(c).zones) for c in fuzz_mix.SLICE if c >= fuzz_mix.K8S_FIRST}


PERTURBATIONS = ("count", "rank", "gate")


def test_one_small_change_of_the_device_s_inputs_is_noticed_by_the_slice():
    """The regime can fail: with the oracle on both sides, the "device" is handed VALID inputs that differ from the reference's in one
    small way -- one node of one scenario moved between two segments (same n_nodes), two entries of one caller rank row swapped, one gate
    moved to the neighbouring segment node.  A single such change need not move any pod (the node may be one nobody would use), so no
    single case is required to notice; but each kind of change must be noticed by some case of the slice, or the slice is blind to it."""
    import fuzz_mix
    caught = {how: [] for how in PERTURBATIONS}
    tried = {how: 0 for how in PERTURBATIONS}
    for case in _array_slice():
        inp = fuzz_mix.draw(case)
        ref = fuzz_mix.reference(inp)
        assert fuzz_mix.compare(inp, ref, fuzz_mix.host_device(inp)) == []           # unperturbed: the harness reports nothing
        for how in PERTURBATIONS:
            other = fuzz_mix.perturb(inp, how)
            if other is None:
                continue
            _valid_segments(other)
            tried[how] += 1
            if fuzz_mix.compare(inp, ref, fuzz_mix.host_device(other)):
                caught[how].append(case)
    print("perturbations caught / tried:", {how: (len(caught[how]), tried[how]) for how in PERTURBATIONS})
    for how in PERTURBATIONS:
        assert tried[how] > 0 and caught[how], (how, tried[how])


def test_the_k8s_regime_s_comparison_by_object_names_holds_on_the_oracle():
    """fuzz_mix's k8s-object cases with a segment-capable oracle engine in the device's place: sweep_mix's batched road (pool, gates,
    rank rows, one segment per type) against Simulate() of every mix alone, pods by (namespace, name)."""
    import fuzz_mix

    class Rec(MU.SegmentOracleEngine):
        def run(self, prob, scen, orders, **kw):
            self.seen = (prob, scen, kw)
            self.out = super().run(prob, scen, orders, **kw)
            return self.out

    zones = set()
    for case in range(fuzz_mix.K8S_FIRST, fuzz_mix.K8S_FIRST + 9):
        ok, info = fuzz_mix.one_case_k8s(case, engine=Rec())
        assert ok and not info["refused"], info
        zones.add(info["zones"])
    assert zones == {1, 2, 3}


def test_a_mix_without_any_node_is_refused_up_front():
    """A cluster without nodes and a grid that holds the mix (0, 0): no scenario of no nodes exists anywhere (flatten needs a node, and
    simon_set_scenario_segments refuses an empty scenario), so a segment-capable engine gets a ValueError instead of a batch."""
    cluster, apps, types = MU.random_zoned(7)
    empty = dict(cluster, Node=[])
    with pytest.raises(ValueError, match="at least one new node in every mix"):
        sim.sweep_mix(empty, apps, types, [[0, 1], [0, 2]], engine=MU.SegmentOracleEngine())
    assert sim.sweep_mix(empty, apps, types, [[1, 2], [0, 2]], engine=MU.SegmentOracleEngine()).batched

"""Order rows composed on the device (simon_load_scenarios_composed, simon_orders.hip) and sweep_scale on the product engine: the composed
orders and presence words against OrderSegments.compose() on the word, wave and workgroup edges, from the kernels and from the host
twin (SIMON_ORDER_STAGE=host); a composed batch against the same rows passed explicitly on every kernel route the switches force;
explain_batch with segments; refusals; sweep_scale on HipEngine against the oracle-backed engine.  Run with -m gpu on an MI355X."""
import functools
import warnings

import numpy as np
import pytest

import evict_util as EU
import image_own_util as U
import mix_util as MU
import podset_util as PU
import randk8s
import randprob
import scale_util as XU
from open_simulator_amd import capi, simulate as sim

pytestmark = pytest.mark.gpu

STAGES = ("device", "host")


def _ctx(monkeypatch, stage):
    """A context whose composed rows come from `stage` (the knob is read once, when the context is made); the library says on stderr
    which road every composed load took (SIMON_DEBUG_ROUTE: _stages)."""
    if stage == "host":
        monkeypatch.setenv("SIMON_ORDER_STAGE", "host")
    else:
        monkeypatch.delenv("SIMON_ORDER_STAGE", raising=False)
    monkeypatch.setenv("SIMON_DEBUG_ROUTE", "1")
    return capi.Context(0)


def _stages(capfd):
    """The road of every composed load since the last call, from the library's own lines."""
    import re
    return re.findall(r"\[orders\] stage (\w+) ", capfd.readouterr().err)


# ---- composition -----------------------------------------------------------------------------------------------------------------------
def _cuts(P):
    """Segment boundaries at 0, 1, 32, 33 and P - 1 where P has them, one of them twice: empty segments at the front and inside."""
    cuts = sorted({c for c in (0, 1, 32, 33, P - 1) if 0 <= c <= P})
    return cuts + cuts[-1:]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("n_orders", [1, 5])
@pytest.mark.parametrize("P", [1, 31, 33, 63, 65, 1000])
def test_composed_rows_equal_compose(P, n_orders, stage, monkeypatch, capfd):
    """P: a partial wave, a word tail, a wave boundary crossed, several workgroups.  live in {0, 1, len}; order 0 picks the last variant
    of every segment; S > n_orders, scenarios sharing an order; the words as the library wrote them have no bit at or beyond P."""
    prob = randprob.rand_problem(P, N=6, P=P)
    segs = XU.table_case(P, _cuts(P), 3, n_orders, 7 * P + n_orders, live_values=lambda n: [0, min(1, n), n], last_everywhere=True)
    assert (np.diff(segs.seg_start) == 0).any() and (segs.choice[0] == 2).all()
    orders, present = segs.compose()
    S = n_orders + 3
    scen = np.array([[6 - s % 2, s % n_orders] for s in range(S)], np.int32)
    with _ctx(monkeypatch, stage) as ctx:
        ctx.load_problem(prob)
        capfd.readouterr()
        ctx.load_scenarios_composed(scen, segs)
        assert _stages(capfd) == [stage], "the rows did not come from the road under test"
        got, words = ctx.fetch_orders(0, n_orders, present="words")
        assert (got == orders).all(), np.argwhere(got != orders)[:4].tolist()
        assert words.shape == (n_orders, (P + 31) // 32) and (words == capi.presence_words(present)).all()
        if P % 32:
            assert not (words[:, -1] >> np.uint32(P % 32)).any()
        _, bits = ctx.fetch_orders(n_orders - 1, 1, present=True)
        assert (bits[0] == present[-1]).all()
        # the pod rows are the order's, scenario by scenario: absent pods read GATED
        ctx.run_loaded(False)
        res = ctx.fetch(True)
        assert ((res.placement != capi.GATED) == present[scen[:, 1]]).all()
        # the caller's rows replace them; fetch_orders then reports every pod
        ctx.set_scenario_pods(np.ones((S, P), bool))
        _, bits = ctx.fetch_orders(0, n_orders, present=True)
        assert bits.all()
        # without live: no rows, all ones with a clean tail
        plain = capi.OrderSegments(segs.seg_start, segs.variants, None, segs.choice)
        ctx.load_scenarios_composed(scen, plain)
        assert _stages(capfd) == [stage]
        got, words = ctx.fetch_orders(0, n_orders, present="words")
        assert (got == orders).all() and (words == capi.presence_words(np.ones((n_orders, P), bool))).all()
        ctx.run_loaded(True)
        assert (ctx.fetch(True).placement != capi.GATED).all()
        # after the plain load call the orders come back as given
        ctx.load_scenarios(scen, orders[::-1].copy())
        assert (ctx.fetch_orders(0, n_orders) == orders[::-1]).all()


def _expect(code, match, fn):
    with pytest.raises(capi.SimonError, match=match) as e:
        fn()
    assert e.value.code == code


def test_refusals_and_the_state_machine():
    P = 40
    prob = randprob.rand_problem(3, N=6, P=P)
    segs = XU.table_case(P, [8, 33], 2, 3, 1, live_values=lambda n: [n])
    scen = np.array([[6, 0], [5, 2]], np.int32)
    with capi.Context(0) as ctx:
        _expect(capi.ESTATE, "load nodes, pods", lambda: ctx.load_scenarios_composed(scen, segs))
        ctx.load_problem(prob)
        _expect(capi.ESTATE, "fetch_orders", lambda: ctx.fetch_orders(0, 1))
        for name, want, *table in [t for t in _tables(P) if t[1] != "ok"]:
            bad = capi.OrderSegments(*table)
            _expect(capi.EINVAL, "load_scenarios_composed", lambda: ctx.load_scenarios_composed(scen, bad))
            _expect(capi.ESTATE, "fetch_orders", lambda: ctx.fetch_orders(0, 1))               # a failing call leaves no batch loaded
        # what simon_load_scenarios refuses
        _expect(capi.EINVAL, "order_id", lambda: ctx.load_scenarios_composed(np.array([[6, 3]], np.int32), segs))
        _expect(capi.EINVAL, "n_nodes", lambda: ctx.load_scenarios_composed(np.array([[7, 0]], np.int32), segs))
        # a wrong struct_size
        o, keep = segs.c_struct()
        o.struct_size -= 8
        rc = ctx.lib.simon_load_scenarios_composed(ctx.h, scen.ctypes.data_as(capi.C.POINTER(capi.Scenario)), len(scen), capi.C.byref(o), segs.n_orders)
        assert rc == capi.EINVAL and b"size mismatch" in ctx.lib.simon_last_error(ctx.h)
        ctx.load_scenarios_composed(scen, segs)
        for first, n in [(-1, 1), (0, 0), (3, 1), (2, 2), (0, 4)]:
            _expect(capi.EINVAL, "fetch_orders", lambda: ctx.fetch_orders(first, n))
        assert ctx.fetch_orders(2, 1).shape == (1, P)
        ctx.set_scenario_pods(None)                                    # NULL detaches the composed rows
        ctx.run_loaded(True)
        assert (ctx.fetch(True).placement != capi.GATED).all()


def _tables(P):
    """(name, the restated rule, seg_start, variants, live, choice) over P = 40 pods: tables the library must refuse."""
    ids = np.arange(P, dtype=np.int32)
    a, b = ids[:8], ids[8:]
    yield "good", "ok", [0, 8, P], [[a, a[::-1]], [b]], [[8, 0], [32]], [[1, 0]] * 3
    yield "start", "starts", [0, 8, P - 1], [[a, a[::-1]], [b[:-1]]], None, [[1, 0]] * 3
    yield "pod id", "pod id", [0, 8, P], [[a, a[::-1]], [np.where(b == 20, P, b)]], None, [[1, 0]] * 3
    yield "overlap", "overlap", [0, 8, P], [[a, a[::-1]], [np.where(b == 20, 3, b)]], None, [[1, 0]] * 3
    yield "perm", "not a permutation", [0, 8, P], [[a, np.where(a == 2, 3, a)], [b]], None, [[1, 0]] * 3
    yield "live", "live", [0, 8, P], [[a, a[::-1]], [b]], [[8, 9], [32]], [[1, 0]] * 3
    yield "choice", "choice", [0, 8, P], [[a, a[::-1]], [b]], None, [[1, 0], [2, 0], [0, 0]]


def test_the_refused_tables_are_the_restated_rules():
    """The tables test_refusals_and_the_state_machine loads break the rules scale_util restates (and the first one none)."""
    for name, want, st, variants, live, choice in _tables(40):
        nv = [len(v) for v in variants]
        pods = np.concatenate([np.asarray(v).reshape(-1) for v in variants]).tolist()
        flat_live = None if live is None else [x for l in live for x in l]
        assert XU.segment_error(40, 3, 2, st, nv, pods, flat_live, np.asarray(choice).reshape(-1).tolist()) == want, name


# ---- run parity: composed rows against the same rows passed explicitly, on every route -------------------------------------------------------
def _scenarios(N, n_orders, S=7):
    sizes = [N, N - 1, max(2, N // 2), max(2, N // 6), N, max(2, N // 3), N - 2]
    return np.array([[sizes[s % len(sizes)], (s * 3) % n_orders] for s in range(S)], np.int32)


def _segments_for(P, seed, n_orders=5):
    return XU.table_case(P, [P // 5, P // 5, P // 2 + 1], 3, n_orders, seed, live_values=lambda n: [n, n, (3 * n) // 4, n // 2, 0])


def _parity(prob, scen, segs, **kw):
    """run(order_segments=) against run(orders=, pod_present=) of compose(): placement, unscheduled, used sums, group counts."""
    P = prob.n_pods
    eng = sim.HipEngine()
    group = (np.arange(P) % 3 - (np.arange(P) % 7 == 0)).astype(np.int32)
    a = eng.run(prob, scen, None, order_segments=segs, pod_groups=group, **kw)
    st = eng.last_stats
    orders, present = segs.compose()
    b = eng.run(prob, scen, orders, pod_present=present[scen[:, 1]], pod_groups=group, **kw)
    assert (st.kernel_variant, st.kernel_generation, st.workgroup_size) == (eng.last_stats.kernel_variant, eng.last_stats.kernel_generation, eng.last_stats.workgroup_size)
    assert (a.placement == b.placement).all(), np.argwhere(a.placement != b.placement)[:4].tolist()
    assert ((a.placement != capi.GATED) <= present[scen[:, 1]]).all() and (a.placement == capi.GATED).any() and (a.placement >= 0).any()
    for f in ("unscheduled", "used_cpu", "used_mem", "used_vg", "group_unscheduled", "group_placed"):
        x, y = getattr(a, f, None), getattr(b, f, None)
        assert (x is None) == (y is None) and (x is None or (np.asarray(x) == np.asarray(y)).all()), f
    return a, b, st


PARITY_ROUTES = XU.ROUTES


@pytest.mark.parametrize("ranks", [False, True], ids=["pool_order", "node_ranks"])
@pytest.mark.parametrize("case,env,gen,wg", PARITY_ROUTES, ids=[r[0] for r in PARITY_ROUTES])
def test_composed_batch_equals_explicit_rows_on_the_score_table_routes(case, env, gen, wg, ranks, monkeypatch):
    """gates_fine / gates_coarse: score-table generations without rest; gpu_*: GPU share; anti: the REST path; service_*: generation 7
    behind a Service.  Prefix batches with and without per-scenario node ranks."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, _ = EU.route_problem(case)
    N, P = prob.n_nodes, prob.n_pods
    scen = _scenarios(N, 5)
    kw = {}
    if ranks:
        rng = np.random.default_rng(N)
        rk = np.tile(np.arange(N, dtype=np.int32), (len(scen), 1))
        for s, (n, _) in enumerate(scen.tolist()):
            rk[s, :n] = rng.permutation(n)
        kw["node_ranks"] = rk
    if prob.gpu_mem is not None:
        kw["want_gpu_slices"] = True
    a, b, st = _parity(prob, scen, _segments_for(P, sum(map(ord, case))), **kw)
    assert (st.kernel_variant, st.kernel_generation) == (capi.KERNEL_NARROW_CACHE, gen)
    if prob.gpu_mem is not None:
        assert (a.gpu_slices == b.gpu_slices).all()


@pytest.mark.parametrize("name,env,variant", [("narrow", {"SIMON_NARROW_V1": "1", "SIMON_NO_CACHE": "1"}, capi.KERNEL_NARROW),
                                              ("fast", {"SIMON_NO_CACHE": "1"}, capi.KERNEL_NARROW_FAST),
                                              ("wide", {"SIMON_FORCE_WIDE": "1"}, capi.KERNEL_WIDE)])
def test_composed_batch_on_the_register_kernels_and_the_all_feature_kernel(name, env, variant, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = randprob.rand_problem(41, N=24, P=200, gates=True, nz_differs=True, pins=name == "wide")
    _, _, st = _parity(prob, _scenarios(24, 5), _segments_for(200, 41))
    assert st.kernel_variant == variant


def test_composed_batch_with_open_local_storage():
    """The storage calls replay the stream from the host copy of the loaded orders (h_orders): a composed load reads the rows back."""
    prob = randprob.rand_problem(5, N=30, P=300, local=True, tight_pods=True)
    scen = _scenarios(30, 5)
    ids = np.arange(len(scen), dtype=np.int32)
    a, b, _ = _parity(prob, scen, _segments_for(300, 5), local_usage_of=ids)
    assert (a.local_usage.vg_req == b.local_usage.vg_req).all() and (a.local_usage.dev_alloc == b.local_usage.dev_alloc).all()
    assert (a.local_usage.vg_req > 0).any()


def test_composed_batch_of_an_image_problem_in_a_node_subset_batch():
    """An own-nodes image batch re-stages the tables from the kept orders (img_orders) when the node rows arrive."""
    im, Cp, masks, _ = U.table_case()
    prob, _ = MU.segmentable(randprob.rand_problem(3, N=150, P=120, n_node_classes=5, n_pod_classes=Cp), fixed=0)
    prob = EU.replaced(prob, image_locality=im)
    masks = masks[[0, 5, 11, 17, 23, 29]]
    scen = np.stack([masks.sum(1), np.arange(len(masks)) % 5], 1).astype(np.int32)
    _parity(prob, scen, _segments_for(120, 9), present=(masks, None))
    _parity(prob, _scenarios(150, 5), _segments_for(120, 9))          # ... and the per-size slots of a prefix batch


def test_explain_batch_with_segments_equals_explicit_rows():
    prob, _ = EU.route_problem("gates_fine")
    N, P = prob.n_nodes, prob.n_pods
    scen = _scenarios(N, 5)
    segs = _segments_for(P, 11)
    eng = sim.HipEngine()
    res = eng.run(prob, scen, None, order_segments=segs)
    failing = [s for s in range(len(scen)) if res.unscheduled[s] > 0]
    assert failing, "no scenario leaves a pod unscheduled"
    s = max(failing, key=lambda q: int(res.unscheduled[q]))
    k = int(res.unscheduled[s])
    orders, present = segs.compose()
    a = eng.explain_batch(prob, scen, None, None, [s], k, order_segments=segs)[0]
    b = eng.explain_batch(prob, scen, orders, None, [s], k, pod_present=present[scen[:, 1]])[0]
    assert (a.scenario, a.n_nodes, a.n_failed) == (b.scenario, b.n_nodes, b.n_failed) == (s, int(scen[s, 0]), k)
    assert a.failed.tolist() == b.failed.tolist() and sorted(a.failed.tolist()) == np.flatnonzero(res.placement[s] == capi.UNSCHEDULED).tolist()
    assert a.bins == b.bins and (a.rows is None) == (b.rows is None) and (a.rows is None or (np.asarray(a.rows) == np.asarray(b.rows)).all())
    with pytest.raises(ValueError, match="neither orders nor pod_present"):
        eng.run(prob, scen, orders, order_segments=segs)


# ---- sweep_scale -----------------------------------------------------------------------------------------------------------------------
def _deployment(name, replicas, cpu, mem):
    return {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": name, "namespace": "default"},
            "spec": {"replicas": replicas, "selector": {"matchLabels": {"app": name}},
                     "template": {"metadata": {"labels": {"app": name}},
                                  "spec": {"containers": [{"name": "c", "image": "busybox", "resources": {"requests": {"cpu": cpu, "memory": mem}}}]}}}}


@functools.lru_cache(maxsize=None)
def _scale_case():
    nodes, workloads, services = randk8s.rand_cluster(10, n_nodes=8, n_workloads=20, max_replicas=5)
    cluster = {"Node": nodes, "Service": services}
    app = sim.AppResource("rand", {"Deployment": [w for w in workloads if w["kind"] == "Deployment"] + [_deployment("web", 3, "6", "4Gi"), _deployment("cache", 2, "2", "24Gi")],
                                   "StatefulSet": [w for w in workloads if w["kind"] == "StatefulSet"]})
    tmpl = MU.shaped({"apiVersion": "v1", "kind": "Node", "metadata": {"name": "new", "labels": {"disk": "ssd"}},
                      "status": {"allocatable": {"cpu": "8", "memory": "16Gi", "pods": "20"}, "capacity": {"cpu": "8", "memory": "16Gi", "pods": "20"}}}, 8, "16Gi")
    return cluster, [app], tmpl


def test_sweep_scale_on_the_device_equals_the_oracle_engine():
    """Two targets in one app at [0, 2, 5, 9] each x counts (0, 1), reasons, node table and a headroom probe: HipEngine (rows composed on
    the device) against the oracle-backed engine (rows composed on the host), field by field."""
    cluster, apps, tmpl = _scale_case()
    scale = [("rand", "Deployment", "web", [0, 2, 5, 9]), ("rand", "Deployment", "cache", [0, 2, 5, 9])]
    kw = dict(new_node=tmpl, counts=(0, 1), reasons=True, node_table=True, headroom=[("default", "web-0")])
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.ScaleFallbackWarning)
        a = sim.sweep_scale(cluster, apps, scale, engine=sim.HipEngine(), **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", sim.UsageFallbackWarning)
            warnings.simplefilter("ignore", sim.ScaleFallbackWarning)      # (the host-side usage figures warn under the sweep's class)
            oracle = PU.PodsetOracleEngine()
            b = sim.sweep_scale(cluster, apps, scale, engine=oracle, **kw)
    assert a.batched and b.batched and oracle.batches == 1 and len(a.combos) == 16
    assert 30 <= len(sim.sweep_batch(cluster, sim._scaled_apps(apps, sim._scale_targets(apps, scale), (9, 9)), tmpl, [0, 1]).flat.pods) <= 80
    for f in ("combos", "counts", "unscheduled", "unscheduled_by_target", "cpu_pct", "mem_pct", "vg_pct", "fits", "min_count", "max_level", "needs_reference",
              "headroom", "headroom_exact", "node_table"):
        assert getattr(a, f) == getattr(b, f), f
    ref = lambda lists: [[[((e["pod"]["metadata"].get("namespace"), e["pod"]["metadata"]["name"]), e["reason"]) for e in l] for l in row] for row in lists]   # noqa: E731
    assert ref(a.unscheduled_pods) == ref(b.unscheduled_pods)
    assert any(a.unscheduled[c][0] > 0 for c in range(16)) and any(a.fits[c][0] for c in range(16))

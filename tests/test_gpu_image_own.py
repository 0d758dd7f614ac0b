"""ImageLocality in segmented and node-subset batches on the device (simon_set_image_node_sizes): the staged score table against the
definition without any scheduling run, by the device kernel and by the host loop; node-subset and segmented batches row by row against
the CPU oracle on each scenario's own folded problem, on the score-table kernel and on the all-feature route; explain_own_batch; the
refusals and what they leave behind; sweep_failures and sweep_mix end to end.  Run with -m gpu on an MI355X."""
import functools
import warnings

import numpy as np
import pytest

import evict_util as EU
import explain_own_util as OU
import image_own_util as U
import image_util as IU
import mix_util as MU
import randprob
import subset_util as SU
from open_simulator_amd import capi, flatten as fl, simulate as sim

pytestmark = pytest.mark.gpu

STAGES = ("device", "host")


def _ctx(monkeypatch, stage="device", **env):
    """A context whose image states come from `stage` (the knobs are read once, when the context is made)."""
    if stage == "host":
        monkeypatch.setenv("SIMON_IMAGE_STAGE", "host")
    else:
        monkeypatch.delenv("SIMON_IMAGE_STAGE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return capi.Context(0)


# ---- 1. the staged table against the definition: no scheduling kernel runs -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table():
    im, Cp, masks, _ = U.table_case()
    prob, _ = MU.segmentable(randprob.rand_problem(3, N=150, P=12, n_node_classes=5, n_pod_classes=Cp), fixed=0)
    prob = EU.replaced(prob, image_locality=im)
    want = np.stack([U.own_image_scores(im, m) for m in masks])
    return prob, masks, want


@pytest.mark.parametrize("stage", STAGES)
def test_staged_scores_equal_the_definition_for_every_scenario(stage, monkeypatch):
    """150 nodes, nine images with sizes on the formula's edges (image_own_util.table_case), 84 scenarios: simon_fetch_image_scores of every
    scenario of the node-subset batch equals own_image_scores, whether the device kernel or the host loop built the table."""
    prob, masks, want = _table()
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    orders = np.arange(prob.n_pods, dtype=np.int32)[None]
    with _ctx(monkeypatch, stage) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks)
        for s in range(len(masks)):
            got = ctx.fetch_image_scores(s)
            assert (got == want[s]).all(), (stage, s, np.argwhere(got != want[s])[:4].tolist())


def test_prefix_batch_scores_equal_the_per_size_formula(monkeypatch):
    """The same readback on a prefix batch of the same problem: im.score(c, j, n) on the first n nodes, 0 behind them."""
    prob, _, _ = _table()
    im, N = prob.image_locality, prob.n_nodes
    sizes = [1, 40, 64, 65, 149, 150]
    scen = np.array([[n, 0] for n in sizes], np.int32)
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, np.arange(prob.n_pods, dtype=np.int32)[None])
        for s, n in enumerate(sizes):
            want = np.array([[im.score(c, j, n) if j < n else 0 for j in range(N)] for c in range(prob.n_pod_classes)])
            assert (ctx.fetch_image_scores(s) == want).all(), n


# ---- 2. node-subset batches row by row against the oracle -------------------------------------------------------------------------------
CASES = {"zones": dict(seed=0, zones=True), "services": dict(seed=0), "gpu": dict(seed=4, gpu=True)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(flat, masks, zone, scen, orders, ranks, oracle rows) of a failure case (image_util.image_sweep_case's cluster with three images,
    its workloads without what only the all-feature kernel takes: image_own_util.table_friendly); conditions (a) and (b) asserted on the
    CPU reference alone, the oracle's rows computed once."""
    flat, masks, zone, scen, orders, ranks = U.failure_case(**CASES[name])
    prob = flat.problem
    assert prob.image_locality is not None and prob.image_locality.node_size is not None
    assert U.vacuity(prob, masks, orders, scen, ranks) == (True, True), name
    rows = [MU.oracle_of_scenario(U.fold_images_own(prob, masks[s]), masks[s], orders[scen[s, 1]], ranks[s]) for s in range(len(masks))]
    return flat, masks, zone, scen, orders, ranks, rows


def _assert_rows(res, rows, want_gpu, what=""):
    for s, (row, ref) in enumerate(rows):
        assert res.placement[s].tolist() == row.tolist(), (what, s)
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (int(ref.unscheduled[0]), int(ref.used_cpu[0]), int(ref.used_mem[0])), (what, s)
        if want_gpu:
            assert (res.gpu_slices[s] == ref.gpu_slices[0]).all(), (what, s)


@pytest.mark.parametrize("name", list(CASES))
def test_node_subsets_match_the_oracle_pod_by_pod(name, monkeypatch):
    """24 nodes, about 60 % listing three images with per-node sizes, about 120 pods; the whole cluster, every single node removed and
    eight random subsets.  Every scenario equals the oracle on its own folded problem, and its staged scores equal the definition."""
    flat, masks, zone, scen, orders, ranks, rows = _case(name)
    prob, want_gpu = flat.problem, flat.problem.gpu_mem is not None
    assert 24 == prob.n_nodes and 80 <= prob.n_pods <= 160
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks, zone)
        for s in (0, 1, len(masks) - 1):
            assert (ctx.fetch_image_scores(s) == U.own_image_scores(prob.image_locality, masks[s])).all(), s
        ctx.run_loaded(True, want_gpu)
        res = ctx.fetch(True, want_gpu)
        st = ctx.stats()
    print(f"[{name}] generation {st.kernel_generation}, workgroup {st.workgroup_size}, unscheduled {res.unscheduled.tolist()}")
    assert st.kernel_variant == capi.KERNEL_NARROW_CACHE and st.kernel_generation >= 4
    if name == "services":                                            # the Services' default spread constraints: generation 7
        assert st.kernel_generation == 7
    _assert_rows(res, rows, want_gpu, name)


def test_node_subsets_with_pod_rows(monkeypatch):
    """The same batch with per-scenario pod rows (simon_set_scenario_pods): the image states and the pod rows do not disturb each other."""
    import podset_util as PU
    flat, masks, zone, scen, orders, ranks, _ = _case("services")
    prob = flat.problem
    rng = np.random.default_rng(11)
    pods_in = rng.random((len(masks), prob.n_pods)) < 0.8
    pods_in[0] = True
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_pods(pods_in)
        ctx.set_scenario_nodes(masks, zone)
        ctx.run_loaded(True, False)
        res = ctx.fetch(True, False)
        assert ctx.stats().kernel_generation >= 4
    for s in (0, 3, 7, 25, len(masks) - 1):
        sub, ids = PU.own_problem(U.fold_images_own(prob, masks[s]), pods_in[s])
        row, ref = MU.oracle_of_scenario(sub, masks[s], np.arange(len(ids), dtype=np.int32), ranks[s])
        got = res.placement[s]
        assert got[ids].tolist() == row.tolist(), s
        assert (got[~pods_in[s]] == capi.GATED).all() and int(res.unscheduled[s]) == int(ref.unscheduled[0]), s


def test_node_subsets_with_evicted_pods(monkeypatch):
    """Eviction flags: a few pods bound to nodes and flagged are scheduled like fresh pods where their node is absent, under that
    scenario's own image scores."""
    flat, masks, zone, scen, orders, ranks, _ = _case("services")
    prob = flat.problem
    whole = MU.oracle_of_scenario(U.fold_images_own(prob, masks[0]), masks[0], orders[0], ranks[0])[0]
    picked = np.flatnonzero(whole >= 0)[::9][:8]
    prob2, evict = EU.flag(prob, {int(p): int(whole[p]) for p in picked})
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob2)
        ctx.set_pod_eviction(evict)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks, zone)
        ctx.run_loaded(True, False)
        res = ctx.fetch(True, False)
        assert ctx.stats().kernel_generation >= 4
    moved = 0
    for s in range(len(masks)):
        ps, gone = EU.scenario_problem(prob2, evict, masks[s])
        row, ref = MU.oracle_of_scenario(U.fold_images_own(ps, masks[s]), masks[s], orders[scen[s, 1]], ranks[s])
        assert res.placement[s].tolist() == row.tolist(), s
        moved += int(np.asarray(gone).sum())
    assert moved > 0


# ---- 3. a segmented batch ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix_case(seed=2):
    cluster, apps, tmpl = IU.image_sweep_case(seed, n_nodes=8, n_workloads=14, template_images=True)
    U.three_images(cluster, apps)
    U.table_friendly(apps)
    plain = MU.shaped({k: v for k, v in tmpl.items()}, 8, "16Gi", "plain")
    # (with ONE listing type every present lister has all earlier listers present, and the own reading equals the per-size one by
    # construction: the second type lists the image too, at another size, so that a short first segment shifts its counts)
    plain["status"] = dict(plain["status"], images=[{"names": ["busybox:latest"], "sizeBytes": 300 * IU.MB}])
    types, top = [tmpl, plain], [4, 4]
    base = list(cluster["Node"])
    pool = base + [n for nodes in sim.mix_fake_nodes(types, top) for n in nodes]
    pods, gates = sim.build_stream(cluster, apps, pool, len(base))
    flat = fl.flatten(pool, pods, cluster.get("Service", []), cluster.get("ReplicaSet", []), cluster.get("StatefulSet", []), gates, image_batch="own")
    seg_start = np.array([len(base), len(base) + top[0]], np.int32)
    cnt = np.array([(a, b) for a in range(5) for b in range(5)], np.int32)
    masks = np.stack([MU.present_mask(len(pool), seg_start, c) for c in cnt])
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    orders = np.arange(len(pods), dtype=np.int32)[None]
    prob = flat.problem
    assert U.vacuity(prob, masks, orders, scen) == (True, True)
    rows = [MU.oracle_of_scenario(U.fold_images_own(prob, m), m, orders[0]) for m in masks]
    return cluster, apps, types, prob, seg_start, cnt, masks, scen, orders, rows


def test_segmented_grid_matches_the_oracle(monkeypatch):
    """Two node types, one of whose template lists a 700 MB image, a 5 x 5 grid of counts: every mix equals the oracle on its own folded
    problem."""
    _, _, _, prob, seg_start, cnt, masks, scen, orders, rows = _mix_case()
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(seg_start, cnt)
        for s in (0, 7, 24):
            assert (ctx.fetch_image_scores(s) == U.own_image_scores(prob.image_locality, masks[s])).all(), s
        ctx.run_loaded(True, False)
        res = ctx.fetch(True, False)
        assert ctx.stats().kernel_variant == capi.KERNEL_NARROW_CACHE
    _assert_rows(res, rows, False, "mix")


# ---- 4. the all-feature route ------------------------------------------------------------------------------------------------------------------
def test_all_feature_route_matches_the_oracle(monkeypatch):
    """SIMON_FORCE_WIDE=1 with own_nodes_all_feature: the all-feature kernel reads the same slot array."""
    flat, masks, zone, scen, orders, ranks, rows = _case("services")
    prob = flat.problem
    with _ctx(monkeypatch, SIMON_FORCE_WIDE="1") as ctx:
        ctx.set_own_nodes_all_feature(True)
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks, zone)
        assert (ctx.fetch_image_scores(5) == U.own_image_scores(prob.image_locality, masks[5])).all()
        ctx.run_loaded(True, False)
        res = ctx.fetch(True, False)
        assert ctx.stats().kernel_variant == capi.KERNEL_WIDE
    _assert_rows(res, rows, False, "wide")


# ---- 5. explain_own_batch ----------------------------------------------------------------------------------------------------------------------
def test_explain_own_batch_on_failing_scenarios(monkeypatch):
    """Failed pods and codes of the failing scenarios equal the oracle's explain of the scenario's own folded problem."""
    flat, masks, zone, scen, orders, ranks, rows = _case("services")
    prob = flat.problem
    failing = [s for s, (_, ref) in enumerate(rows) if int(ref.unscheduled[0]) > 0][:6]
    assert failing
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks, zone)
        eb = ctx.explain_own_batch(failing, max_failed=32, max_bins=32, rows=True)
    for k, s in enumerate(failing):
        OU.assert_explained(eb, k, U.fold_images_own(prob, masks[s]), masks[s], orders[scen[s, 1]], ranks[s], 32, 32, True)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def _prefix_equals_per_size(ctx, prob, scen, orders):
    ctx.run_loaded(True, False)
    res = ctx.fetch(True, False)
    ref = IU.oracle_per_size(prob, scen, orders)
    assert (res.placement == ref.placement).all() and res.unscheduled.tolist() == ref.unscheduled.tolist()


def test_refusals_leave_a_working_prefix_batch(monkeypatch):
    flat, masks, zone, _, orders, _, _ = _case("services")
    prob, N = flat.problem, flat.problem.n_nodes
    im = prob.image_locality
    masks = masks[:12]
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    # a node_count that is not the pool-order reading
    bad = capi.ImageLocality(im.size, im.node_off, im.node_image, im.node_count[::-1].copy(), im.class_off, im.class_image, im.node_size).normalise()
    assert (bad.node_count != im.node_count).any()
    bad.node_count = np.clip(bad.node_count, 1, N)
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(EU.replaced(prob, image_locality=bad))
        ctx.load_scenarios(scen, orders)
        with pytest.raises(capi.SimonError, match="arrival order is not pool order") as e:
            ctx.set_scenario_nodes(masks, zone)
        assert e.value.code == capi.EINVAL
        _prefix_equals_per_size(ctx, EU.replaced(prob, image_locality=bad), scen, orders)
    # a table just over a 1 MB cap: the table case's 84 scenarios x 11 rows x 155 classes stay below it, 800 distinct rows do not
    tprob, tmasks, _ = _table()
    rng = np.random.default_rng(9)
    many = np.ones((800, tprob.n_nodes), bool)
    for s in range(800):
        many[s, rng.choice(tprob.n_nodes, 2, replace=False)] = False
    mscen = np.stack([many.sum(1), np.zeros(800, np.int64)], 1).astype(np.int32)
    torders = np.arange(tprob.n_pods, dtype=np.int32)[None]
    with _ctx(monkeypatch, SIMON_IMAGE_STATE_MB="1") as ctx:
        ctx.load_problem(tprob)
        ctx.load_scenarios(mscen, torders)
        with pytest.raises(capi.SimonError, match="image states") as e:
            ctx.set_scenario_nodes(many)
        assert e.value.code == capi.ESTATE
        ctx.run_loaded(True, False)                               # the batch it was: 800 prefix scenarios of 148 nodes, all alike
        res = ctx.fetch(True, False)
        ref = IU.oracle_per_size(tprob, mscen[:1], torders)
        assert (res.placement == ref.placement[0]).all() and (res.unscheduled == ref.unscheduled[0]).all()
        ctx.load_scenarios(mscen[:40], torders)                   # ... and below the cap the same context takes a batch
        ctx.set_scenario_nodes(many[:40])
        assert (ctx.fetch_image_scores(3) == U.own_image_scores(tprob.image_locality, many[3])).all()
    # sizes before image locality; sizes out of range
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(EU.replaced(prob, image_locality=None))
        with pytest.raises(capi.SimonError) as e:
            ctx.set_image_node_sizes(np.zeros(3, np.int64))
        assert e.value.code == capi.ESTATE
        ctx.load_problem(prob)
        with pytest.raises(capi.SimonError) as e:
            ctx.set_image_node_sizes(np.full(len(im.node_image), 1 << 53, np.int64))
        assert e.value.code == -34                                # SIMON_ERANGE
        # without sizes the refusal is the one existing hosts know
        ctx.set_image_node_sizes(None)
        ctx.load_scenarios(scen, orders)
        with pytest.raises(capi.SimonError, match="ImageLocality is in effect") as e:
            ctx.set_scenario_nodes(masks, zone)
        assert e.value.code == capi.ESTATE


def test_sizes_attached_after_the_scenarios(monkeypatch):
    """The header lets simon_set_image_node_sizes come at any time after simon_set_image_locality: after load_scenarios, and detached and
    attached again, the batch is taken and scored like one whose sizes came with the problem."""
    flat, masks, zone, _, orders, ranks, rows = _case("services")
    prob = flat.problem
    im = prob.image_locality
    masks, rows = masks[:8], rows[:8]
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    bare = capi.ImageLocality(im.size, im.node_off, im.node_image, im.node_count, im.class_off, im.class_image).normalise()
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(EU.replaced(prob, image_locality=bare))
        ctx.load_scenarios(scen, orders)
        ctx.set_image_node_sizes(im.node_size)
        ctx.set_scenario_nodes(masks, zone)
        assert (ctx.fetch_image_scores(3) == U.own_image_scores(im, masks[3])).all()
        ctx.run_loaded(True, False)
        _assert_rows(ctx.fetch(True, False), rows, False, "late sizes")
        ctx.set_image_node_sizes(None)                                # detached with the image batch loaded: the scenarios are loaded again
        ctx.load_scenarios(scen, orders)
        ctx.set_image_node_sizes(im.node_size)
        ctx.set_scenario_nodes(masks, zone)
        ctx.run_loaded(True, False)
        _assert_rows(ctx.fetch(True, False), rows, False, "sizes again")


def test_counts_in_a_global_row_per_slot(monkeypatch):
    """150 nodes, 90 images listed on most of them: nnz + I passes the 12 288 int32 the kernel keeps in LDS, so the counts of a slot live
    in a global row.  The table equals the definition, by the kernel and by the host loop."""
    rng = np.random.default_rng(21)
    N, I = 150, 90
    lists = [rng.random(N) < 0.95 for _ in range(I)]
    classes = [[0], [5, 17], [89, 3, 44, -1, 60], [-1]]
    im = U.pool_order_image(rng, N, lists, classes)
    assert len(im.node_image) + I > 12288
    prob, _ = MU.segmentable(randprob.rand_problem(4, N=N, P=12, n_node_classes=5, n_pod_classes=len(classes)), fixed=0)
    prob = EU.replaced(prob, image_locality=im)
    masks = np.stack([np.ones(N, bool), np.arange(N) != 0, np.arange(N) != 77, rng.random(N) < 0.5, rng.random(N) < 0.9, np.arange(N) == N - 1])
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    want = [U.own_image_scores(im, m) for m in masks]
    for stage in STAGES:
        with _ctx(monkeypatch, stage) as ctx:
            ctx.load_problem(prob)
            ctx.load_scenarios(scen, np.arange(prob.n_pods, dtype=np.int32)[None])
            ctx.set_scenario_nodes(masks)
            for s in range(len(masks)):
                assert (ctx.fetch_image_scores(s) == want[s]).all(), (stage, s)


def test_segment_refusals_leave_a_working_prefix_batch(monkeypatch):
    """simon_set_scenario_segments: the pool-order refusal, the cap, and a count beyond its segment while an image batch is loaded.  After
    each the batch runs as the prefix batch it was."""
    _, _, _, prob, seg_start, cnt, masks, scen, orders, rows = _mix_case()
    im, N = prob.image_locality, prob.n_nodes
    bad = capi.ImageLocality(im.size, im.node_off, im.node_image, np.clip(im.node_count[::-1], 1, N).copy(), im.class_off, im.class_image, im.node_size).normalise()
    assert (bad.node_count != im.node_count).any()
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(EU.replaced(prob, image_locality=bad))
        ctx.load_scenarios(scen, orders)
        with pytest.raises(capi.SimonError, match="arrival order is not pool order") as e:
            ctx.set_scenario_segments(seg_start, cnt)
        assert e.value.code == capi.EINVAL
        _prefix_equals_per_size(ctx, EU.replaced(prob, image_locality=bad), scen, orders)
    with _ctx(monkeypatch, SIMON_IMAGE_STATE_MB="0") as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        with pytest.raises(capi.SimonError, match="image states") as e:
            ctx.set_scenario_segments(seg_start, cnt)
        assert e.value.code == capi.ESTATE
        _prefix_equals_per_size(ctx, prob, scen, orders)
    monkeypatch.delenv("SIMON_IMAGE_STATE_MB")
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments(seg_start, cnt)                     # the image batch is in
        ctx.run_loaded(True, False)
        _assert_rows(ctx.fetch(True, False), rows, False, "mix")
        over = cnt.copy()
        over[3, 1] = 9                                                # beyond the segment's four nodes
        with pytest.raises(capi.SimonError, match="outside") as e:
            ctx.set_scenario_segments(seg_start, over)
        assert e.value.code == capi.EINVAL
        _prefix_equals_per_size(ctx, prob, scen, orders)              # ... and out again: per-size slots, a prefix batch
        ctx.set_scenario_segments(seg_start, cnt)
        ctx.run_loaded(True, False)
        _assert_rows(ctx.fetch(True, False), rows, False, "mix again")


def test_back_to_prefix_restores_the_per_size_slots(monkeypatch):
    """set_scenario_nodes(None) after an accepted image batch: the prefix batch with its per-size slots, equal to the per-size oracle."""
    flat, masks, zone, _, orders, _, _ = _case("services")
    prob = flat.problem
    masks = masks[:10]
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    with _ctx(monkeypatch) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_nodes(masks, zone)
        ctx.run_loaded(True, False)
        ctx.set_scenario_nodes(None)
        _prefix_equals_per_size(ctx, prob, scen, orders)


# ---- 7. end to end on HipEngine ------------------------------------------------------------------------------------------------------------------
class _OneByOne(sim.HipEngine):
    """HipEngine without the own image states: the sweeps take their one-by-one road, as on the parent commit."""
    supports_image_own_nodes = False


def _texts(lists):
    return [[(u["pod"]["metadata"].get("namespace"), u["pod"]["metadata"]["name"], u["reason"]) for u in lst] for lst in lists]


def test_sweep_failures_end_to_end():
    cluster, apps, _ = IU.image_sweep_case(2, n_nodes=10, n_workloads=24, listing_share=0.6)
    U.table_friendly(apps)
    with pytest.warns(sim.FailureFallbackWarning, match="ImageLocality"):
        ref = sim.sweep_failures(cluster, apps, "node", engine=_OneByOne(), reasons=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.FailureFallbackWarning)
        hip = sim.sweep_failures(cluster, apps, "node", engine=sim.HipEngine(), reasons=True)
    assert hip.batched and hip.fallback is None and not ref.batched and any(hip.unscheduled)
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.critical, hip.survives) == (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.critical, ref.survives)
    assert hip.placements == ref.placements
    assert _texts(hip.unscheduled_pods) == _texts(ref.unscheduled_pods)


def test_sweep_mix_end_to_end():
    cluster, apps, types = _mix_case()[:3]
    counts = [[0, 1, 2, 4], [0, 1, 3]]
    with pytest.warns(sim.MixFallbackWarning, match="ImageLocality"):
        ref = sim.sweep_mix(cluster, apps, types, counts, engine=_OneByOne(), reasons=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.MixFallbackWarning)
        hip = sim.sweep_mix(cluster, apps, types, counts, engine=sim.HipEngine(), reasons=True)
    assert hip.batched and hip.fallback is None and not ref.batched
    assert (hip.unscheduled, hip.cpu_pct, hip.mem_pct, hip.best, hip.cost) == (ref.unscheduled, ref.cpu_pct, ref.mem_pct, ref.best, ref.cost)
    assert _texts(hip.unscheduled_pods) == _texts(ref.unscheduled_pods)
    assert (hip.result is None) == (ref.result is None)
    if hip.result is not None:
        assert SU.names_of(hip.result) == SU.names_of(ref.result)

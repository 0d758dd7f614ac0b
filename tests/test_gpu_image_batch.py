"""GPU tests of ImageLocality in batched sweeps (ABI v7): the library's per-size image scores against the C oracle on every size's
one-size problem (tests/image_util.py: fold_images), scenario by scenario and row by row, on the score-table kernel and the all-feature
kernel; the FitError replay; a group of two members; sweep() on the engine against its own size-by-size path."""
import re

import numpy as np
import pytest

import image_util as IU
import oracle_lib as O
from open_simulator_amd import capi, flatten as fl, simulate as sim, workloads as wl

pytestmark = pytest.mark.gpu
MB = IU.MB


def _node(name, images=(), cpu="8", mem="16Gi", zone=None):
    labels = {"kubernetes.io/hostname": name}
    if zone is not None:
        labels["topology.kubernetes.io/zone"] = zone
    n = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": name, "labels": labels},
         "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": "40"}, "capacity": {"cpu": cpu, "memory": mem}}}
    if images:
        n["status"]["images"] = [{"names": [nm], "sizeBytes": int(sz)} for nm, sz in images]
    return n


def _pod(name, images, cpu, mem):
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default"},
            "spec": {"containers": [{"name": f"c{i}", "image": im, "resources": {"requests": {"cpu": cpu, "memory": mem}}}
                                    for i, im in enumerate(images)]}}


def _plain(seed, n_cluster, n_clones, n_pods, listing_share=0.5, template_images=True, n_shapes=3, gpu=False):
    """n_shapes node shapes (3: 8 / 16 / 32 cpus; more: distinct cpu counts, one internal node class each); about listing_share of the
    cluster nodes list the pods' images; a template that lists one (or not); gpu: GPU-share capacity on half the nodes, GPU requests
    on a fifth of the pods."""
    rng = np.random.default_rng(seed)
    shapes = [("8", "16Gi"), ("16", "32Gi"), ("32", "64Gi")] if n_shapes == 3 else [(str(8 + k), "64Gi") for k in range(n_shapes)]
    imgs = [("busybox:latest", 300 * MB), ("nginx:1.25", 900 * MB), ("app:2", 2000 * MB)]
    nodes = []
    for j in range(n_cluster):
        cpu, mem = shapes[j % len(shapes)]
        lst = [im for im in imgs if rng.random() < 0.7] if rng.random() < listing_share else []
        nodes.append(_node(f"n{j}", lst, cpu, mem))
        if gpu and j % 2 == 0:
            for part in ("capacity", "allocatable"):
                nodes[-1]["status"][part]["alibabacloud.com/gpu-count"] = "2"
            nodes[-1]["status"]["capacity"]["alibabacloud.com/gpu-mem"] = "32Gi"
    tmpl = _node("tmpl", [imgs[1]] if template_images else (), "16", "32Gi")
    pool = nodes + wl.new_fake_nodes(tmpl, n_clones)
    names = ["busybox", "nginx:1.25", "app:2", "none:1"]
    pods = [_pod(f"p{i}", [names[int(rng.integers(4))] for _ in range(1 + (i % 5 == 0))], f"{int(rng.integers(2, 30)) * 100}m",
                 f"{int(rng.integers(1, 20)) * 256}Mi") for i in range(n_pods)]
    if gpu:
        for i, p in enumerate(pods):
            if i % 5 == 0:
                p["metadata"]["annotations"] = {"alibabacloud.com/gpu-mem": ["2Gi", "4Gi", "8Gi"][i % 3], "alibabacloud.com/gpu-count": "1"}
    return pool, pods, n_cluster


def _run(prob, scen, orders, node_ranks=None, want_gpu_slices=False, group=None):
    ctx = capi.Group(group) if group else capi.Context(0)
    with ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        if node_ranks is not None:
            ctx.set_node_ranks(node_ranks)
        ctx.run_loaded(True, want_gpu_slices)
        res = ctx.fetch(True, want_gpu_slices)
        st = ctx.member_stats(0) if group else ctx.stats()
    return res, st


def _check_rows(prob, scen, orders, res, node_ranks=None, want_gpu_slices=False):
    for s, (n, o) in enumerate(np.asarray(scen)):
        ref = O.run(IU.fold_images(prob, int(n)), [[int(n), int(o)]], orders, want_gpu_slices=want_gpu_slices,
                    node_ranks=None if node_ranks is None else node_ranks[s:s + 1])
        assert res.placement[s].tolist() == ref.placement[0].tolist(), f"scenario {s} ({n} nodes): placements differ"
        assert int(res.unscheduled[s]) == int(ref.unscheduled[0])
        assert int(res.used_cpu[s]) == int(ref.used_cpu[0]) and int(res.used_mem[s]) == int(ref.used_mem[0])
        if want_gpu_slices:
            assert res.gpu_slices[s].tolist() == ref.gpu_slices[0].tolist()


def _batch(pool, pods, n0):
    flat = fl.flatten(pool, pods, image_batch=True)
    assert flat.problem.image_locality is not None
    scen = np.array([[n, 0] for n in range(n0, len(pool) + 1)], np.int32)
    return flat, scen, np.arange(len(pods), dtype=np.int32)[None]


def test_plain_cluster_stays_on_the_score_table():
    pool, pods, n0 = _plain(1, n_cluster=24, n_clones=12, n_pods=160, listing_share=0.3)
    flat, scen, orders = _batch(pool, pods, n0)
    res, st = _run(flat.problem, scen, orders)
    assert st.kernel_generation >= 4, (st.kernel_generation, st.kernel_variant)
    _check_rows(flat.problem, scen, orders, res)
    # ... and the image scores decide something: without them some scenario places differently
    res0, _ = _run(fl.flatten([dict(n, status={k: v for k, v in n["status"].items() if k != "images"}) for n in pool], pods).problem, scen, orders)
    assert res0.placement.tolist() != res.placement.tolist()


@pytest.mark.parametrize("n_shapes,lo,hi,gpu", [(90, 65, 128, False), (170, 129, 256, False), (90, 65, 128, True)])
def test_score_table_beyond_64_node_classes(n_shapes, lo, hi, gpu, monkeypatch, capfd):
    """65 .. 128 internal node classes (two per lane: renormalise's two-half form; with GPU share the REST select's class_term2) and
    129 .. 256 (the four-group form of simon_table_cls4.hip), image scores in the class terms, row by row against the oracle."""
    monkeypatch.setenv("SIMON_DEBUG_ROUTE", "1")
    # (129 .. 256 classes: the one-level layout keeps (signatures x classes) in 64 KB of LDS, hence fewer request signatures)
    pool, pods, n0 = _plain(11 + n_shapes, n_cluster=n_shapes + 40, n_clones=6, n_pods=100 if n_shapes <= 128 else 30, listing_share=0.08,
                            n_shapes=n_shapes, gpu=gpu)
    flat, scen, orders = _batch(pool, pods, n0)
    capfd.readouterr()
    res, st = _run(flat.problem, scen, orders, want_gpu_slices=gpu)
    route = capfd.readouterr().err
    print(route)
    cn_t = [int(x) for x in re.findall(r"Cn_t (\d+)", route)]
    assert st.kernel_variant != capi.KERNEL_WIDE and st.kernel_generation >= 4, (st.kernel_generation, st.kernel_variant)
    assert cn_t and lo <= cn_t[-1] <= hi, cn_t
    _check_rows(flat.problem, scen, orders, res, want_gpu_slices=gpu)


def test_many_image_classes_take_the_all_feature_kernel():
    pool, pods, n0 = _plain(2, n_cluster=300, n_clones=6, n_pods=400, listing_share=1.0)
    flat, scen, orders = _batch(pool, pods, n0)
    res, st = _run(flat.problem, scen, orders)
    assert st.kernel_variant == capi.KERNEL_WIDE
    _check_rows(flat.problem, scen, orders, res)


@pytest.mark.parametrize("seed,template_images,zones,gpu", [(1, False, False, False), (4, True, False, False), (7, True, True, False),
                                                             (3, True, False, True), (12, False, True, True)])
def test_k8s_batches_agree_with_the_oracle_per_size(seed, template_images, zones, gpu):
    """Services (soft spread: generation 7), GPU share, several zones (per-scenario node ranks), a template that lists an image."""
    cluster, apps, template = IU.image_sweep_case(seed, n_nodes=10, n_workloads=10, template_images=template_images, zones=zones, gpu=gpu)
    batch = sim.sweep_batch(cluster, apps, template, [0, 1, 2, 4, 6], image_batch=True)
    prob = batch.flat.problem
    assert prob.image_locality is not None
    want_gpu = prob.gpu_mem is not None
    res, st = _run(prob, batch.scen, batch.orders, batch.node_ranks, want_gpu)
    print(f"seed {seed}: generation {st.kernel_generation} variant {st.kernel_variant}")
    _check_rows(prob, batch.scen, batch.orders, res, batch.node_ranks, want_gpu)


def test_explain_loaded_uses_the_scenario_size():
    pool, pods, n0 = _plain(5, n_cluster=6, n_clones=4, n_pods=220, listing_share=0.6)
    flat, scen, orders = _batch(pool, pods, n0)
    outside = n0 + 1                                          # a size the loaded batch does not have
    scen = scen[scen[:, 0] != outside]
    with capi.Context(0) as ctx:
        ctx.load_problem(flat.problem)
        ctx.load_scenarios(scen, orders)
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        failing = [s for s in range(len(scen)) if res.unscheduled[s] > 0]
        assert failing, "no scenario leaves a pod unscheduled"
        for s in failing[:3]:
            n = int(scen[s, 0])
            nf, failed, codes = ctx.explain_loaded(s, 16)
            _, (rnf, rfailed, rcodes) = O.run(IU.fold_images(flat.problem, n), [[n, 0]], orders, explain_scenario=0, max_failed=16)
            assert nf == rnf and failed.tolist() == rfailed.tolist() and codes.tolist() == rcodes.tolist()
        # a size outside the batch: simon_explain scores the images of THAT size
        n = outside
        assert n not in scen[:, 0].tolist()
        nf, failed, codes = ctx.explain(n, orders[0], 16)
        _, (rnf, rfailed, rcodes) = O.run(IU.fold_images(flat.problem, n), [[n, 0]], orders, explain_scenario=0, max_failed=16)
        assert nf == rnf and failed.tolist() == rfailed.tolist() and codes.tolist() == rcodes.tolist()


def test_group_of_two_members_gives_the_same_answers():
    pool, pods, n0 = _plain(6, n_cluster=20, n_clones=10, n_pods=150)
    flat, scen, orders = _batch(pool, pods, n0)
    one, _ = _run(flat.problem, scen, orders)
    two, _ = _run(flat.problem, scen, orders, group=[0, 0])
    assert two.placement.tolist() == one.placement.tolist() and two.unscheduled.tolist() == one.unscheduled.tolist()
    _check_rows(flat.problem, scen, orders, two)


@pytest.mark.parametrize("seed,template_images", [(2, True), (9, False)])
def test_sweep_on_the_engine_equals_its_size_by_size_path(seed, template_images):
    cluster, apps, template = IU.image_sweep_case(seed, n_nodes=10, n_workloads=10, template_images=template_images)
    counts = list(range(0, 9))
    eng = sim.HipEngine()
    got = sim.sweep(cluster, apps, template, counts, engine=eng)
    ref = sim._sweep_per_size(cluster, apps, template, counts, sim.HipEngine(), 100, 100, 100)
    for f in ("counts", "unscheduled", "cpu_pct", "mem_pct", "best", "vg_pct", "needs_reference"):
        assert getattr(got, f) == getattr(ref, f), f
    assert (got.result is None) == (ref.result is None)
    if got.result is not None:
        assert got.result.node_status == ref.result.node_status


def test_bad_image_inputs_are_refused():
    pool, pods, n0 = _plain(8, n_cluster=6, n_clones=2, n_pods=20)
    flat, scen, orders = _batch(pool, pods, n0)
    im = flat.problem.image_locality
    import copy
    for field, bad, code in (("class_image", lambda a: a.__setitem__(0, len(im.size)), "-22"), ("node_count", lambda a: a.__setitem__(0, 0), "-34"),
                             ("size", lambda a: a.__setitem__(0, -1), "-34")):
        p = copy.copy(flat.problem)
        p.image_locality = copy.deepcopy(im)
        arr = getattr(p.image_locality, field)
        if len(arr) == 0:
            continue
        bad(arr)
        with capi.Context(0) as ctx, pytest.raises(capi.SimonError, match=code):
            ctx.load_problem(p)

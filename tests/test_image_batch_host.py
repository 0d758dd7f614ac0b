"""CPU tests of ImageLocality in batched sweeps (ABI v7): the inputs flatten(image_batch=True) hands the engine, the one-size pod
classes that carry the container images, sweep() over an engine that takes the batch, and the built library's exports."""
import ctypes
import os

import numpy as np
import pytest

import image_util as IU
import oracle_lib as O
import pyref_sched
from open_simulator_amd import capi, flatten as fl, k8s, simulate as sim, workloads as wl

MB = IU.MB


def _node(name, images=(), cpu="8", mem="16Gi"):
    n = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": name, "labels": {"kubernetes.io/hostname": name}},
         "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": "20"}, "capacity": {"cpu": cpu, "memory": mem}}}
    if images:
        n["status"]["images"] = [{"names": list(names), "sizeBytes": int(size)} for names, size in images]
    return n


def _pod(name, images, cpu="100m"):
    return {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default"},
            "spec": {"containers": [{"name": f"c{i}", "image": im, "resources": {"requests": {"cpu": cpu, "memory": "64Mi"}}}
                                    for i, im in enumerate(images)]}}


def _random_pool(seed, n_cluster=7, n_clones=5, template_images=True):
    """cluster nodes + clones of a template (pool order = arrival order), images listed under tagged and untagged names, sizes on
    both sides of 23 MB and of 1000 MB x containers; pods with one to three containers."""
    rng = np.random.default_rng(seed)
    names = ["busybox:latest", "nginx:1.25", "registry.local:5000/app/web:2", "redis:latest", "tiny:1"]
    def imgs():
        out = []
        for nm in names:
            if rng.random() < 0.5:
                size = int(rng.choice([1, 10, 22, 23, 24, 300, 999, 1000, 1001, 2500, 4000])) * MB + int(rng.integers(0, 3))
                out.append(([nm, nm.split(":")[0] + "@sha256:" + str(int(rng.integers(1 << 20)))], size))
        return out
    nodes = [_node(f"n{j}", imgs() if rng.random() < 0.7 else ()) for j in range(n_cluster)]
    tmpl = _node("tmpl", imgs() if template_images else ())
    pool = nodes + (wl.new_fake_nodes(tmpl, n_clones) if n_clones else [])
    refs = ["busybox", "nginx:1.25", "registry.local:5000/app/web:2", "redis", "tiny:1", "unlisted:3", "registry.local:5000/app/web"]
    pods = [_pod(f"p{i}", [refs[int(rng.integers(len(refs)))] for _ in range(int(rng.integers(1, 4)))]) for i in range(14)]
    return pool, pods, len(nodes)


@pytest.mark.parametrize("seed", range(8))
def test_abi_formula_equals_the_one_size_static_add(seed):
    """capi.ImageLocality.score (the ABI's formula) over flatten(image_batch=True)'s arrays = the ImageLocality part of the one-size
    flattening of every prefix of the pool (static_add % 10000), pod by pod and node by node."""
    pool, pods, n0 = _random_pool(seed, template_images=seed % 2 == 0)
    flat = fl.flatten(pool, pods, image_batch=True)
    im = flat.problem.image_locality
    assert im is not None
    if flat.problem.static_add is not None:
        assert (flat.problem.static_add % 10000 == 0).all()          # NodePreferAvoidPods only: the engine adds ImageLocality
    scored = 0
    for n in range(n0, len(pool) + 1):
        one = fl.flatten(pool[:n], pods, image_total=n)
        add = one.problem.static_add
        ncls = one.problem.node_class
        for i in range(len(pods)):
            cb, cr = int(flat.pod_class_of[i]), int(one.pod_class_of[i])
            for j in range(n):
                want = 0 if add is None else int(add[cr, ncls[j]] % 10000)
                assert im.score(cb, j, n) == want, (n, i, j)
                scored += want > 0
    assert scored > 0


def test_default_still_raises_for_a_batch():
    pool, pods, _ = _random_pool(3)
    with pytest.raises(fl.Unsupported, match="ImageLocality"):
        fl.flatten(pool, pods)


def test_pods_that_differ_only_in_their_image_are_two_classes():
    """Two bare pods a (small:1) and b (big:1, 900 MB, listed on n0): b scores 100 x (450 MB - 23 MB) / (1000 MB - 23 MB) = 43 on n0
    in a cluster of two nodes.  The one-size oracle run agrees with the object-level scheduler."""
    nodes = [_node("n0", [(["big:1"], 900 * MB)], cpu="4"), _node("n1", cpu="8")]
    pods = [_pod("a", ["small:1"]), _pod("b", ["big:1"])]
    flat = fl.flatten(nodes, pods, image_total=2)
    assert flat.pod_class_of.tolist() == [0, 1]
    assert flat.problem.static_add is not None
    assert int(flat.problem.static_add[1, flat.problem.node_class[0]] % 10000) == 43
    res = O.run(flat.problem, [[2, 0]], np.arange(2, dtype=np.int32)[None])
    ref = pyref_sched.Scheduler(nodes, [], [], []).run(pods)
    assert [None if j < 0 else flat.node_names[j] for j in res.placement[0].tolist()] == ref


@pytest.mark.parametrize("seed,template_images,zones", [(1, False, False), (4, True, False), (7, True, True), (11, False, True)])
def test_sweep_on_an_image_batch_engine_equals_size_by_size(seed, template_images, zones):
    cluster, apps, template = IU.image_sweep_case(seed, template_images=template_images, zones=zones)
    counts = [0, 1, 2, 3, 5]
    got = sim.sweep(cluster, apps, template, counts, engine=IU.PerSizeOracleEngine())
    ref = sim._sweep_per_size(cluster, apps, template, counts, OracleEngineNoImages(), 100, 100, 100)
    for f in ("counts", "unscheduled", "cpu_pct", "mem_pct", "best", "vg_pct", "needs_reference"):
        assert getattr(got, f) == getattr(ref, f), f
    assert (got.result is None) == (ref.result is None)
    if got.result is not None:
        assert got.result.node_status == ref.result.node_status


def test_sweep_batches_only_where_the_engine_says_so():
    cluster, apps, template = IU.image_sweep_case(4, template_images=True)
    calls = []

    class Counting(IU.PerSizeOracleEngine):
        def run(self, prob, scen, *a, **kw):
            calls.append((prob.image_locality is not None, len(scen)))
            return super().run(prob, scen, *a, **kw)
    sim.sweep(cluster, apps, template, [0, 1, 2], engine=Counting())
    assert calls == [(True, 3)]                                                # one batch, with the image inputs


class OracleEngineNoImages:
    """The one-size path's engine: the C oracle, without supports_image_locality."""

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False):
        assert prob.image_locality is None
        return O.run(prob, scen, orders, want_placement, node_ranks=node_ranks, want_gpu_slices=want_gpu_slices)


def test_library_reports_abi_7_and_exports_the_setters():
    path = capi.library_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: build() first")
    lib = ctypes.CDLL(path)
    assert lib.simon_hip_version() == 7 == capi.ABI_VERSION
    for name in ("simon_set_image_locality", "simon_group_set_image_locality"):
        assert hasattr(lib, name)
    assert "simon_set_image_locality" in capi.EXPORTS and "simon_group_set_image_locality" in capi.EXPORTS

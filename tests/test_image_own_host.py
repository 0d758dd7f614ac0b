"""ImageLocality in own-nodes batches, host side (no GPU): the definition in image_own_util against the existing one-size flattening;
flatten(image_batch="own")'s node sizes; sweep_failures and sweep_mix batching image clusters on a stub engine that answers every scenario
from its own folded problem, against their one-by-one roads."""
import warnings

import numpy as np
import pytest

import image_own_util as U
import image_util as IU
import mix_util as MU
import subset_util as SU
from open_simulator_amd import capi, flatten as fl, simulate as sim

MB = IU.MB


# ---- the helper against the one-size road ---------------------------------------------------------------------------------------------------
def _flat(nodes, pods, cluster, **kw):
    return fl.flatten(nodes, pods, cluster.get("Service", []), cluster.get("ReplicaSet", []), cluster.get("StatefulSet", []), **kw)


def _per_pod(flat):
    """int [P][N]: static_add of every (pod, node) of a flattening, through its classes (None: NodePreferAvoidPods' constant)."""
    pr = flat.problem
    add = np.full((pr.n_pod_classes, pr.n_node_classes), 100 * 10000, np.int64) if pr.static_add is None else np.asarray(pr.static_add, np.int64)
    pc = np.zeros(pr.n_pods, np.int64) if pr.pod_class is None else np.asarray(pr.pod_class, np.int64)
    nc = np.zeros(pr.n_nodes, np.int64) if pr.node_class is None else np.asarray(pr.node_class, np.int64)
    return add[pc][:, nc]


def _subsets(rng, N):
    masks = [np.ones(N, bool)] + [np.arange(N) != j for j in range(N)]
    for _ in range(4):
        m = rng.random(N) < rng.uniform(0.3, 0.9)
        m[int(rng.integers(N))] = True
        masks.append(m)
    return masks


def test_own_scores_equal_the_one_size_flattening_of_the_reduced_cluster():
    """For random image clusters: the whole cluster, each single node removed and a few random subsets.  own_image_scores of the scenario
    equals the ImageLocality part of flatten(reduced nodes, image_total=n)'s static_add, pod by pod, mapped back to pool nodes.  The
    inputs hold a scenario that lacks the first lister of an image whose listers disagree on sizeBytes, and one where a later lister's
    score drops a step against the whole cluster while an earlier lister's does not."""
    lacks_first = later_drops = 0
    for seed in range(4):
        cluster, apps, _ = IU.image_sweep_case(seed, n_nodes=9, n_workloads=8, listing_share=0.7)
        pool = list(cluster["Node"])
        pods, _ = sim.build_stream(cluster, apps, pool, len(pool))
        own = _flat(pool, pods, cluster, image_batch="own")
        im = own.problem.image_locality
        assert im is not None and im.node_size is not None and len(im.node_size) == len(im.node_image)
        base = _per_pod(own)                                          # (without ImageLocality: the batch's static_add leaves it out)
        pc = np.asarray(own.problem.pod_class, np.int64)
        full = U.own_image_scores(im, np.ones(len(pool), bool))
        assert (full == U.per_size_scores(im, np.ones(len(pool), bool))).all()          # the whole pool: the caller's own reading
        for m in _subsets(np.random.default_rng(seed), len(pool)):
            idx = np.flatnonzero(m)
            one = _flat([pool[j] for j in idx], pods, cluster, image_total=len(idx), node_arrival_order=[pool[j]["metadata"]["name"] for j in idx])
            want = _per_pod(one) - base[:, idx]
            got = U.own_image_scores(im, m)
            assert (got[pc][:, idx] == want).all(), (seed, idx.tolist())
            assert not got[:, ~m].any()
            # what the inputs must hold
            for i in range(len(im.size)):
                ent = [(j, q) for j in range(len(pool)) for q in range(int(im.node_off[j]), int(im.node_off[j + 1])) if im.node_image[q] == i]
                if len(ent) < 2:
                    continue
                first = ent[0][0]
                if not m[first] and any(m[j] and im.node_size[q] != im.node_size[ent[0][1]] for j, q in ent[1:]):
                    lacks_first += 1
            listers = [j for j in range(len(pool)) if im.node_off[j + 1] > im.node_off[j]]
            for a in listers:
                for b in listers:
                    if a < b and m[a] and m[b] and ((got[:, b] < full[:, b]) & (got[:, a] >= full[:, a]) & (full[:, a] > 0)).any():
                        later_drops += 1
    assert lacks_first > 0 and later_drops > 0


def test_node_size_of_a_name_listed_under_two_entries():
    """node_size is the sizeBytes of the node's FIRST image that carries the name (cache.go reads the images in order and keeps the first
    summary of a name), also where a later entry repeats the name with another size."""
    def node(name, images):
        return {"apiVersion": "v1", "kind": "Node", "metadata": {"name": name, "labels": {}},
                "status": {"allocatable": {"cpu": "8", "memory": "16Gi", "pods": "20"}, "capacity": {"cpu": "8", "memory": "16Gi"}, "images": images}}
    nodes = [node("a", [{"names": ["app:1"], "sizeBytes": 100 * MB}]),
             node("b", [{"names": ["other:1", "app:1"], "sizeBytes": 300 * MB}, {"names": ["app:1", "app@sha256:1"], "sizeBytes": 700 * MB}]),
             node("c", [])]
    pod = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "p", "namespace": "d", "labels": {}},
           "spec": {"containers": [{"name": "c", "image": "app:1", "resources": {"requests": {"cpu": "1", "memory": "1Gi"}}}]}}
    im = fl.flatten(nodes, [pod], image_batch="own").problem.image_locality
    assert im.size.tolist() == [100 * MB] and im.node_off.tolist() == [0, 1, 2, 2]
    assert im.node_count.tolist() == [1, 2] and im.node_size.tolist() == [100 * MB, 300 * MB]
    # without node a, node b is the first lister: Size = its first entry's 300 MB, NumNodes 1 of 2
    got = U.own_image_scores(im, np.array([False, True, True]))
    assert got[0].tolist() == [0, 100 * (150 * MB - 23 * MB) // (977 * MB), 0]
    one = fl.flatten(nodes[1:], [pod], image_total=2)
    assert (_per_pod(one)[0] - 100 * 10000).tolist() == got[0][1:].tolist()
    # image_batch=True keeps producing today's problem; "own" wants pool order
    assert fl.flatten(nodes, [pod], image_batch=True).problem.image_locality.node_size is None
    with pytest.raises(ValueError, match="pool order"):
        fl.flatten(nodes, [pod], image_batch="own", node_arrival_order=["b", "a", "c"])


# ---- the sweeps on the stub engine -------------------------------------------------------------------------------------------------------------
class _NoOwn(U.OwnImageOracleEngine):
    supports_image_own_nodes = False


def _same_failures(a, b):
    for name in ("domains", "unscheduled", "cpu_pct", "mem_pct", "vg_pct", "survives", "needs_reference", "baseline", "critical", "evicted",
                 "evicted_unscheduled"):
        assert getattr(a, name) == getattr(b, name), name
    assert a.placements == b.placements


@pytest.mark.parametrize("reschedule", [False, "owned"])
def test_sweep_failures_batches_an_image_cluster(reschedule):
    cluster, apps, _ = IU.image_sweep_case(1, n_nodes=8, n_workloads=8, listing_share=0.7)
    if reschedule:                                                    # a few Running pods owned by a ReplicaSet, bound to listing nodes
        import evict_util as EU
        names = [n["metadata"]["name"] for n in cluster["Node"]]
        pods = [EU._pod(f"web-{i}", names[i], "500m", "256Mi", ("ReplicaSet", "web")) for i in range(4)]
        for p in pods:
            p["spec"]["containers"][0]["image"] = "busybox"
        cluster = dict(cluster, Pod=list(cluster.get("Pod", [])) + pods)
    eng = U.OwnImageOracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.FailureFallbackWarning)
        got = sim.sweep_failures(cluster, apps, "node", engine=eng, reschedule=reschedule)
    assert got.batched and got.fallback is None and eng.batches >= 1
    with pytest.warns(sim.FailureFallbackWarning, match="nodes list the pods' images: ImageLocality depends on the node set"):
        ref = sim.sweep_failures(cluster, apps, "node", engine=_NoOwn(), reschedule=reschedule)
    assert not ref.batched and ref.fallback == "nodes list the pods' images: ImageLocality depends on the node set"
    _same_failures(got, ref)
    doms = sim.failure_domains(list(cluster["Node"]), "node")
    with pytest.warns(sim.FailureFallbackWarning):
        each = sim._sweep_failures_each(cluster, apps, doms, U.OwnImageOracleEngine(), sim._caps(100, 100, 100), False, "asked for", reschedule or False)
    _same_failures(got, each)


def test_sweep_mix_batches_an_image_cluster():
    """One template lists an image, one does not."""
    cluster, apps, tmpl = IU.image_sweep_case(3, n_nodes=6, n_workloads=8, template_images=True)
    plain = MU.shaped(dict(tmpl), 8, "16Gi", "plain")
    plain["status"] = {k: v for k, v in plain["status"].items() if k != "images"}
    types, counts = [tmpl, plain], [[0, 1, 3], [0, 2]]
    eng = U.OwnImageOracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.MixFallbackWarning)
        got = sim.sweep_mix(cluster, apps, types, counts, engine=eng)
    assert got.batched and got.fallback is None and eng.batches == 1
    with pytest.warns(sim.MixFallbackWarning, match="nodes list the pods' images: ImageLocality depends on the node set"):
        ref = sim.sweep_mix(cluster, apps, types, counts, engine=_NoOwn())
    assert not ref.batched
    for name in ("counts", "unscheduled", "cpu_pct", "mem_pct", "vg_pct", "needs_reference", "best", "cost"):
        assert getattr(got, name) == getattr(ref, name), name
    assert (got.result is None) == (ref.result is None)
    if got.result is not None:
        assert SU.names_of(got.result) == SU.names_of(ref.result)
    import itertools
    mixes = [tuple(m) for m in itertools.product(*counts)]
    with pytest.warns(sim.MixFallbackWarning):
        each = sim._sweep_mix_per_mix(cluster, apps, types, mixes, [1, 1], U.OwnImageOracleEngine(), sim._caps(100, 100, 100), "asked for", False, None, False, False, False)
    for name in ("counts", "unscheduled", "cpu_pct", "mem_pct", "vg_pct", "needs_reference", "best", "cost"):
        assert getattr(got, name) == getattr(each, name), name


def test_binding_and_engine_surface():
    assert sim.HipEngine.supports_image_own_nodes
    assert "simon_set_image_node_sizes" in capi.EXPORTS and "simon_fetch_image_scores" in capi.EXPORTS
    assert callable(capi.Context.set_image_node_sizes) and callable(capi.Context.fetch_image_scores)
    im, Cp, masks, landmarks = U.table_case()
    assert Cp == 12 and masks.shape == (84, 150) and len(landmarks) == 10
    lens = sorted(int((im.node_image == i).sum()) for i in range(9))
    assert 100 in lens and 64 in lens and 1 in lens and int(im.node_size.max()) == (1 << 53) - 1 and int(im.node_size.min()) == 0

"""Shared helpers of the ImageLocality batch tests (tests/test_image_batch_host.py, tests/test_gpu_image_batch.py, tests/fuzz_images.py).

fold_images(prob, n) is the one-size reading of ABI v7: every node its own class, the image scores of a cluster of n nodes added to
static_add.  The C oracle runs that problem as it runs any one-size flattening."""
import copy

import numpy as np

import randk8s
from open_simulator_amd import capi, k8s, simulate as sim

MB = 1 << 20
TABLES = ("simon_raw", "node_affinity_raw", "taint_prefer_raw", "static_add")


def fold_images(prob: capi.Problem, n: int) -> capi.Problem:
    """prob (with image_locality) -> the same problem for ONE cluster size n, ImageLocality inside static_add."""
    im = prob.image_locality
    out = copy.copy(prob)
    out.image_locality = None
    N, Cp = prob.n_nodes, prob.n_pod_classes
    nc = np.asarray(prob.node_class if prob.node_class is not None else np.zeros(N, np.int32), np.int64)
    for name in TABLES:
        t = getattr(prob, name)
        if t is not None:
            setattr(out, name, np.ascontiguousarray(np.asarray(t, np.int64)[:, nc]))
    add = np.array(out.static_add if out.static_add is not None else np.full((Cp, N), 100 * 10000), np.int64)
    if im is not None:
        for c in range(Cp):
            if not (im.class_image[im.class_off[c]:im.class_off[c + 1]] >= 0).any():
                continue
            for j in range(N):
                add[c, j] += im.score(c, j, n)
    out.static_add = add
    out.node_class = np.arange(N, dtype=np.int32)
    out.n_node_classes = N
    return out.normalise()


def oracle_per_size(prob: capi.Problem, scen, orders, want_gpu_slices=False) -> capi.BatchResult:
    """The oracle on every scenario's one-size problem, stacked like a batch result."""
    import oracle_lib as O
    scen = np.asarray(scen, np.int32).reshape(-1, 2)
    rows = [O.run(fold_images(prob, int(n)), [[int(n), int(o)]], orders, want_gpu_slices=want_gpu_slices) for n, o in scen]
    res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
    for s, r in enumerate(rows):
        res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = r.unscheduled[0], r.used_cpu[0], r.used_mem[0]
        res.placement[s] = r.placement[0]
        if want_gpu_slices and r.gpu_slices is not None:
            res.gpu_slices[s] = r.gpu_slices[0]
    return res


def with_images(nodes, rng, images=("busybox", "nginx:1.25", "registry.local/app/web:2", "redis"), share=0.5):
    """Give about `share` of the nodes container images the generated pods run (and one nobody runs), random sizes around 23 MB .. 2 GB."""
    for n in nodes:
        if rng.random() >= share:
            continue
        lst = [{"names": ["registry.local/other:1.0"], "sizeBytes": 500 * MB}]
        for name in images:
            if rng.random() < 0.6:
                norm = name if name.rfind(":") > name.rfind("/") else name + ":latest"
                lst.append({"names": [norm, name.split(":")[0] + "@sha256:" + format(int(rng.integers(1 << 30)), "x")],
                            "sizeBytes": int(rng.integers(5, 2500)) * MB})
        n.setdefault("status", {})["images"] = lst
    return nodes


def image_sweep_case(seed, n_nodes=8, n_workloads=8, template_images=False, zones=False, gpu=False, max_replicas=6, listing_share=0.5):
    """(cluster, apps, template): a random cluster whose nodes list the apps' images, a new-node template (optionally listing one too)."""
    rng = np.random.default_rng(seed)
    nodes, workloads, services = randk8s.rand_cluster(seed, n_nodes=n_nodes, n_workloads=n_workloads, gpu=gpu, max_replicas=max_replicas)
    if not zones:
        for n in nodes:
            n["metadata"]["labels"].pop(randk8s.ZONE, None)
    images = ("busybox", "nginx:1.25", "registry.local/app/web:2", "redis")
    with_images(nodes, rng, images, listing_share)
    for w in workloads:                                       # the workloads run a mix of those images, some with two containers
        spec = w["spec"]["template"]["spec"] if "template" in w.get("spec", {}) else w["spec"]
        conts = spec.get("containers") or []
        for c in conts:
            c["image"] = images[int(rng.integers(len(images)))]
        if conts and rng.random() < 0.3:
            extra = copy.deepcopy(conts[0])
            extra["name"] = extra.get("name", "c") + "-side"
            extra["image"] = images[int(rng.integers(len(images)))]
            extra.pop("ports", None)
            extra.pop("resources", None)
            conts.append(extra)
    cluster = k8s.group_resources(nodes + services)
    apps = [sim.AppResource("app", k8s.group_resources(workloads))]
    template = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": "tmpl", "labels": {}},
                "status": {"allocatable": {"cpu": "16", "memory": "32Gi", "pods": "30"}, "capacity": {"cpu": "16", "memory": "32Gi"}}}
    if template_images:
        template["status"]["images"] = [{"names": ["busybox:latest"], "sizeBytes": 700 * MB}]
    return cluster, apps, template


class PerSizeOracleEngine:
    """A stub engine that takes the image batch (supports_image_locality) and answers every scenario by a one-size oracle run."""
    supports_image_locality = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False):
        import oracle_lib as O
        scen = np.asarray(scen, np.int32).reshape(-1, 2)
        res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
        for s, (n, o) in enumerate(scen):
            r = O.run(fold_images(prob, int(n)), [[int(n), int(o)]], orders, want_gpu_slices=want_gpu_slices,
                      node_ranks=None if node_ranks is None else node_ranks[s:s + 1])
            res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = r.unscheduled[0], r.used_cpu[0], r.used_mem[0]
            res.placement[s] = r.placement[0]
            if r.used_vg is not None and res.used_vg is not None:
                res.used_vg[s] = r.used_vg[0]
            if want_gpu_slices and r.gpu_slices is not None:
                res.gpu_slices[s] = r.gpu_slices[0]
            if r.preempt_risk is not None:
                if getattr(res, "preempt_risk", None) is None:
                    res.preempt_risk = np.zeros(len(scen), np.uint8)
                res.preempt_risk[s] = r.preempt_risk[0]
        return res

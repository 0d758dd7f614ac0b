"""Shared inputs of the node-type mix tests (test_mix_host.py, test_gpu_mix.py, fuzz_mix.py): the reference's example/ clusters with
two or three new-node types, random k8s clusters over several zones, and the per-mix answer of the CPU oracle keyed by object names."""
import copy
import os

import numpy as np

import oracle_lib as O
import randk8s
import golden_util as G
from open_simulator_amd import capi, k8s, simulate as sim

REF_EXAMPLE = os.path.join(G.GOLDEN, "example")


class OracleEngine:
    """Test-only engine with the HipEngine interface and no pool segments: sweep_mix runs every mix as its own problem on it."""

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False):
        return O.run(prob, scen, orders, want_placement, node_ranks=node_ranks, want_gpu_slices=want_gpu_slices)

    def explain(self, prob, n_nodes, order, max_failed):
        _, (nf, failed, codes) = O.run(prob, [[n_nodes, 0]], np.asarray(order)[None], explain_scenario=0, max_failed=max_failed)
        return nf, failed, codes, O.LAST_LOCAL_DETAIL[0]


def _load(path):
    return k8s.group_resources(k8s.load_objects(os.path.join(REF_EXAMPLE, path)))


def shaped(template, cpu, mem, name=None):
    """A copy of a node template with another allocatable / capacity shape."""
    n = copy.deepcopy(template)
    for k in ("allocatable", "capacity"):
        n.setdefault("status", {}).setdefault(k, {})
        n["status"][k] = dict(n["status"][k], cpu=str(cpu), memory=mem)
    if name:
        n["metadata"]["name"] = name
    return n


def example_simple():
    cluster = _load("cluster/demo_1")
    apps = [sim.AppResource("simple", _load("application/simple"))]
    tmpl = _load("newnode/demo_1")["Node"][0]
    return cluster, apps, [tmpl, shaped(tmpl, 4, "8Gi", "small")]


def example_gpushare():
    cfg = sim.load_config(os.path.join(REF_EXAMPLE, "simon-gpushare-config.yaml"), base_dir=os.path.dirname(REF_EXAMPLE))
    tmpl = cfg["new_node"]
    return cfg["cluster"], cfg["apps"], [tmpl, shaped(tmpl, 8, "16Gi", "gpu-small")]


def example_open_local():
    cluster = _load("cluster/demo_1")
    sim.attach_local_storage(cluster["Node"], os.path.join(REF_EXAMPLE, "cluster/demo_1"))
    yoda = [{"apiVersion": "storage.k8s.io/v1", "kind": "StorageClass", "metadata": {"name": "yoda-lvm-default"}, "parameters": {"volumeType": "LVM"}},
            {"apiVersion": "storage.k8s.io/v1", "kind": "StorageClass", "metadata": {"name": "yoda-device-hdd"},
             "parameters": {"volumeType": "Device", "mediaType": "hdd"}}]
    app = sim.AppResource("open_local", k8s.group_resources(k8s.load_objects(os.path.join(REF_EXAMPLE, "application/open_local")) + yoda))
    tmpl = _load("newnode/demo_1")["Node"]
    sim.attach_local_storage(tmpl, os.path.join(REF_EXAMPLE, "newnode/demo_1"))
    return cluster, [app], [tmpl[0], shaped(tmpl[0], 16, "32Gi", "big")]


def random_zoned(seed, n_nodes=10, n_types=2, zones=("za", "zb")):
    """A random k8s cluster (tests/randk8s.py) over several zones with a DaemonSet, and n_types node types in alternating zones."""
    rng = np.random.default_rng(seed)
    nodes, workloads, services = randk8s.rand_cluster(seed, n_nodes=n_nodes, n_workloads=6, max_replicas=4)
    for j, n in enumerate(nodes):
        n["metadata"].setdefault("labels", {})[k8s.LABEL_ZONE] = zones[int(rng.integers(0, len(zones)))]
    cluster = {"Node": nodes, "Service": services,
               "DaemonSet": [{"apiVersion": "apps/v1", "kind": "DaemonSet", "metadata": {"name": "agent", "namespace": "kube-system"},
                              "spec": {"selector": {"matchLabels": {"app": "agent"}}, "template": {"metadata": {"labels": {"app": "agent"}},
                                       "spec": {"containers": [{"name": "a", "image": "agent", "resources": {"requests": {"cpu": "100m", "memory": "64Mi"}}}]}}}}]}
    apps = [sim.AppResource("rand", {"Deployment": [w for w in workloads if w["kind"] == "Deployment"],
                                     "StatefulSet": [w for w in workloads if w["kind"] == "StatefulSet"]})]
    types = []
    for t in range(n_types):
        tmpl = copy.deepcopy(nodes[t % len(nodes)])
        tmpl["metadata"] = {"name": f"type-{t}", "labels": {k8s.LABEL_ZONE: zones[t % len(zones)], "disk": "ssd"}}
        tmpl.pop("spec", None)
        types.append(shaped(tmpl, [4, 8, 16][t % 3], ["8Gi", "16Gi", "32Gi"][t % 3]))
    return cluster, apps, types


def mix_answer(cluster, apps, new_nodes, mix, engine=None):
    """What Simulate(cluster + NewFakeNodes(type_1, c_1) + ...) gives for one mix, by object names: {(namespace, pod name): node name or
    None}, unscheduled count, used cpu / memory."""
    engine = engine or OracleEngine()
    nodes = list(cluster.get("Node", [])) + [n for nn in sim.mix_fake_nodes(new_nodes, mix) for n in nn]
    res = sim.simulate(dict(cluster, Node=list(cluster.get("Node", []))), apps, engine=engine,
                       new_nodes=[n for nn in sim.mix_fake_nodes(new_nodes, mix) for n in nn])
    where = {}
    for st in res.node_status:
        for p in st["pods"]:
            where[(p["metadata"].get("namespace", ""), p["metadata"]["name"])] = st["node"]["metadata"]["name"]
    for u in res.unscheduled_pods:
        where[(u["pod"]["metadata"].get("namespace", ""), u["pod"]["metadata"]["name"])] = None
    return res, where, nodes


# ---- the oracle's view of one scenario of a segmented batch ------------------------------------------------------------------------
_NODE_1D = ("alloc_cpu", "alloc_mem", "alloc_pods", "alloc_eph", "init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem",
            "init_npods", "node_class", "gpu_cnt", "gpu_mem_total", "local_flags", "local_vg_cnt", "local_dev_cnt", "local_dev_media",
            "init_dev_alloc", "init_gpu_used", "local_vg_cap", "init_vg_req", "local_vg_name", "local_dev_cap")   # node = axis 0
_NODE_COL = ("scalar_alloc", "init_scalar_req", "topo_dom", "static_reason")                                        # node = axis 1
_NODE_BITS = ("static_mask", "node_sets")                                                                            # [rows][words] bitsets
_POD_NODE = ("preset_node", "gate_node", "pin_node")


def _bits_permute(rows, perm, N):
    rows = np.asarray(rows, np.uint64)
    bits = ((rows[:, np.arange(N) // 64] >> (np.arange(N) % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)[:, perm]
    out = np.zeros_like(rows)
    for j in range(N):
        out[:, j // 64] |= bits[:, j].astype(np.uint64) << np.uint64(j % 64)
    return out


def permute_nodes(prob: capi.Problem, perm) -> capi.Problem:
    """The same problem with its nodes reordered: node i of the result is node perm[i] of prob (pod ids, classes and tables unchanged).
    A segmented scenario's nodes moved to the front make it a PREFIX scenario the oracle runs as it stands."""
    import dataclasses
    perm = np.asarray(perm, np.int64)
    N = prob.n_nodes
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    kw = {}
    for f in dataclasses.fields(prob):
        if f.name.startswith("_"):
            continue
        v = getattr(prob, f.name)
        if v is None or not isinstance(v, np.ndarray):
            kw[f.name] = v
        elif f.name in _NODE_1D:
            kw[f.name] = v[perm].copy()
        elif f.name in _NODE_COL:
            kw[f.name] = v[:, perm].copy()
        elif f.name in _NODE_BITS:
            kw[f.name] = _bits_permute(v, perm, N)
        elif f.name in _POD_NODE:
            kw[f.name] = np.where(v >= 0, inv[np.maximum(v, 0)], v).astype(v.dtype)
        else:
            kw[f.name] = v
    return capi.Problem(**kw).normalise()


def oracle_of_scenario(prob, present, order, ranks=None):
    """Oracle placement row (pool node indices, by pod id) of the scenario that holds the pool nodes `present` (bool [N]), its nodes in
    pool order unless `ranks` (its rank row over present nodes) says otherwise."""
    own = np.flatnonzero(present)
    if ranks is not None:
        own = own[np.argsort(np.asarray(ranks)[own], kind="stable")]
    perm = np.concatenate([own, np.flatnonzero(~present)])
    res = O.run(permute_nodes(prob, perm), [[len(own), 0]], np.asarray(order, np.int32)[None])
    row = res.placement[0]
    return np.where(row >= 0, perm[np.maximum(row, 0)], row), res

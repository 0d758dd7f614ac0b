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


class SegmentOracleEngine(OracleEngine):
    """Test-only engine that DOES take pool segments, every scenario through oracle_of_restricted: the device's stand-in where the
    harness around a segmented batch (fuzz_mix.py's comparison by object names) is itself under test on a host without a GPU."""
    supports_scenario_segments = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, segments=None):
        if segments is None:
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices)
        scen = capi.scenarios_array(scen)
        res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
        for s in range(len(scen)):
            row, r = oracle_of_restricted(prob, present_mask(prob.n_nodes, segments[0], np.asarray(segments[1])[s]), np.asarray(orders)[scen[s, 1]],
                                          None if node_ranks is None else node_ranks[s])
            res.placement[s], res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = row, r.unscheduled[0], r.used_cpu[0], r.used_mem[0]
            if want_gpu_slices and r.gpu_slices is not None:
                res.gpu_slices[s] = r.gpu_slices[0]
        self.last_stats = None
        return res


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
# Every field of capi.Problem belongs to exactly one of these lists (test_mix_host.py: the field guard): a node-indexed field that
# permute_nodes / restrict_nodes passed through untouched would make the yardstick of the segmented batches wrong without a failing test.
_NODE_1D = ("alloc_cpu", "alloc_mem", "alloc_pods", "alloc_eph", "init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem",
            "init_npods", "node_class", "gpu_cnt", "gpu_mem_total", "local_flags", "local_vg_cnt", "local_dev_cnt", "local_dev_media",
            "init_dev_alloc", "init_gpu_used", "local_vg_cap", "init_vg_req", "local_vg_name", "local_dev_cap")   # node = axis 0
_NODE_COL = ("scalar_alloc", "init_scalar_req", "topo_dom", "static_reason")                                        # node = axis 1
_NODE_BITS = ("static_mask", "node_sets")                                                                            # [rows][words] bitsets
_POD_NODE = ("preset_node", "gate_node", "pin_node")                                                                 # [P] node index or -1
_NODE_SIZED = ("spread_log",)                          # [N + 1], indexed by a COUNT of nodes: a problem of fewer nodes takes a prefix
_NODE_SET = ("image_locality",)                        # depends on the node set as a whole: no segments with it (SIMON_ESTATE), must be None
_NODE_FREE = ("topo_n_dom", "req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "scalar_req", "pod_class", "gpu_mem", "pod_gpu_cnt", "gpu_index",
              "scalar_entries", "priority", "init_min_priority", "n_pod_classes", "n_node_classes", "simon_raw", "const_score",
              "node_affinity_raw", "taint_prefer_raw", "static_add", "term_topo_key", "term_node_set", "anti_off", "anti_idx", "match_off",
              "match_idx", "port_off", "port_idx", "aff_off", "aff_idx", "class_flags", "pref_off", "pref_idx", "pref_w", "own_off", "own_idx",
              "own_w", "spread_hard_off", "spread_hard_idx", "spread_hard_skew", "spread_hard_self", "spread_hard_set", "spread_soft_off",
              "spread_soft_idx", "spread_soft_skew", "local_spec_of", "local_specs", "topo_is_hostname")
FIELD_LISTS = {"node axis 0": _NODE_1D, "node axis 1": _NODE_COL, "node bitset": _NODE_BITS, "pod -> node": _POD_NODE,
               "sized by nodes": _NODE_SIZED, "node set": _NODE_SET, "node-free": _NODE_FREE}


def problem_fields():
    import dataclasses
    return [f.name for f in dataclasses.fields(capi.Problem) if not f.name.startswith("_")]


def unclassified_fields():
    """Fields of capi.Problem in none of the lists above, and names listed twice or not fields at all (all empty when the lists are right)."""
    listed = [n for names in FIELD_LISTS.values() for n in names]
    fields = problem_fields()
    return ([f for f in fields if f not in listed], sorted({n for n in listed if listed.count(n) > 1}), [n for n in listed if n not in fields])


def _kind_of(name):
    for kind, names in FIELD_LISTS.items():
        if name in names:
            return kind
    raise KeyError(f"capi.Problem.{name} is in none of mix_util's field lists: say how it depends on the nodes")


def segmentable(prob, scen=None, fixed=None):
    """The problem with nodes from `fixed` on (default: the batch's smallest size) made segment-ready: no pod bound there before the
    stream or by Spec.NodeName (a preset pod there keeps its gate and becomes a gated pod that is neither preset nor pinned)."""
    import dataclasses
    F = int(fixed) if fixed is not None else int(np.asarray(scen)[:, 0].min())
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    for name in ("init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem", "init_npods", "init_gpu_used", "init_vg_req",
                 "init_dev_alloc"):
        if kw[name] is not None:
            v = np.array(kw[name])
            v[F:] = 0
            kw[name] = v
    if kw["init_scalar_req"] is not None:
        v = np.array(kw["init_scalar_req"])
        v[:, F:] = 0
        kw["init_scalar_req"] = v
    if kw["preset_node"] is not None:
        pr = np.array(kw["preset_node"])
        if kw["gate_node"] is None:
            kw["gate_node"] = np.full(len(pr), -1, np.int32)
        kw["gate_node"] = np.where(pr >= F, np.maximum(kw["gate_node"], pr), kw["gate_node"]).astype(np.int32)
        kw["preset_node"] = np.where(pr >= F, -1, pr).astype(np.int32)
    return capi.Problem(**kw).normalise(), F


def present_mask(N, seg_start, counts_row):
    """bool [N]: the fixed nodes [0, seg_start[0]) and the first counts_row[g] nodes of every segment."""
    present = np.zeros(N, bool)
    present[:int(seg_start[0])] = True
    for g, st in enumerate(np.asarray(seg_start).tolist()):
        present[st:st + int(counts_row[g])] = True
    return present


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
        kind = _kind_of(f.name)
        if kind == "node set":
            assert v is None, f"{f.name} depends on the node set: no node order but its own"
        if v is None or not isinstance(v, np.ndarray) or kind in ("node-free", "sized by nodes"):
            kw[f.name] = v
        elif kind == "node axis 0":
            kw[f.name] = v[perm].copy()
        elif kind == "node axis 1":
            kw[f.name] = v[:, perm].copy()
        elif kind == "node bitset":
            kw[f.name] = _bits_permute(v, perm, N)
        else:
            kw[f.name] = np.where(v >= 0, inv[np.maximum(v, 0)], v).astype(v.dtype)
    return capi.Problem(**kw).normalise()


def oracle_of_scenario(prob, present, order, ranks=None):
    """Oracle placement row (pool node indices, by pod id) of the scenario that holds the pool nodes `present` (bool [N]), its nodes in
    pool order unless `ranks` (its rank row over present nodes) says otherwise."""
    own = np.flatnonzero(present)
    if ranks is not None:
        own = own[np.argsort(np.asarray(ranks)[own], kind="stable")]
    perm = np.concatenate([own, np.flatnonzero(~present)])
    res = O.run(permute_nodes(prob, perm), [[len(own), 0]], np.asarray(order, np.int32)[None], want_gpu_slices=prob.gpu_mem is not None)
    row = res.placement[0]
    return np.where(row >= 0, perm[np.maximum(row, 0)], row), res


def restrict_nodes(prob: capi.Problem, own):
    """The problem of the nodes `own` ALONE (pool indices, in the scenario's order), every node-indexed field sliced -- built without
    permute_nodes, as the second opinion on it.  Where a gate, pin or preset names a node outside `own`, one such node stays behind the
    scenario's as a placeholder so that the index remains valid (run the result with n_nodes = len(own)).  Returns (problem, nodes):
    nodes[i] = pool index of the result's node i.  What this second opinion cannot see: it reads the same FIELD_LISTS, so a field
    wrongly listed as node-free is wrong in both; it checks how a listed field is gathered (axis, bitset, pod -> node index) and what
    the oracle makes of nodes behind the scenario."""
    import dataclasses
    own = np.asarray(own, np.int64)
    N = prob.n_nodes
    new_of = np.full(N, -1, np.int64)
    new_of[own] = np.arange(len(own))
    named = np.concatenate([np.asarray(getattr(prob, n))[np.asarray(getattr(prob, n)) >= 0] for n in _POD_NODE if getattr(prob, n) is not None] or
                           [np.zeros(0, np.int64)])
    outside = named[new_of[named] < 0]
    nodes = np.concatenate([own, outside[:1]]) if len(outside) else own
    M = len(nodes)
    kw = {}
    for f in dataclasses.fields(prob):
        if f.name.startswith("_"):
            continue
        v = getattr(prob, f.name)
        kind = _kind_of(f.name)
        if kind == "node set":
            assert v is None, f"{f.name} depends on the node set"
        if v is None or not isinstance(v, np.ndarray) or kind == "node-free":
            kw[f.name] = v
        elif kind == "node axis 0":
            kw[f.name] = np.take(v, nodes, axis=0)
        elif kind == "node axis 1":
            kw[f.name] = np.take(v, nodes, axis=1)
        elif kind == "node bitset":
            bits = np.unpackbits(np.ascontiguousarray(v, "<u8").view(np.uint8), axis=1, bitorder="little")[:, nodes]
            bits = np.pad(bits, ((0, 0), (0, -M % 64)))
            kw[f.name] = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(len(v), -1)
        elif kind == "sized by nodes":
            kw[f.name] = v[:M + 1].copy()
        else:   # pod -> node: the scenario's own index, or the placeholder behind it
            kw[f.name] = np.where(v >= 0, np.where(new_of[np.maximum(v, 0)] >= 0, new_of[np.maximum(v, 0)], len(own)), v).astype(v.dtype)
    return capi.Problem(**kw).normalise(), nodes


def oracle_of_restricted(prob, present, order, ranks=None):
    """oracle_of_scenario's answer by the other road: the oracle on restrict_nodes' problem of the scenario's nodes alone."""
    own = np.flatnonzero(present)
    if ranks is not None:
        own = own[np.argsort(np.asarray(ranks)[own], kind="stable")]
    sub, nodes = restrict_nodes(prob, own)
    res = O.run(sub, [[len(own), 0]], np.asarray(order, np.int32)[None], want_gpu_slices=prob.gpu_mem is not None)
    row = res.placement[0]
    return np.where(row >= 0, nodes[np.maximum(row, 0)], row), res

"""Shared helpers of the own-nodes ImageLocality tests (test_image_own_host.py, test_gpu_image_own.py).  Pure Python / NumPy: nothing here
reads the library.

A scenario of a segmented or node-subset batch holds the pool nodes `present`, fed to the scheduler cache in pool order
(schedulerCache.addNodeImageStates, cache.go:675-698): NumNodes of node j's entry of image i = the present listers of i at or before j,
Size(i) = the sizeBytes the first present lister lists, totalNumNodes = the number of present nodes.  own_image_scores restates that;
fold_images_own turns a scenario into the one-size problem the C oracle runs; OwnImageOracleEngine answers own-nodes batches that way."""
import copy

import numpy as np

import evict_util as EU
import image_util as IU
import mix_util as MU
from open_simulator_amd import capi

MB = 1 << 20


def own_image_scores(im: capi.ImageLocality, present) -> np.ndarray:
    """int [Cp][N]: ImageLocality.Score of every (pod class, pool node) in the scenario that holds `present` (bool [N]); 0 for the nodes
    it lacks and for classes without containers."""
    present = np.asarray(present, bool)
    N, Cp = len(im.node_off) - 1, len(im.class_off) - 1
    n = int(present.sum())
    run, size = {}, {}
    cnt = np.zeros(len(im.node_image), np.int64)
    for j in np.flatnonzero(present).tolist():
        for q in range(int(im.node_off[j]), int(im.node_off[j + 1])):
            i = int(im.node_image[q])
            run[i] = run.get(i, 0) + 1
            cnt[q] = run[i]
            size.setdefault(i, int(im.node_size[q]))
    out = np.zeros((Cp, N), np.int64)
    for c in range(Cp):
        e0, e1 = int(im.class_off[c]), int(im.class_off[c + 1])
        if e1 == e0:
            continue
        hi = 1000 * MB * (e1 - e0)
        for j in np.flatnonzero(present).tolist():
            mine = {int(im.node_image[q]): q for q in range(int(im.node_off[j]), int(im.node_off[j + 1]))}
            total = 0
            for e in range(e0, e1):
                i = int(im.class_image[e])
                if i >= 0 and i in mine:
                    total += int(float(size[i]) * (float(int(cnt[mine[i]])) / float(n)))
            total = min(max(total, 23 * MB), hi)
            out[c, j] = 100 * (total - 23 * MB) // (hi - 23 * MB)
    return out


def per_size_scores(im: capi.ImageLocality, present) -> np.ndarray:
    """The per-size reading a prefix batch applies, im.score(c, j, n_s), on the scenario's nodes: what own_image_scores must differ from
    somewhere for an own-nodes case to test anything."""
    present = np.asarray(present, bool)
    N, Cp = len(im.node_off) - 1, len(im.class_off) - 1
    out = np.zeros((Cp, N), np.int64)
    for c in range(Cp):
        for j in np.flatnonzero(present).tolist():
            out[c, j] = im.score(c, j, int(present.sum()))
    return out


def _folded(prob: capi.Problem, scores) -> capi.Problem:
    base = copy.copy(prob)
    base.image_locality = None
    out = IU.fold_images(base, 0)                            # (every node its own class, static_add spelled out; no image part)
    out.static_add = np.asarray(out.static_add, np.int64) + np.asarray(scores, np.int64)
    return out.normalise()


def fold_images_own(prob: capi.Problem, present) -> capi.Problem:
    """prob (image_locality with node_size) -> the problem of the scenario `present`: every node its own class, the scenario's own scores
    inside static_add, no image_locality -- ready for mix_util.oracle_of_scenario(..., present, order, ranks)."""
    return _folded(prob, own_image_scores(prob.image_locality, present))


def fold_images_per_size(prob: capi.Problem, present) -> capi.Problem:
    """The same with the per-size reading: the placement an own-nodes case must NOT be explained by."""
    return _folded(prob, per_size_scores(prob.image_locality, present))


def pool_order_image(rng, N, lists, class_images, sizes=None):
    """capi.ImageLocality in the pool-order reading.  lists[i] = bool [N] listers of image i; class_images = per pod class the image id
    of every container (-1: listed nowhere); sizes[i] = int [N] per-node sizeBytes (default: random 5 MB .. 2.5 GB)."""
    I = len(lists)
    if sizes is None:
        sizes = [rng.integers(5, 2500, N) * MB for _ in range(I)]
    node_off, node_image, node_count, node_size = [0], [], [], []
    run = [0] * I
    size = [0] * I
    for j in range(N):
        for i in range(I):
            if lists[i][j]:
                run[i] += 1
                if run[i] == 1:
                    size[i] = int(sizes[i][j])
                node_image.append(i)
                node_count.append(run[i])
                node_size.append(int(sizes[i][j]))
        node_off.append(len(node_image))
    class_off = np.concatenate([[0], np.cumsum([len(c) for c in class_images])])
    return capi.ImageLocality(np.array(size, np.int64), np.array(node_off, np.int32), np.array(node_image, np.int32), np.array(node_count, np.int32),
                              class_off.astype(np.int32), np.array([i for c in class_images for i in c], np.int32),
                              np.array(node_size, np.int64)).normalise()


def vacuity(prob, masks, orders, scen, ranks=None):
    """(a, b) of an oracle-compared case, from the CPU reference alone: a = at some present node of some scenario the own-state score differs
    from the per-size one; b = in some scenario the oracle places differently under the two."""
    a = b = False
    for s, m in enumerate(np.asarray(masks, bool)):
        if (own_image_scores(prob.image_locality, m) != per_size_scores(prob.image_locality, m)).any():
            a = True
            r = None if ranks is None else ranks[s]
            own, _ = MU.oracle_of_scenario(fold_images_own(prob, m), m, np.asarray(orders)[scen[s][1]], r)
            per, _ = MU.oracle_of_scenario(fold_images_per_size(prob, m), m, np.asarray(orders)[scen[s][1]], r)
            b = b or bool((own != per).any())
        if a and b:
            break
    return a, b


class OwnImageOracleEngine(EU.EvictOracleEngine):
    """Test-only engine that takes an image problem in segmented and node-subset batches (supports_image_own_nodes): every scenario is
    folded to its own one-size problem and answered by the oracle-backed engines of the subset / eviction tests, one at a time."""
    supports_scenario_segments = True
    supports_image_own_nodes = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, evict=None, segments=None):
        if present is None and segments is None:
            assert prob.image_locality is None, "a prefix image batch is image_util.PerSizeOracleEngine's"
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices)
        scen = capi.scenarios_array(scen)
        if segments is not None:
            mask = np.stack([MU.present_mask(prob.n_nodes, segments[0], np.asarray(segments[1])[s]) for s in range(len(scen))])
            zone = None
            if node_ranks is None:                           # (a segmented batch's own order: pool order over its nodes)
                node_ranks = np.where(mask, np.cumsum(mask, axis=1) - 1, -1).astype(np.int32)
        else:
            mask, zone = present
        mask = np.asarray(mask, bool)
        self.batches = getattr(self, "batches", 0) + 1
        res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
        for s in range(len(scen)):
            ps = fold_images_own(prob, mask[s]) if prob.image_locality is not None else prob
            one = super().run(ps, scen[s:s + 1], orders, want_placement, None if node_ranks is None else node_ranks[s:s + 1], want_gpu_slices,
                              (mask[s:s + 1], zone), evict)
            res.placement[s], res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = one.placement[0], one.unscheduled[0], one.used_cpu[0], one.used_mem[0]
            if want_gpu_slices and one.gpu_slices is not None:
                res.gpu_slices[s] = one.gpu_slices[0]
            if res.used_vg is not None and one.used_vg is not None:
                res.used_vg[s] = one.used_vg[0]
            if one.preempt_risk is not None:
                if res.preempt_risk is None:
                    res.preempt_risk = np.zeros(len(scen), np.uint8)
                res.preempt_risk[s] = one.preempt_risk[0]
        self.last_stats = None
        return res


# ---- the table case of test_gpu_image_own.py: sizes that land on the formula's edges ----------------------------------------------------
def _size_landing(target, c, n):
    """An integer sizeBytes X with int(float(X) * (float(c) / float(n))) == target (the map is monotone with steps of at most 1)."""
    x = max(int(target * n // c) - 4, 0)
    while int(float(x) * (float(c) / float(n))) < target:
        x += 1
    assert int(float(x) * (float(c) / float(n))) == target
    return x


def table_case(seed=5):
    """(im, Cp, masks, landmarks): 150 nodes (five presence words with tail bits), nine images, twelve pod classes -- one container on each
    image, two containers, five containers, and one class that runs nothing listed.  Image 0 is listed by 100 nodes (two chunk boundaries
    of its lister list) and its first lister lists size 0; image 1 by exactly 64 nodes; image 2 by the last node alone, with 2^53 - 1.
    Images 3 .. 7 are listed by nodes A = 2k, B = 2k + 1, D = 80 + k and a few later ones: with the whole pool D reads Size from A at
    count 3 of 150, without A from B at count 2 of 149, and those two sizes are chosen so that size x count / n lands on 23 MB, on the
    step to score 37 of a one-container class and on the upper clamp, each exactly and one byte either side (but for clamp + 1: ten
    places, two per image).  masks: the whole pool, each of the first 70 nodes removed, twelve random subsets of 40 .. 149 nodes, one
    scenario of the last node alone.  landmarks: (scenario, class, node, score) the edge sizes must give."""
    rng = np.random.default_rng(seed)
    N, I = 150, 9
    lists = [np.zeros(N, bool) for _ in range(I)]
    sizes = [rng.integers(5, 2500, N) * MB for _ in range(I)]
    lists[0][rng.choice(np.arange(1, N), 99, replace=False)] = True
    lists[0][0] = True
    sizes[0][0] = 0
    lists[1][rng.choice(N, 64, replace=False)] = True
    lists[2][N - 1] = True
    sizes[2][N - 1] = (1 << 53) - 1
    lists[8][rng.choice(N, 30, replace=False)] = True
    step = 23 * MB + -(-37 * 977 * MB // 100)                # the least sum that scores 37 with one container
    edges = [(23 * MB, 0), (23 * MB - 1, 0), (23 * MB + 1, 0), (step, 37), (step - 1, 36), (step + 1, 37),
             (1000 * MB, 100), (1000 * MB - 1, 99), (1000 * MB + 1, 100), (1000 * MB + 2, 100)]
    landmarks = []
    for k in range(3, 8):
        A, B, D = 2 * k, 2 * k + 1, 80 + k
        lists[k][[A, B, D]] = True
        lists[k][rng.choice(np.arange(100, N), 6, replace=False)] = True
        (ta, sa), (tb, sb) = edges[2 * (k - 3)], edges[2 * (k - 3) + 1]
        sizes[k][A] = _size_landing(ta, 3, N)
        sizes[k][B] = _size_landing(tb, 2, N - 1)
        landmarks += [(0, k, D, sa), (1 + A, k, D, sb)]      # (scenario 1 + j = the pool without node j; class k = one container on image k)
    classes = [[i] for i in range(I)] + [[3, 8], [0, 1, 4, -1, 6], [-1, -1]]
    im = pool_order_image(rng, N, lists, classes, sizes)
    masks = [np.ones(N, bool)]
    for j in range(70):
        m = np.ones(N, bool)
        m[j] = False
        masks.append(m)
    for _ in range(12):
        m = np.zeros(N, bool)
        m[rng.choice(N, int(rng.integers(40, 150)), replace=False)] = True
        masks.append(m)
    last = np.zeros(N, bool)
    last[N - 1] = True
    masks.append(last)
    masks = np.stack(masks)
    for s, c, j, want in landmarks:                          # the design holds, by the definition alone
        assert own_image_scores(im, masks[s])[c, j] == want, (s, c, j, want)
    return im, len(classes), masks, landmarks


# ---- k8s-level cases: a random cluster whose nodes list three images with per-node sizes -----------------------------------------------
def three_images(cluster, apps):
    """image_util.image_sweep_case's cluster with the fourth image folded onto the first: three images, per-node sizes as they are."""
    for n in cluster.get("Node", []):
        imgs = (n.get("status") or {}).get("images")
        if imgs:
            n["status"]["images"] = [i for i in imgs if not any(x.startswith("redis") for x in i.get("names") or [])]
    for a in apps:
        for objs in a.resource.values():
            for w in objs:
                spec = w["spec"]["template"]["spec"] if "template" in w.get("spec", {}) else w["spec"]
                for c in spec.get("containers") or []:
                    if c.get("image") == "redis":
                        c["image"] = "busybox"
    return cluster, apps


def table_friendly(apps, ports=True):
    """The apps without what sends a problem to the all-feature kernel, where own-nodes batches run only on request: pod (anti-)affinity
    and DoNotSchedule spread constraints go (ports=False: host ports too); node affinity, selectors, tolerations, ScheduleAnyway spread
    constraints and the Services' default spread stay."""
    for a in apps:
        for objs in a.resource.values():
            for w in objs:
                spec = w["spec"]["template"]["spec"] if "template" in w.get("spec", {}) else w["spec"]
                aff = spec.get("affinity") or {}
                aff.pop("podAffinity", None)
                aff.pop("podAntiAffinity", None)
                if not aff:
                    spec.pop("affinity", None)
                tsc = [c for c in spec.get("topologySpreadConstraints") or [] if c.get("whenUnsatisfiable") != "DoNotSchedule"]
                if tsc:
                    spec["topologySpreadConstraints"] = tsc
                else:
                    spec.pop("topologySpreadConstraints", None)
                if not ports:
                    for c in spec.get("containers") or []:
                        c.pop("ports", None)
    return apps


def failure_case(seed, zones=False, gpu=False, n_nodes=24, n_workloads=34, n_random=8, ports=True):
    """(flat, masks, zone, scen, orders, ranks) of a node-subset image batch: 24 nodes, about 60 % of them listing three images, about 120
    pods; the whole cluster, every single node removed and eight random subsets, each in the nodeTree order of its own nodes."""
    import subset_util as SU
    from open_simulator_amd import flatten as fl, k8s, simulate as sim
    cluster, apps, _ = IU.image_sweep_case(seed, n_nodes=n_nodes, n_workloads=n_workloads, zones=zones, gpu=gpu, listing_share=0.6)
    three_images(cluster, apps)
    table_friendly(apps, ports)
    pool = list(cluster["Node"])
    pods, gates = sim.build_stream(cluster, apps, pool, 0)
    flat = fl.flatten(pool, pods, cluster.get("Service", []), cluster.get("ReplicaSet", []), cluster.get("StatefulSet", []), gates, image_batch="own")
    N = len(pool)
    rng = np.random.default_rng(seed + 77)
    masks = [np.ones(N, bool)] + [np.arange(N) != j for j in range(N)]
    for _ in range(n_random):
        m = rng.random(N) < rng.uniform(0.3, 0.9)
        m[int(rng.integers(N))] = True
        masks.append(m)
    masks = np.stack(masks)
    zid = {}
    zone = np.array([zid.setdefault(k8s.zone_key(n), len(zid)) for n in pool], np.int32)
    zone = zone if len(zid) > 1 else None
    scen = np.stack([masks.sum(1), np.zeros(len(masks), np.int64)], 1).astype(np.int32)
    orders = np.arange(len(pods), dtype=np.int32)[None, :]
    ranks = SU.zone_ranks(masks, zone)
    return flat, masks, zone, scen, orders, ranks

"""GPU-share device usage and the device bound of headroom, the host side (no GPU): hand cases of the closed form; the definition
against the unmodified oracle -- fit + 3 copies of a GPU probe appended to the stream, exactly fit of them placed; the device sums
against the oracle's own slices; the header text and the ctypes prototypes; the sweeps' devices=True on oracle-backed engines with
and without supports_gpu_usage, and devices=False against what the sweeps returned before the switch existed."""
import ctypes as C
import functools
import os
import re
import warnings

import numpy as np
import pytest

import gpu_usage_util as GU
import mix_util as MU
import oracle_lib as O
import randprob
import usage_util as UU
from open_simulator_amd import capi, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30
# (seed, N, P): pools of 5 to 40 nodes, streams that leave room (every probe's fit + 3 copies run through the oracle again)
CASES = [(1, 5, 30), (2, 9, 54), (3, 20, 120), (4, 40, 120), (5, 9, 40), (6, 20, 100)]


def test_cap_gpu_hand_cases():
    # tightest fit, one device per pod: 16 GiB devices with 10, 4 and 0 GiB booked hold 1 + 3 + 4 pods of 4 GiB
    assert GU.cap_gpu(16 * GiB, 3, [10 * GiB, 4 * GiB, 0, 0, 0, 0, 0, 0], 4 * GiB, 1) == 8
    # a remainder below one slice on every device is lost: 3 x 3 GiB idle hold no 4 GiB pod
    assert GU.cap_gpu(16 * GiB, 3, [13 * GiB] * 3 + [0] * 5, 4 * GiB, 1) == 0
    # c = 2 and c = 3 take several slices from one device: one idle 16 GiB device holds 4 slices = 2 pods of two, 1 pod of three
    assert GU.cap_gpu(16 * GiB, 2, [16 * GiB, 0, 0, 0, 0, 0, 0, 0], 4 * GiB, 2) == 2
    assert GU.cap_gpu(16 * GiB, 2, [16 * GiB, 0, 0, 0, 0, 0, 0, 0], 4 * GiB, 3) == 1
    assert GU.cap_gpu(16 * GiB, 2, [12 * GiB, 8 * GiB, 0, 0, 0, 0, 0, 0], 4 * GiB, 3) == 1        # 1 + 2 slices across two devices
    assert GU.cap_gpu(16 * GiB, 2, [12 * GiB, 12 * GiB, 0, 0, 0, 0, 0, 0], 4 * GiB, 3) == 0
    # an over-booked device clamps to 0 instead of eating the others' room
    assert GU.cap_gpu(16 * GiB, 2, [40 * GiB, 8 * GiB, 0, 0, 0, 0, 0, 0], 4 * GiB, 1) == 2
    # a node of more than 8 devices: the per-device total divides by the unclamped count, 8 devices are walked
    prob = randprob.rand_problem(1, N=2, P=4, gpu=True)
    prob.gpu_cnt = np.array([16, 0], np.int32)
    prob.gpu_mem_total = np.array([16 * 8 * GiB, 0], np.int64)
    assert GU.node_devices(prob, 0) == (8, 8 * GiB) and GU.node_devices(prob, 1) == (0, 0)
    assert GU.cap_gpu(8 * GiB, 8, [0] * 8, 4 * GiB, 1) == 16
    # a pod with gpu_cnt = 0 (gpu_allocate returns 0), a node without devices, a count above 64
    assert GU.cap_gpu(16 * GiB, 2, [0] * 8, 4 * GiB, 0) == 0
    assert GU.cap_gpu(0, 0, [0] * 8, 4 * GiB, 1) == 0
    assert GU.cap_gpu(1 << 40, 8, [0] * 8, 1 << 30, 100) == 8 * 1024 // 64


@functools.lru_cache(maxsize=None)
def _case(seed, N, P):
    """(problem, order, oracle result with its slices, held rows) of one full-size scenario."""
    prob = randprob.rand_problem(seed, N=N, P=P, gpu=True, static_mask=True, init_state=True, gates=True)
    order = np.random.default_rng(seed).permutation(prob.n_pods).astype(np.int32)
    res = O.run(prob, [[N, 0]], order[None], want_gpu_slices=True)
    return prob, order, res, UU.held_rows(prob, [[N, 0]])


def _gpu_probes(prob):
    """One exact GPU probe per distinct (class, memory, count)."""
    seen, out = set(), []
    for p in range(prob.n_pods):
        key = (int(prob.pod_class[p]), int(prob.gpu_mem[p]), int(prob.pod_gpu_cnt[p]))
        if prob.gpu_mem[p] > 0 and key not in seen and GU.probe_exact_gpu(prob, p):
            seen.add(key)
            out.append(p)
    return out


@pytest.mark.parametrize("seed,N,P", CASES)
def test_device_bounded_headroom_is_what_the_oracle_places_of_appended_probes(seed, N, P):
    prob, order, res, held = _case(seed, N, P)
    probes = _gpu_probes(prob)
    assert len(probes) >= 6
    fit, nodes, exact, res_cap, gpu_cap = GU.headroom_gpu(prob, res.placement, res.gpu_slices, held, probes, parts=True)
    old, _, old_exact = UU.headroom(prob, res.placement, held, probes)
    assert exact.all() and not old_exact.any()                                  # simon_fetch_headroom keeps exact = 0 for them
    assert (fit <= old).all()
    # every seed has a probe whose device bound is strictly below the resource bound, and (probe, node) pairs of both kinds: the
    # devices the tighter bound, and the resources (test_both_kinds_of_probe_occur_over_the_cases: probes of both kinds)
    assert (fit[0] < old[0]).any(), "no probe whose device bound is below the resource bound"
    counted = res_cap[0] >= 0
    tighter = counted & (gpu_cap[0] < res_cap[0])
    loose = counted & (gpu_cap[0] >= res_cap[0]) & (res_cap[0] > 0)
    assert tighter.any() and loose.any(), (int(tighter.sum()), int(loose.sum()))
    for k, p in enumerate(probes):
        UU.check_probe_against_oracle(prob, N, order, res.placement[0], p, fit[0, k])
        assert (fit[0, k] > 0) == (nodes[0, k] > 0)
    zero_cnt = [k for k, p in enumerate(probes) if prob.pod_gpu_cnt[p] == 0]
    assert all(fit[0, k] == 0 for k in zero_cnt)


def test_a_node_of_more_than_eight_devices_against_the_oracle():
    """gpu_cnt = 16: AllocateGpuId walks the first eight devices, each of gpu_mem_total / 16 bytes (the library refuses such a node at
    simon_load_nodes; the definition and the host road still follow the oracle)."""
    import evict_util as EU
    base, order, _, held = _case(3, 20, 120)
    wide = np.asarray(base.gpu_cnt) == 8
    assert wide.any()
    prob = EU.replaced(base, gpu_cnt=np.where(wide, 16, base.gpu_cnt).astype(np.int32),
                       gpu_mem_total=np.where(wide, 2 * np.asarray(base.gpu_mem_total), base.gpu_mem_total).astype(np.int64))
    j = int(np.flatnonzero(wide)[0])
    assert GU.node_devices(prob, j) == (8, int(base.gpu_mem_total[j]) // 8)
    res = O.run(prob, [[20, 0]], order[None], want_gpu_slices=True)
    probes = _gpu_probes(prob)[:12]
    fit, _, exact = GU.headroom_gpu(prob, res.placement, res.gpu_slices, held, probes)
    hf, _, _ = sim.host_headroom(prob, res.placement, held, probes, res.gpu_slices, devices=True)
    assert exact.all() and (fit > 0).any() and hf.tolist() == fit.tolist()
    for k, p in enumerate(probes):
        UU.check_probe_against_oracle(prob, 20, order, res.placement[0], p, fit[0, k])


def test_both_kinds_of_probe_occur_over_the_cases():
    strictly, equal = 0, 0
    for seed, N, P in CASES:
        prob, order, res, held = _case(seed, N, P)
        probes = _gpu_probes(prob)
        fit, _, _ = GU.headroom_gpu(prob, res.placement, res.gpu_slices, held, probes)
        old, _, _ = UU.headroom(prob, res.placement, held, probes)
        strictly += int((fit[0] < old[0]).sum())
        equal += int(((fit[0] == old[0]) & (old[0] > 0)).sum())
    assert strictly > 0 and equal > 0, (strictly, equal)


@pytest.mark.parametrize("seed,N,P", CASES)
def test_device_sums_of_the_oracle_s_slices(seed, N, P):
    prob, order, _, _ = _case(seed, N, P)
    scen = np.array([[N, 0], [max(1, N // 2), 0], [max(1, N - 1), 0]], np.int32)
    res = O.run(prob, scen, order[None], want_gpu_slices=True)
    held = UU.held_rows(prob, scen)
    g = GU.dev_usage(prob, res.placement, res.gpu_slices, held)
    init = np.asarray(prob.init_gpu_used).reshape(N, GU.D)
    for s in range(len(scen)):
        for j in range(N):
            on = np.flatnonzero(res.placement[s] == j)
            n_slices = sum(sum((int(res.gpu_slices[s][p]) >> (8 * d)) & 255 for d in range(GU.D)) for p in on)
            booked = sum(sum((int(res.gpu_slices[s][p]) >> (8 * d)) & 255 for d in range(GU.D)) * int(prob.gpu_mem[p]) for p in on)
            cnt, per = GU.node_devices(prob, j)
            if not held[s, j]:
                assert (g.dev_used[s, j] == 0).all() and (g.dev_pods[s, j] == -1).all() and n_slices == 0
                continue
            assert int(g.dev_used[s, j].sum()) == booked + int(init[j, :cnt].sum()), (s, j)
            assert (g.dev_used[s, j, cnt:] == 0).all() and (g.dev_pods[s, j, cnt:] == 0).all()
            assert (g.dev_used[s, j, :cnt] <= per).all()                       # Reserve never over-books a device of this stream
    assert g.dev_pods.max() > 0
    # the host road of the sweeps is the same definition, vectorised
    h = sim.host_gpu_usage(prob, res.placement, res.gpu_slices, held)
    assert (h.dev_used == g.dev_used).all() and (h.dev_pods == g.dev_pods).all()
    sub = sim.host_gpu_usage(prob, res.placement, res.gpu_slices, held, [2, 0, 2])
    assert (sub.dev_used == g.dev_used[[2, 0, 2]]).all() and (sub.dev_pods == g.dev_pods[[2, 0, 2]]).all()
    probes = _gpu_probes(prob) + [p for p in range(prob.n_pods) if prob.gpu_mem[p] == 0][:3]
    fit, nodes, exact = GU.headroom_gpu(prob, res.placement, res.gpu_slices, held, probes)
    hf, hn, hx = sim.host_headroom(prob, res.placement, held, probes, res.gpu_slices, devices=True)
    assert (hf == fit).all() and (hn == nodes).all() and hx.tolist() == exact.tolist()
    # without the switch the host road is simon_fetch_headroom's: the resource bound, exact = 0 for GPU probes
    of, on_, ox = sim.host_headroom(prob, res.placement, held, probes)
    rf, rn, rx = UU.headroom(prob, res.placement, held, probes)
    assert (of == rf).all() and (on_ == rn).all() and ox.tolist() == rx.tolist()
    k0 = len(probes) - 3
    assert (fit[:, k0:] == rf[:, k0:]).all() and exact[k0:].tolist() == rx[k0:].tolist()    # no GPU request: bit for bit the old call


def test_a_probe_with_a_gpu_index_gets_no_device_bound_and_is_not_exact():
    prob, order, res, held = _case(1, 5, 30)
    p = _gpu_probes(prob)[0]
    idx = np.zeros(prob.n_pods, np.uint32)
    idx[p] = capi.pack_gpu_index([0])
    import evict_util as EU
    marked = EU.replaced(prob, gpu_index=idx)
    fit, _, exact = GU.headroom_gpu(marked, res.placement, res.gpu_slices, held, [p])
    old, _, _ = UU.headroom(marked, res.placement, held, [p])
    assert fit.tolist() == old.tolist() and not exact[0]
    hf, _, hx = sim.host_headroom(marked, res.placement, held, [p], res.gpu_slices, devices=True)
    assert hf.tolist() == old.tolist() and not hx[0]


def test_the_refusal_rules_restated():
    assert GU.gpu_usage_errors(6, None, 6) == [] and GU.gpu_usage_errors(6, [5, 0, 5], 3) == []
    assert GU.gpu_usage_errors(6, None, 0) == ["n"] and GU.gpu_usage_errors(6, None, 7) == ["scenario id"]
    assert GU.gpu_usage_errors(6, None, 6, have_dev_used=False) == ["missing array"]
    assert GU.gpu_usage_errors(6, None, 6, struct_ok=False) == ["struct_size"]
    assert GU.gpu_usage_errors(6, None, 6, have_placement=False) == ["no placements"] == GU.gpu_usage_errors(6, None, 6, reloaded=True)
    assert GU.gpu_usage_errors(6, None, 6, gpu=True, have_slices=False) == ["no devices recorded"]
    assert GU.gpu_usage_errors(6, None, 6, gpu=False, have_slices=False) == []             # no GPU request anywhere: answered
    assert GU.headroom_gpu_errors(10, [0, 9], 2) == [] and GU.headroom_gpu_errors(10, [0], 0) == ["K"]
    assert GU.headroom_gpu_errors(10, [10], 1) == ["pod id"] and GU.headroom_gpu_errors(10, [0], 1, have_fit=False) == ["missing array"]
    assert GU.headroom_gpu_errors(10, [0], 1, gpu=True, have_slices=False) == ["no devices recorded"]
    assert GU.headroom_gpu_errors(10, [0], 1, have_placement=False, gpu=True, have_slices=False) == ["no placements"]
    prob = _case(1, 5, 30)[0]
    assert GU.has_gpu(prob) and not GU.has_gpu(randprob.rand_problem(1, N=5, P=20))


def test_header_declares_and_capi_exports_both_calls():
    text = open(os.path.join(ROOT, "include", "simon_hip.h")).read()
    hdr = re.sub(r"[ \n]+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int simon_fetch_gpu_usage(simon_ctx* ctx, const int32_t* scen_ids , int32_t n, simon_gpu_usage* out);" in hdr
    assert ("int simon_fetch_headroom_gpu(simon_ctx* ctx, const int32_t* probe_pod , int32_t K, int64_t* fit , int32_t* fit_nodes , "
            "uint8_t* exact );") in hdr
    assert "typedef struct simon_gpu_usage { uint32_t struct_size; int64_t* dev_used; int32_t* dev_pods; } simon_gpu_usage;" in hdr
    assert "#define SIMON_HIP_ABI_VERSION 7 " in text and capi.ABI_VERSION == 7
    assert "SIMON_WANT_GPU_SLICES" in text and "Not covered: GPU-share device usage" not in text
    assert {"simon_fetch_gpu_usage", "simon_fetch_headroom_gpu"} <= set(capi.EXPORTS)
    assert "simon_group_fetch_gpu_usage" not in text and "simon_group_fetch_headroom_gpu" not in text
    lib = capi.load_library()
    assert lib.simon_fetch_gpu_usage.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(capi.GpuUsageC)]
    assert lib.simon_fetch_headroom_gpu.argtypes == lib.simon_fetch_headroom.argtypes
    assert lib.simon_fetch_gpu_usage.restype is C.c_int and lib.simon_fetch_headroom_gpu.restype is C.c_int
    assert C.sizeof(capi.GpuUsageC) == 24 and capi.GpuUsageC.dev_pods.offset == 16
    assert sim.HipEngine.supports_gpu_usage is True and sim.HipEngine.supports_node_usage is True


# ---- the sweeps ----------------------------------------------------------------------------------------------------------------------

def _gpu_refs(cluster, apps, n=2):
    """(namespace, name) of the first pods of n distinct workloads that request GPU memory, and of one that does not."""
    pods, _ = sim.build_stream(cluster, apps, list(cluster["Node"]), len(cluster["Node"]))
    from open_simulator_amd import flatten as fl
    gpu_mem = lambda p: fl._gpu_annotations(p)[0]                                                       # noqa: E731
    gpu, plain, seen = [], [], set()
    for p in pods:
        owner = (p["metadata"].get("ownerReferences") or [{}])[0].get("name") or p["metadata"]["name"]
        if owner in seen or (p.get("spec") or {}).get("nodeName") or "_daemon_node" in p:
            continue
        seen.add(owner)
        (gpu if gpu_mem(p) > 0 else plain).append((p["metadata"]["namespace"], p["metadata"]["name"]))
    return gpu[:n] + plain[:1]


@functools.lru_cache(maxsize=None)
def _gpushare():
    cluster, apps, types = MU.example_gpushare()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    return cluster, apps, types, _gpu_refs(cluster, apps)


FIELDS = ("headroom", "headroom_exact", "node_table", "gpu_table")


def _same(a, b):
    for f in FIELDS:
        assert getattr(a, f) == getattr(b, f), f


def test_sweep_with_devices_on_engines_with_and_without_the_calls():
    cluster, apps, types, refs = _gpushare()
    assert len(refs) >= 2
    counts = [0, 1, 2]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                             # the device road warns nowhere
        a = sim.sweep(cluster, apps, types[0], counts, engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
    with pytest.warns(sim.UsageFallbackWarning, match="supports_gpu_usage"):
        b = sim.sweep(cluster, apps, types[0], counts, engine=GU.NodeUsageOnlyEngine(), headroom=refs, node_table=True, devices=True)
    with pytest.warns(sim.UsageFallbackWarning, match="supports_node_usage"):
        c = sim.sweep(cluster, apps, types[0], counts, engine=UU.PlainOracleEngine(), headroom=refs, node_table=True, devices=True)
    _same(a, b)
    _same(a, c)
    assert a.headroom_exact[0] and len(a.gpu_table) == len(counts) == len(a.node_table)
    # the devices are the bottleneck for the GPU probe somewhere: below the resource bound of the old call
    old = sim.sweep(cluster, apps, types[0], counts, engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
    assert all(x <= y for ra, ro in zip(a.headroom, old.headroom) for x, y in zip(ra, ro))
    assert any(x < y for ra, ro in zip(a.headroom, old.headroom) for x, y in zip(ra[:-1], ro[:-1])) and not old.headroom_exact[0]
    assert [ra[-1] for ra in a.headroom] == [ro[-1] for ro in old.headroom]          # the probe without a GPU request: unchanged
    # the table: one row per GPU node the size holds, arithmetic of the "GPU Node Resource" table
    for s, k in enumerate(counts):
        names = [r["node"] for r in a.node_table[s] if r["gpu_mem_allocatable"] > 0]
        assert [r["node"] for r in a.gpu_table[s]] == names and len(a.node_table[s]) == len(cluster["Node"]) + k
        for row, full in zip(a.gpu_table[s], [r for r in a.node_table[s] if r["gpu_mem_allocatable"] > 0]):
            assert sum(d["used"] for d in row["devices"]) == full["gpu_mem_requests"]
            assert sum(d["total"] for d in row["devices"]) <= full["gpu_mem_allocatable"] and row["model"]
            assert all(d["used"] <= d["total"] and d["pods"] >= 0 for d in row["devices"])
    assert any(d["pods"] > 0 for rows in a.gpu_table for r in rows for d in r["devices"])


def test_gpu_table_is_simulate_s_node_annotation():
    """The per-device figures against simulate()'s own result of one size: the simon/node-gpu-share annotation _gpu_node_status writes."""
    import json
    from open_simulator_amd import k8s, workloads as wl
    cluster, apps, types, refs = _gpushare()
    sw = sim.sweep(cluster, apps, types[0], [1], engine=GU.GpuUsageOracleEngine(), devices=True)
    assert sw.headroom is None and sw.node_table is None
    res = sim.simulate(cluster, apps, engine=MU.OracleEngine(), new_nodes=wl.new_fake_nodes(types[0], 1))
    want = {}
    for st in res.node_status:
        anno = (st["node"]["metadata"].get("annotations") or {}).get(k8s.ANNO_NODE_GPU_SHARE)
        if anno:
            info = json.loads(anno)
            want[st["node"]["metadata"]["name"]] = [(v["GpuUsedMemory"], len(v["PodList"] or [])) for _, v in sorted(info["DevsBrief"].items(), key=lambda kv: int(kv[0]))]
    got = {r["node"]: [(sim._mi(d["used"]), d["pods"]) for d in r["devices"]] for r in sw.gpu_table[0]}
    assert want and all(got[n] == want[n] for n in want)
    assert all(all(u == "0" and k == 0 for u, k in v) for n, v in got.items() if n not in want)


def test_the_other_sweeps_with_devices():
    cluster, apps, types, refs = _gpushare()
    fa = sim.sweep_failures(cluster, apps, "node", engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
    with pytest.warns(sim.FailureFallbackWarning, match="supports_gpu_usage"):
        fb = sim.sweep_failures(cluster, apps, "node", engine=GU.NodeUsageOnlyEngine(), headroom=refs, node_table=True, devices=True)
    with pytest.warns(sim.FailureFallbackWarning, match="one by one"):
        fc = sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine(), headroom=refs, node_table=True, devices=True)
    assert fa.batched and fb.batched and not fc.batched
    _same(fa, fb)
    _same(fa, fc)
    assert len(fa.gpu_table) == len(fa.domains) + 1 and fa.headroom_exact[0]
    with pytest.warns(sim.MixFallbackWarning):
        ma = sim.sweep_mix(cluster, apps, types, [[0, 1], [0, 1]], engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
    assert len(ma.gpu_table) == 4 == len(ma.headroom) and ma.headroom_exact[0]
    for s, mix in enumerate(ma.counts):
        one = sim.sweep(dict(cluster, Node=list(cluster["Node"]) + [n for nn in sim.mix_fake_nodes(types, mix) for n in nn]), apps, None, [0],
                        engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
        assert ma.headroom[s] == one.headroom[0] and ma.gpu_table[s] == one.gpu_table[0], mix
    split = [sim.AppResource(f"{k.lower()}-{o['metadata']['name']}", {k: [o]}) for a in apps for k, v in a.resource.items()
             if k in ("Pod", "ReplicaSet") for o in v]
    prefs = _gpu_refs(cluster, split)
    pa = sim.sweep_apps(cluster, split, new_node=types[0], counts=[0, 1], engine=GU.GpuUsageOracleEngine(), headroom=prefs, node_table=True, devices=True)
    with pytest.warns(sim.AppFallbackWarning, match="supports_gpu_usage"):
        pb = sim.sweep_apps(cluster, split, new_node=types[0], counts=[0, 1], engine=GU.NodeUsageOnlyEngine(), headroom=prefs, node_table=True, devices=True)
    assert pa.batched and pb.batched
    _same(pa, pb)
    assert np.asarray(pa.headroom).shape == (len(pa.subsets), 2, len(prefs)) and len(pa.gpu_table[0]) == 2
    # ... and every scenario as its own problem (an engine without pod subsets): the whole set of apps, where the streams are the same
    whole = [[a.name for a in split]]
    pc = sim.sweep_apps(cluster, split, subsets=whole, new_node=types[0], counts=[0, 1], engine=GU.GpuUsageOracleEngine(), headroom=prefs, node_table=True, devices=True)
    with pytest.warns(sim.AppFallbackWarning, match="one by one"):
        pd = sim.sweep_apps(cluster, split, subsets=whole, new_node=types[0], counts=[0, 1], engine=MU.OracleEngine(), headroom=prefs, node_table=True, devices=True)
    assert pc.batched and not pd.batched
    _same(pc, pd)


def test_without_devices_the_sweeps_return_what_they_returned():
    cluster, apps, types, refs = _gpushare()
    keys = ["node", "cpu_allocatable", "cpu_requests", "memory_allocatable", "memory_requests", "pods", "new"]
    for eng in (UU.UsageOracleEngine, GU.GpuUsageOracleEngine, UU.PlainOracleEngine):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = sim.sweep(cluster, apps, types[0], [0, 2], engine=eng(), headroom=refs, node_table=True)
            b = sim.sweep(cluster, apps, types[0], [0, 2], engine=eng(), headroom=refs, node_table=True, devices=False)
            plain = sim.sweep(cluster, apps, types[0], [0, 2], engine=eng())
        assert a.gpu_table is None and b.gpu_table is None and plain.gpu_table is None and plain.headroom is None
        _same(a, b)
        assert all(list(r) == keys for rows in a.node_table for r in rows)
        assert not a.headroom_exact[0]                                             # the GPU probe: the resource bound, not exact
    fa = sim.sweep_failures(cluster, apps, "node", engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
    assert fa.gpu_table is None and all(list(r) == keys for rows in fa.node_table for r in rows)

"""Shared pieces of the GPU-share usage / headroom tests (test_gpu_share_usage_host.py, test_gpu_share_usage.py): both definitions of
include/simon_hip.h (simon_fetch_gpu_usage, simon_fetch_headroom_gpu) restated in plain loops over a placement matrix, the recorded
devices and a capi.Problem, the refusal rules restated, and oracle-backed engines with and without supports_gpu_usage."""
import dataclasses

import numpy as np

import usage_util as UU
from open_simulator_amd import capi

D = capi.MAX_GPU_DEV


def _at(v, i, d=0):
    return d if v is None else int(np.asarray(v)[i])


def node_devices(prob, j):
    """(cnt, per) of pool node j: the devices the kernels see, min(gpu_cnt, 8), and the bytes of each, gpu_mem_total / gpu_cnt by the
    UNCLAMPED count (gpu_allocate's dev_total)."""
    raw = _at(prob.gpu_cnt, j)
    return (min(raw, D), _at(prob.gpu_mem_total, j) // raw) if raw > 0 else (0, 0)


@dataclasses.dataclass
class DevUsage:
    dev_used: np.ndarray       # [S][N][8] int64
    dev_pods: np.ndarray       # [S][N][8] int32, -1 = absent node


def dev_usage(prob, placement, slices, held):
    """simon_fetch_gpu_usage restated: pod by pod, slice byte by slice byte, onto the devices of the node its placement names, on top
    of init_gpu_used; 0 / -1 on a node the scenario lacks, 0 / 0 on a device the node lacks."""
    placement, held = np.asarray(placement), np.asarray(held, bool)
    S, N = held.shape
    used, pods = np.zeros((S, N, D), np.int64), np.zeros((S, N, D), np.int32)
    for s in range(S):
        for p, j in enumerate(placement[s].tolist()):
            if j < 0 or slices is None or _at(prob.gpu_mem, p) <= 0:
                continue
            assert held[s, j], (s, p, j)
            w = int(slices[s][p])
            for d in range(D):
                b = (w >> (8 * d)) & 255
                if b:
                    used[s, j, d] += b * _at(prob.gpu_mem, p)
                    pods[s, j, d] += 1
        for j in range(N):
            cnt, _ = node_devices(prob, j)
            for d in range(D):
                if not held[s, j]:
                    used[s, j, d], pods[s, j, d] = 0, -1
                elif d >= cnt:
                    assert pods[s, j, d] == 0, "a slice on a device the node lacks"
                    used[s, j, d] = 0
                elif prob.init_gpu_used is not None:
                    used[s, j, d] += int(np.asarray(prob.init_gpu_used).reshape(N, D)[j, d])
    return DevUsage(used, pods)


def cap_gpu(per, cnt, used, m, c):
    """How many further pods of m bytes per slice on c devices GpuNodeInfo.AllocateGpuId + Reserve accept on a node of cnt devices of
    per bytes each with used[d] booked: T = sum max(per - used[d], 0) // m slices are left, every pod takes min(c, 64) of them."""
    if m <= 0 or c <= 0 or cnt <= 0:
        return 0
    T = sum(max(int(per) - int(used[d]), 0) // int(m) for d in range(min(cnt, D)))
    return T // min(c, 64)


def probe_bound(prob, p):
    """The device bound applies to probe p: a GPU request that arrives without a gpu-index annotation."""
    return _at(prob.gpu_mem, p) > 0 and _at(prob.gpu_index, p) == 0


def probe_exact_gpu(prob, p):
    """simon_fetch_headroom_gpu's exact: simon_fetch_headroom's conditions, a bounded GPU request no longer disqualifying."""
    if not probe_bound(prob, p):
        return UU.probe_exact(prob, p)
    cls = int(prob.pod_class[p]) if prob.pod_class is not None else 0
    if _at(prob.pin_node, p, -1) >= 0 or _at(prob.preset_node, p, -1) >= 0:
        return False
    if prob.term_topo_key is not None and len(prob.term_topo_key):
        for off in (prob.match_off, prob.anti_off, prob.port_off, prob.aff_off, prob.spread_hard_off):
            if off is not None and off[cls + 1] != off[cls]:
                return False
    return prob.local_spec_of is None or int(prob.local_spec_of[cls]) < 0


def headroom_gpu(prob, placement, slices, held, probes, parts=False):
    """simon_fetch_headroom_gpu restated: (fit [S][K] int64, fit_nodes [S][K] int32, exact [K] bool); parts=True: also the two bounds
    per (scenario, probe, node) as int64 [S][K][N] arrays (resources, devices; -1 = the node is not counted / no device bound)."""
    held = np.asarray(held, bool)
    S, N = held.shape
    K = UU._n_scalar(prob)
    u = UU.node_usage(prob, placement, held)
    g = dev_usage(prob, placement, slices, held)
    alloc = np.stack([UU._vec(prob.alloc_cpu, N), UU._vec(prob.alloc_mem, N), UU._vec(prob.alloc_eph, N)] + [np.asarray(prob.scalar_alloc[k], np.int64) for k in range(K)])
    probes = np.asarray(probes).tolist()
    fit, nodes = np.zeros((S, len(probes)), np.int64), np.zeros((S, len(probes)), np.int32)
    res_cap, gpu_cap = np.full((S, len(probes), N), -1, np.int64), np.full((S, len(probes), N), -1, np.int64)
    for k, p in enumerate(probes):
        q, entries = UU.probe_request(prob, p)
        cls = int(prob.pod_class[p]) if prob.pod_class is not None else 0
        for s in range(S):
            for j in np.flatnonzero(held[s]).tolist():
                if not UU.static_ok(prob, cls, j):
                    continue
                used = [u.req_cpu[s, j], u.req_mem[s, j], u.req_eph[s, j]] + [u.scalar_req[s, i, j] for i in range(K)]
                c = res_cap[s, k, j] = UU.cap_of(prob.alloc_pods[j], u.npods[s, j], alloc[:, j], used, q, entries)
                if probe_bound(prob, p):
                    cnt, per = node_devices(prob, j)
                    gpu_cap[s, k, j] = cap_gpu(per, cnt, g.dev_used[s, j], _at(prob.gpu_mem, p), _at(prob.pod_gpu_cnt, p))
                    c = min(c, int(gpu_cap[s, k, j]))
                fit[s, k] += c
                nodes[s, k] += c > 0
    out = fit, nodes, np.array([probe_exact_gpu(prob, p) for p in probes], bool)
    return out + (res_cap, gpu_cap) if parts else out


def has_gpu(prob):
    """The library's has_gpu: the pool carries GPU arrays, or some pod requests GPU memory."""
    return prob.gpu_cnt is not None or (prob.gpu_mem is not None and bool((np.asarray(prob.gpu_mem) > 0).any()))


def gpu_usage_errors(S, scen_ids, n, have_dev_used=True, struct_ok=True, have_placement=True, reloaded=False, gpu=False, have_slices=True):
    """simon_fetch_gpu_usage's refusals, restated: the rules a call breaks ([] = accepted)."""
    bad = UU.usage_errors(S, scen_ids, n, have=("req_cpu", "req_mem", "npods") if have_dev_used else (), struct_ok=struct_ok,
                          have_placement=have_placement, reloaded=reloaded)
    if not bad and gpu and not have_slices:
        bad.append("no devices recorded")
    return bad


def headroom_gpu_errors(P, probes, K, have_fit=True, have_placement=True, reloaded=False, gpu=False, have_slices=True):
    """simon_fetch_headroom_gpu's refusals, restated."""
    bad = UU.headroom_errors(P, probes, K, have_fit, have_placement, reloaded)
    if not bad and gpu and not have_slices:
        bad.append("no devices recorded")
    return bad


class NodeUsageOnlyEngine(UU.UsageOracleEngine):
    """Oracle-backed engine with supports_node_usage alone: with devices=True the sweeps compute everything on the host and warn."""


class GpuUsageOracleEngine(UU.UsageOracleEngine):
    """Oracle-backed engine that answers gpu_usage_of / headroom_devices as HipEngine does, from the restatement above."""
    supports_gpu_usage = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, pod_present=None,
            pod_groups=None, headroom_pods=None, usage_of=None, gpu_usage_of=None, headroom_devices=False):
        record = want_gpu_slices or ((gpu_usage_of is not None or headroom_devices) and prob.gpu_mem is not None)
        res = super().run(prob, scen, orders, True, node_ranks, record, present, pod_present, pod_groups,
                          None if headroom_devices else headroom_pods, usage_of)
        held = UU.held_rows(prob, capi.scenarios_array(scen), None if present is None else present[0])
        if headroom_pods is not None and headroom_devices:
            res.headroom, _, res.headroom_exact = headroom_gpu(prob, res.placement, res.gpu_slices, held, headroom_pods)
        if gpu_usage_of is not None:
            ids = np.asarray(gpu_usage_of, np.int32)
            g = dev_usage(prob, res.placement[ids], None if res.gpu_slices is None else res.gpu_slices[ids], held[ids])
            res.gpu_usage = capi.GpuUsage(ids, g.dev_used, g.dev_pods)
        if not want_gpu_slices:
            res.gpu_slices = None
        return res

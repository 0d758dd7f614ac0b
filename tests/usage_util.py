"""Shared pieces of the node-usage / headroom tests (test_usage_host.py, test_gpu_usage.py): both definitions of include/simon_hip.h
(simon_fetch_node_usage, simon_fetch_headroom) restated in plain loops over a placement matrix and a capi.Problem, the refusal rules
restated, the appended-probes check against the unmodified oracle, and oracle-backed engines with and without supports_node_usage."""
import dataclasses

import numpy as np

import evict_util as EU
import oracle_lib as O
import podset_util as PU
from open_simulator_amd import capi


def held_rows(prob, scen, present=None):
    """bool [S][N]: the pool nodes every scenario holds -- its presence row, or the prefix of its n_nodes."""
    if present is not None:
        return np.asarray(present, bool)
    return np.arange(prob.n_nodes)[None, :] < np.asarray(scen)[:, :1]


def _vec(v, n):
    return np.zeros(n, np.int64) if v is None else np.asarray(v, np.int64)


def _n_scalar(prob):
    return 0 if prob.scalar_alloc is None else int(np.asarray(prob.scalar_alloc).shape[0])


@dataclasses.dataclass
class Usage:
    req_cpu: np.ndarray        # [S][N]
    req_mem: np.ndarray
    req_eph: np.ndarray
    scalar_req: np.ndarray     # [S][K][N]
    npods: np.ndarray          # [S][N], -1 = absent


def node_usage(prob, placement, held):
    """simon_fetch_node_usage restated: pod by pod onto the node its placement names, on top of the state before the stream."""
    placement, held = np.asarray(placement), np.asarray(held, bool)
    S, N = held.shape
    P, K = prob.n_pods, _n_scalar(prob)
    cpu, mem, eph = _vec(prob.req_cpu, P), _vec(prob.req_mem, P), _vec(prob.req_eph, P)
    sc = np.zeros((K, P), np.int64) if prob.scalar_req is None else np.asarray(prob.scalar_req, np.int64).reshape(K, P)
    isc = np.zeros((K, N), np.int64) if prob.init_scalar_req is None else np.asarray(prob.init_scalar_req, np.int64).reshape(K, N)
    u = Usage(np.zeros((S, N), np.int64), np.zeros((S, N), np.int64), np.zeros((S, N), np.int64), np.zeros((S, K, N), np.int64),
              np.full((S, N), -1, np.int32))
    for s in range(S):
        for j in np.flatnonzero(held[s]).tolist():
            u.req_cpu[s, j], u.req_mem[s, j], u.req_eph[s, j] = _vec(prob.init_req_cpu, N)[j], _vec(prob.init_req_mem, N)[j], _vec(prob.init_req_eph, N)[j]
            u.scalar_req[s, :, j] = isc[:, j]
            u.npods[s, j] = _vec(prob.init_npods, N)[j]
        for p, j in enumerate(placement[s].tolist()):
            if j < 0:
                continue
            assert held[s, j], (s, p, j)                       # (a pod never lands on a node its scenario lacks)
            u.req_cpu[s, j] += cpu[p]
            u.req_mem[s, j] += mem[p]
            u.req_eph[s, j] += eph[p]
            u.scalar_req[s, :, j] += sc[:, p]
            u.npods[s, j] += 1
    return u


def probe_request(prob, p):
    """(quantities [3 + K], entry bits) of "one more pod like pod p"."""
    K = _n_scalar(prob)
    q = [int(_vec(prob.req_cpu, prob.n_pods)[p]), int(_vec(prob.req_mem, prob.n_pods)[p]), int(_vec(prob.req_eph, prob.n_pods)[p])]
    q += [int(prob.scalar_req[k][p]) if prob.scalar_req is not None else 0 for k in range(K)]
    entries = int(prob.scalar_entries[p]) if prob.scalar_entries is not None else 0
    for k in range(K):
        if q[3 + k]:
            entries |= 1 << k
    return q, entries


def cap_of(alloc_pods, npods, alloc, used, q, entries):
    """The largest m >= 0 such that m further pods of request q pass fitsRequest (fit.go:230-302, as oracle/simon_oracle.c restates it) on
    a node with `used` requested of `alloc` (rows cpu, memory, ephemeral storage, scalars) and npods of alloc_pods pods."""
    cap = max(int(alloc_pods) - int(npods), 0)
    if q[0] == 0 and q[1] == 0 and q[2] == 0 and not entries:
        return cap                                             # the all-zero shortcut: pod slots only
    for r in range(len(q)):
        if r >= 3 and not (entries >> (r - 3)) & 1:
            continue                                           # no ScalarResources entry: not compared
        room = int(alloc[r]) - int(used[r])
        if room < 0:
            return 0                                           # Allocatable < request + Requested whatever the request
        if q[r] > 0:
            cap = min(cap, room // q[r])
    return cap


def static_ok(prob, cls, j):
    return True if prob.static_mask is None else bool((int(prob.static_mask[cls][j // 64]) >> (j % 64)) & 1)


def probe_exact(prob, p):
    cls = int(prob.pod_class[p]) if prob.pod_class is not None else 0
    at = lambda v, d=0: d if v is None else int(np.asarray(v)[p])                                         # noqa: E731
    if at(prob.gpu_mem) or at(prob.pod_gpu_cnt) or at(prob.gpu_index) or at(prob.pin_node, -1) >= 0 or at(prob.preset_node, -1) >= 0:
        return False
    if prob.term_topo_key is not None and len(prob.term_topo_key):
        for off in (prob.match_off, prob.anti_off, prob.port_off, prob.aff_off, prob.spread_hard_off):
            if off is not None and off[cls + 1] != off[cls]:
                return False
    return prob.local_spec_of is None or int(prob.local_spec_of[cls]) < 0


def headroom(prob, placement, held, probes, usage=None):
    """simon_fetch_headroom restated: (fit [S][K] int64, fit_nodes [S][K] int32, exact [K] bool)."""
    held = np.asarray(held, bool)
    S, N = held.shape
    K = _n_scalar(prob)
    u = usage or node_usage(prob, placement, held)
    alloc = np.stack([_vec(prob.alloc_cpu, N), _vec(prob.alloc_mem, N), _vec(prob.alloc_eph, N)] + [np.asarray(prob.scalar_alloc[k], np.int64) for k in range(K)])
    fit, nodes = np.zeros((S, len(probes)), np.int64), np.zeros((S, len(probes)), np.int32)
    for k, p in enumerate(np.asarray(probes).tolist()):
        q, entries = probe_request(prob, p)
        cls = int(prob.pod_class[p]) if prob.pod_class is not None else 0
        for s in range(S):
            for j in np.flatnonzero(held[s]).tolist():
                if not static_ok(prob, cls, j):
                    continue
                used = [u.req_cpu[s, j], u.req_mem[s, j], u.req_eph[s, j]] + [u.scalar_req[s, i, j] for i in range(K)]
                c = cap_of(prob.alloc_pods[j], u.npods[s, j], alloc[:, j], used, q, entries)
                fit[s, k] += c
                nodes[s, k] += c > 0
    return fit, nodes, np.array([probe_exact(prob, p) for p in np.asarray(probes).tolist()], bool)


def usage_errors(S, scen_ids, n, have=("req_cpu", "req_mem", "npods"), struct_ok=True, have_placement=True, reloaded=False):
    """simon_fetch_node_usage's refusals, restated: the rules a call breaks ([] = accepted)."""
    bad = []
    if not struct_ok:
        bad.append("struct_size")
    if any(name not in have for name in ("req_cpu", "req_mem", "npods")):
        bad.append("missing array")
    if n < 1:
        bad.append("n")
    elif scen_ids is None and n > S:
        bad.append("scenario id")
    elif scen_ids is not None and ((np.asarray(scen_ids)[:n] < 0).any() or (np.asarray(scen_ids)[:n] >= S).any()):
        bad.append("scenario id")
    if not bad and (not have_placement or reloaded):
        bad.append("no placements")
    return bad


def headroom_errors(P, probes, K, have_fit=True, have_placement=True, reloaded=False):
    """simon_fetch_headroom's refusals, restated."""
    bad = []
    if not have_fit:
        bad.append("missing array")
    if K < 1 or K > capi.MAX_PROBES:
        bad.append("K")
    elif (np.asarray(probes)[:K] < 0).any() or (np.asarray(probes)[:K] >= P).any():
        bad.append("pod id")
    if not bad and (not have_placement or reloaded):
        bad.append("no placements")
    return bad


def with_copies(prob, probe, m):
    """The problem with m copies of pod `probe` appended to the pod arrays (ids P .. P + m - 1)."""
    ids = np.concatenate([np.arange(prob.n_pods), np.full(m, probe)]).astype(np.int64)
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    for name in PU.POD_1D:
        if kw[name] is not None:
            kw[name] = np.asarray(kw[name])[ids].copy()
    for name in PU.POD_COL:
        if kw[name] is not None and np.asarray(kw[name]).size:
            kw[name] = np.asarray(kw[name])[:, ids].copy()
    return capi.Problem(**kw).normalise()


def check_probe_against_oracle(prob, n_nodes, order, placement, probe, fit, extra=3):
    """What `exact` promises: append fit + extra copies of the probe pod to the stream and run the unmodified oracle again -- exactly
    `fit` of them are placed, `extra` are not, and every earlier placement is unchanged."""
    P, m = prob.n_pods, int(fit) + extra
    more = with_copies(prob, probe, m)
    res = O.run(more, [[n_nodes, 0]], np.concatenate([np.asarray(order), np.arange(P, P + m)]).astype(np.int32)[None])
    row = res.placement[0]
    assert row[:P].tolist() == np.asarray(placement).tolist(), "the appended probes moved an earlier pod"
    assert int((row[P:] >= 0).sum()) == int(fit), (probe, int(fit), int((row[P:] >= 0).sum()))
    assert int((row[P:] == capi.UNSCHEDULED).sum()) == extra, (probe, row[P:].tolist())


def constructed_problem(seed, N):
    """(problem, named probes): randprob's problem (gates, pins, presets, a static mask, tight pod slots, K = 1 scalar) with four probe
    pods made by construction -- `besteffort` (no request at all: pod slots only), `zero_cpu` (no cpu, some memory) next to node 0
    over-committed in cpu through a preset pod (its cap there is 0), `zero_entry` (no request, one scalar ENTRY of quantity 0: the
    shortcut is off), `masked` (an ordinary pod whose class masks out nodes) and `fat` (more cpu than any node has: fits nowhere).
    The larger pool has few pod slots per node, the smaller one the default 110."""
    import randprob
    prob = randprob.rand_problem(seed, N=N, P=200, gates=True, pins=True, presets=True, static_mask=True, tight_pods=N > 20, scalars=1)
    P = prob.n_pods
    free = EU.eligible(prob)                                                   # no gate, pin, preset, eph or scalar request
    assert len(free) >= 6
    be, zc, ze, mk, big, fat = free[:6].tolist()
    cpu, mem = np.array(prob.req_cpu, np.int64), np.array(prob.req_mem, np.int64)
    pre, gate = np.array(prob.preset_node, np.int32), np.array(prob.gate_node, np.int32)
    ent = np.zeros(P, np.uint8)
    cpu[[be, zc, ze]] = 0
    mem[[be, ze]] = 0
    mem[zc] = 64 << 20
    ent[ze] = 1
    cpu[big] = 2 * int(prob.alloc_cpu[0])                                      # bound without a filter: node 0 ends over-committed in cpu
    cpu[fat] = int(np.max(prob.alloc_cpu)) + 1
    pre[big], gate[big] = 0, 0
    prob = EU.replaced(prob, req_cpu=cpu, req_mem=mem, nz_cpu=None, nz_mem=None, preset_node=pre,
                       gate_node=gate, scalar_entries=ent)
    return prob, {"besteffort": be, "zero_cpu": zc, "zero_entry": ze, "masked": mk, "fat": fat}


class PlainOracleEngine(PU.PodsetOracleEngine):
    """Oracle-backed engine without supports_node_usage: the sweeps compute the figures on the host and warn."""


class UsageOracleEngine(PU.PodsetOracleEngine):
    """Oracle-backed engine that answers headroom_pods / usage_of as HipEngine does, from the numpy restatement above."""
    supports_node_usage = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, pod_present=None,
            pod_groups=None, headroom_pods=None, usage_of=None):
        res = super().run(prob, scen, orders, True, node_ranks, want_gpu_slices, present, pod_present, pod_groups)
        held = held_rows(prob, capi.scenarios_array(scen), None if present is None else present[0])
        if headroom_pods is not None:
            res.headroom, _, res.headroom_exact = headroom(prob, res.placement, held, headroom_pods)
        if usage_of is not None:
            ids = np.asarray(usage_of, np.int32)
            u = node_usage(prob, res.placement[ids], held[ids])
            res.node_usage = capi.NodeUsage(ids, u.req_cpu, u.req_mem, u.npods, u.req_eph, u.scalar_req)
        return res

"""Shared pieces of the pod-subset tests (test_podsets_host.py, test_gpu_podsets.py): the yardstick -- the unmodified oracle on every
scenario's OWN problem, the capi.Problem with the absent pods deleted and the order compacted -- the presence rows the tests load, the
rules of simon_set_scenario_pods / simon_fetch_group_counts restated, and an oracle-backed engine that honours `pod_present`."""
import dataclasses
import functools

import numpy as np

import evict_util as EU
import mix_util as MU
import oracle_lib as O
import subset_util as SU
from open_simulator_amd import capi

# every pod-indexed field of capi.Problem ([P], or [K][P] for scalar_req)
POD_1D = ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "pod_class", "preset_node", "gate_node", "pin_node", "gpu_mem", "pod_gpu_cnt",
          "gpu_index", "scalar_entries", "priority")
POD_COL = ("scalar_req",)


def own_problem(prob, keep):
    """The problem with the pods outside `keep` (bool [P]) deleted: (problem, ids) with ids[i] = the pod id in `prob` of its pod i."""
    keep = np.asarray(keep, bool)
    ids = np.flatnonzero(keep)
    kw = {f.name: getattr(prob, f.name) for f in dataclasses.fields(prob) if not f.name.startswith("_")}
    for name in POD_1D:
        if kw[name] is not None:
            kw[name] = np.asarray(kw[name])[ids].copy()
    for name in POD_COL:
        if kw[name] is not None and np.asarray(kw[name]).size:
            kw[name] = np.asarray(kw[name])[:, ids].copy()
    return capi.Problem(**kw).normalise(), ids


def own_order(keep, order):
    """`order` restricted to the kept pods, in the own problem's pod ids."""
    keep = np.asarray(keep, bool)
    new_id = np.cumsum(keep) - 1
    order = np.asarray(order)
    return new_id[order[keep[order]]].astype(np.int32)


@dataclasses.dataclass
class OwnResult:
    placement: np.ndarray          # [P] by the pool problem's pod ids: absent pods read capi.GATED
    unscheduled: int
    used_cpu: int
    used_mem: int
    gpu_slices: np.ndarray = None  # [P] uint64, 0 for absent pods
    preempt_risk: int = 0


def _empty(prob, nodes):
    """A scenario holding no pod: nothing is scheduled, the used sums are the state before the stream over its nodes."""
    P = prob.n_pods
    cpu = int(np.asarray(prob.init_req_cpu)[nodes].sum()) if prob.init_req_cpu is not None else 0
    mem = int(np.asarray(prob.init_req_mem)[nodes].sum()) if prob.init_req_mem is not None else 0
    return OwnResult(np.full(P, capi.GATED, np.int32), 0, cpu, mem, np.zeros(P, np.uint64), 0)


def _widen(prob, ids, row, res):
    P = prob.n_pods
    full = np.full(P, capi.GATED, np.int32)
    full[ids] = row
    sl = np.zeros(P, np.uint64)
    if res.gpu_slices is not None:
        sl[ids] = res.gpu_slices[0]
    risk = int(res.preempt_risk[0]) if res.preempt_risk is not None else 0
    return OwnResult(full, int(res.unscheduled[0]), int(res.used_cpu[0]), int(res.used_mem[0]), sl, risk)


def oracle_prefix(prob, keep, n_nodes, order):
    """The oracle on the own problem of a PREFIX scenario: the first n_nodes pool nodes, the pods `keep`, fed in `order` restricted to them."""
    keep = np.asarray(keep, bool)
    if not keep.any():
        return _empty(prob, np.arange(n_nodes))
    own, ids = own_problem(prob, keep)
    res = O.run(own, [[n_nodes, 0]], own_order(keep, order)[None], want_gpu_slices=prob.gpu_mem is not None)
    return _widen(prob, ids, res.placement[0], res)


def oracle_nodes(prob, keep, present, order, ranks=None, evict=None):
    """The same for a scenario that holds the pool nodes `present` (bool [N]) in the order of its rank row; `evict`: the flagged pods
    (simon_set_pod_eviction) whose node it lacks are ordinary pods there (evict_util.scenario_problem)."""
    keep = np.asarray(keep, bool)
    if not keep.any():
        return _empty(prob, np.flatnonzero(present))
    if evict is not None:
        prob, _ = EU.scenario_problem(prob, evict, present)
    own, ids = own_problem(prob, keep)
    row, res = MU.oracle_of_scenario(own, np.asarray(present, bool), own_order(keep, order), ranks)
    return _widen(prob, ids, row, res)


def explain_prefix(prob, keep, n_nodes, order, max_failed=64):
    """The oracle's explain of the own problem: (n_failed, failed pods in the pool problem's ids, code rows [k][n_nodes])."""
    keep = np.asarray(keep, bool)
    if not keep.any():
        return 0, np.zeros(0, np.int32), np.zeros((0, n_nodes), np.uint16)
    own, ids = own_problem(prob, keep)
    _, (nf, failed, codes) = O.run(own, [[n_nodes, 0]], own_order(keep, order)[None], explain_scenario=0, max_failed=max_failed)
    return nf, ids[failed].astype(np.int32), codes


def explain_nodes(prob, keep, present, order, ranks, evict=None, max_failed=64):
    """... of a node-subset scenario: code rows by POOL node (0 on the nodes the scenario lacks), as simon_explain_own_batch writes them."""
    keep, present = np.asarray(keep, bool), np.asarray(present, bool)
    N = prob.n_nodes
    if not keep.any():
        return 0, np.zeros(0, np.int32), np.zeros((0, N), np.uint16)
    if evict is not None:
        prob, _ = EU.scenario_problem(prob, evict, present)
    own, ids = own_problem(prob, keep)
    nodes = np.flatnonzero(present)
    nodes = nodes[np.argsort(np.asarray(ranks)[nodes], kind="stable")]
    perm = np.concatenate([nodes, np.flatnonzero(~present)])
    _, (nf, failed, codes) = O.run(MU.permute_nodes(own, perm), [[len(nodes), 0]], own_order(keep, order)[None], explain_scenario=0, max_failed=max_failed)
    rows = np.zeros((len(codes), N), np.uint16)
    rows[:, nodes] = codes
    return nf, ids[failed].astype(np.int32), rows


def bins_of(row):
    """(code, node count) pairs of one code row over the scenario's own nodes (code 0 = a node it lacks), ascending by code."""
    codes, counts = np.unique(np.asarray(row)[np.asarray(row) != 0], return_counts=True)
    return list(zip(codes.tolist(), counts.tolist()))


def standard_rows(prob, orders, scen, seed=0):
    """bool [8][P]: all pods; no pods; only stream position 0; all but the last position; one whole pod class (the most frequent) absent;
    three seeded random rows at density 0.5.  Positions are those of each scenario's own order."""
    P = prob.n_pods
    rng = np.random.default_rng(seed)
    rows = np.ones((8, P), bool)
    rows[1] = False
    rows[2] = False
    rows[2, orders[scen[2, 1]][0]] = True
    rows[3, orders[scen[3, 1]][P - 1]] = False
    cls = np.asarray(prob.pod_class) if prob.pod_class is not None else np.zeros(P, np.int64)
    rows[4] = cls != np.bincount(cls).argmax()
    for s in (5, 6, 7):
        rows[s] = rng.random(P) < 0.5
    return rows


def conditions(full, others):
    """The two properties a case must have by the oracle alone: (a) some scenario places a pod that the all-present one leaves
    unscheduled; (b) some present pod lands on another node than in the all-present one."""
    a = any(((o.placement >= 0) & (full.placement == capi.UNSCHEDULED)).any() for o in others)
    b = any(((o.placement >= 0) & (full.placement >= 0) & (o.placement != full.placement)).any() for o in others)
    return a, b


@functools.lru_cache(maxsize=None)
def route_case(case):
    """(problem, scen, orders, rows [8][P], oracle results) of one score-table route: evict_util.route_problem's problem (gates, no
    presets) with four pods preset to nodes 0 and 1, as a PREFIX batch of eight scenarios over both orders.  The node count is the
    largest at which the all-present scenario leaves pods unscheduled that a sparser scenario places (conditions): found with the oracle,
    once, and shared.  Rows 6 and 7 hold a few nodes more, so that the gate rule and the rows meet."""
    prob, orders = EU.route_problem(case)
    N, P = prob.n_nodes, prob.n_pods
    ok = EU.eligible(prob)
    pre = np.full(P, -1, np.int32) if prob.preset_node is None else np.array(prob.preset_node, np.int32)
    pre[ok[:4]] = [0, 1, 0, 1][:len(ok[:4])]
    prob = EU.replaced(prob, preset_node=pre)
    return search_case(prob, orders, sum(map(ord, case)))


def search_case(prob, orders, seed, rows_of=None, order_of=None, more=3):
    """(problem, scen, orders, rows [8][P], oracle results): eight prefix scenarios of the largest node count (two at least: the preset
    pods sit on nodes 0 and 1; pools of at most 80 nodes try every count, larger ones a fixed ladder) at which the all-present scenario 0
    and the others on the same nodes meet `conditions`; scenarios 6 and 7 hold `more` nodes more.  rows_of(scen): the presence rows
    (default standard_rows); order_of: the order of every scenario."""
    N = prob.n_nodes
    ladder = range(N, 1, -1) if N <= 80 else sorted({N, 3 * N // 4, N // 2, N // 3, N // 4, N // 6, N // 8, N // 12, N // 16, N // 24, N // 32, N // 48, N // 64, 3, 2}, reverse=True)
    for n in ladder:
        if n < 2:
            continue
        scen = np.array([[n if s < 6 else min(N, n + more), (s % len(orders)) if order_of is None else order_of[s]] for s in range(8)], np.int32)
        rows = standard_rows(prob, orders, scen, seed) if rows_of is None else rows_of(scen)
        assert rows[0].all() and scen[0, 1] == 0
        full = oracle_prefix(prob, rows[0], n, orders[0])
        if full.unscheduled == 0:
            continue
        res = [full] + [oracle_prefix(prob, rows[s], int(scen[s, 0]), orders[scen[s, 1]]) for s in range(1, 8)]
        if all(conditions(full, res[1:6] if more else res[1:])):
            return prob, scen, orders, rows, res
    raise AssertionError("no node count at which absence changes what the other pods get")


def compare(res, want, gpu=False):
    """A device BatchResult against the oracle's own-problem results, scenario by scenario, pod by pod."""
    for s, w in enumerate(want):
        got = res.placement[s]
        assert got.tolist() == w.placement.tolist(), (s, np.flatnonzero(got != w.placement)[:8].tolist())
        assert (int(res.unscheduled[s]), int(res.used_cpu[s]), int(res.used_mem[s])) == (w.unscheduled, w.used_cpu, w.used_mem), s
        if gpu:
            assert (res.gpu_slices[s] == w.gpu_slices).all(), s


def podset_errors(P, S, words, loaded=True):
    """simon_set_scenario_pods' refusals (include/simon_hip.h), restated: the rules a call breaks ([] = accepted).  words: what the call
    receives, [S][ceil(P / 32)] uint32, or None (detach)."""
    if not loaded:
        return ["nothing loaded"]
    if words is None:
        return []
    w = np.asarray(words, np.uint32).reshape(S, -1)
    assert w.shape[1] == (P + 31) // 32
    bits = np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=1, bitorder="little").astype(bool)
    return ["bit beyond P"] if bits[:, P:].any() else []


def group_errors(P, pod_group, G, have_placement=True):
    """simon_fetch_group_counts' refusals, restated."""
    bad = []
    if G < 1 or G > capi.MAX_POD_GROUPS:
        bad.append("G")
    elif (np.asarray(pod_group) < -1).any() or (np.asarray(pod_group) >= G).any():
        bad.append("group id")
    if not bad and not have_placement:
        bad.append("no placements")
    return bad


def group_counts(placement, pod_group, G):
    """numpy's answer to simon_fetch_group_counts: (unscheduled [S][G], placed [S][G])."""
    placement, g = np.asarray(placement), np.asarray(pod_group)
    uns = np.zeros((len(placement), G), np.int32)
    pl = np.zeros((len(placement), G), np.int32)
    for s, row in enumerate(placement):
        uns[s] = np.bincount(g[(g >= 0) & (row == capi.UNSCHEDULED)], minlength=G)
        pl[s] = np.bincount(g[(g >= 0) & (row >= 0)], minlength=G)
    return uns, pl


class PodsetOracleEngine(SU.SubsetOracleEngine):
    """Test-only engine that honours `pod_present` (and `pod_groups`): scenario s runs on the oracle on its own problem -- the device's
    stand-in where sweep_apps' batched road is under test on a host without a GPU."""
    supports_pod_subsets = True

    def __init__(self):
        self.batches = 0
        self.explained = []

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, pod_present=None,
            pod_groups=None):
        if pod_present is None:
            res = super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices, present)
        else:
            assert present is None
            self.batches += 1
            scen = capi.scenarios_array(scen)
            rows = np.asarray(pod_present, bool)
            assert rows.shape == (len(scen), prob.n_pods)
            res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
            for s in range(len(scen)):
                if node_ranks is not None:
                    one = oracle_nodes(prob, rows[s], np.arange(prob.n_nodes) < scen[s, 0], np.asarray(orders)[scen[s, 1]], node_ranks[s])
                else:
                    one = oracle_prefix(prob, rows[s], int(scen[s, 0]), np.asarray(orders)[scen[s, 1]])
                res.placement[s], res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = one.placement, one.unscheduled, one.used_cpu, one.used_mem
                if want_gpu_slices:
                    res.gpu_slices[s] = one.gpu_slices
            self._last = (prob, scen, np.asarray(orders), rows, node_ranks)
        if pod_groups is not None:
            G = int(np.max(pod_groups, initial=-1)) + 1
            res.group_unscheduled, res.group_placed = group_counts(res.placement, pod_groups, max(G, 1))
        return res

    supports_explain_batch = True

    def explain_batch(self, prob, scen, orders, node_ranks, ids, max_failed, max_bins=32, *, pod_present=None):
        """HipEngine.explain_batch's answer from the oracle's explain of every listed scenario's own problem (full code rows)."""
        from open_simulator_amd.simulate import ExplainedScenario
        scen = capi.scenarios_array(scen)
        rows = np.ones((len(scen), prob.n_pods), bool) if pod_present is None else np.asarray(pod_present, bool)
        out = []
        for s in ids:
            n = int(scen[s, 0])
            if node_ranks is None:
                nf, failed, codes = explain_prefix(prob, rows[s], n, np.asarray(orders)[scen[s, 1]], max_failed)
            else:                                                      # (rows by pool node: the scenario's are the first n)
                nf, failed, codes = explain_nodes(prob, rows[s], np.arange(prob.n_nodes) < n, np.asarray(orders)[scen[s, 1]], node_ranks[s], None, max_failed)
                codes = codes[:, :n]
            out.append(ExplainedScenario(int(s), int(scen[s, 0]), nf, failed, [None] * len(failed), codes, O.LAST_LOCAL_DETAIL[0]))
        self.explained.append([int(s) for s in ids])
        return out

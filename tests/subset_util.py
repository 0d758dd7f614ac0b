"""Shared pieces of the node-subset tests (test_subsets_host.py, test_gpu_subsets.py): an oracle-backed engine that takes presence rows,
the rank rows of a presence matrix restated in plain loops, the validator's rules in numpy, the presence rows of the staging test and
sweep_failures' answer for a cluster by the slow road (simulate() of every reduced cluster on the oracle)."""
import numpy as np

import mix_util as MU
from open_simulator_amd import capi, simulate as sim


def zone_ranks(present, node_zone=None):
    """rank[s][j] of pool node j in nodeTree.list() of scenario s's own nodes (zones in first-appearance order, one node per zone per
    round), -1 where absent: plain loops, the second opinion on simulate.mix_node_ranks and on the device's closed form."""
    present = np.asarray(present, bool)
    S, N = present.shape
    z = np.zeros(N, np.int64) if node_zone is None else np.asarray(node_zone)
    out = np.full((S, N), -1, np.int32)
    for s in range(S):
        zones, tree = [], {}
        for j in np.flatnonzero(present[s]).tolist():
            if int(z[j]) not in tree:
                zones.append(int(z[j]))
                tree[int(z[j])] = []
            tree[int(z[j])].append(j)
        r, k = 0, 0
        while r < int(present[s].sum()):
            for q in zones:
                if k < len(tree[q]):
                    out[s, tree[q][k]] = r
                    r += 1
            k += 1
    return out


class SubsetOracleEngine(MU.OracleEngine):
    """Test-only engine that takes node subsets, every scenario through oracle_of_scenario on its own node set in its own nodeTree order:
    the device's stand-in where sweep_failures' batched road is under test on a host without a GPU."""
    supports_scenario_subsets = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None):
        if present is None:
            return super().run(prob, scen, orders, want_placement, node_ranks, want_gpu_slices)
        mask, zone = present
        scen = capi.scenarios_array(scen)
        assert (np.asarray(mask).sum(1) == scen[:, 0]).all()
        ranks = node_ranks if node_ranks is not None else zone_ranks(mask, zone)
        res = capi.BatchResult.alloc(len(scen), prob.n_pods, True, want_gpu_slices)
        for s in range(len(scen)):
            row, r = MU.oracle_of_scenario(prob, np.asarray(mask)[s], np.asarray(orders)[scen[s, 1]], ranks[s])
            res.placement[s], res.unscheduled[s], res.used_cpu[s], res.used_mem[s] = row, r.unscheduled[0], r.used_cpu[0], r.used_mem[0]
            if want_gpu_slices and r.gpu_slices is not None:
                res.gpu_slices[s] = r.gpu_slices[0]
            if res.used_vg is not None and r.used_vg is not None:
                res.used_vg[s] = r.used_vg[0]
            if r.preempt_risk is not None:
                if res.preempt_risk is None:
                    res.preempt_risk = np.zeros(len(scen), np.uint8)
                res.preempt_risk[s] = r.preempt_risk[0]
        self.last_stats = None
        return res


def names_of(res):
    """(namespace, pod name) -> node name or None of a SimulateResult."""
    where = {}
    for st in res.node_status:
        for p in st["pods"]:
            where[(p["metadata"].get("namespace", ""), p["metadata"]["name"])] = st["node"]["metadata"]["name"]
    for u in res.unscheduled_pods:
        where[(u["pod"]["metadata"].get("namespace", ""), u["pod"]["metadata"]["name"])] = None
    return where


def reduced_answers(cluster, apps, doms, engine=None):
    """simulate() of the whole cluster and of the cluster without every domain, on the oracle: [(where, unscheduled count)]."""
    engine = engine or MU.OracleEngine()
    out = []
    for names in [[]] + list(doms):
        res = sim.simulate(*sim.cluster_without(cluster, apps, names), engine=engine)
        out.append((names_of(res), len(res.unscheduled_pods)))
    return out


def subset_errors(prob, scen, present, node_zone=None, n_zones=None):
    """simon_set_scenario_nodes' refusals (include/simon_hip.h), restated: the list of rules a call breaks ([] = accepted).  present is
    the WORD matrix [S][ceil(N / 32)] the call receives."""
    N, S = prob.n_nodes, len(scen)
    words = np.asarray(present, np.uint32).reshape(S, -1)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little").astype(bool)
    bad = []
    if bits[:, N:].any():
        bad.append("bits beyond N")
    own = bits[:, :N]
    if (own.sum(1) == 0).any():
        bad.append("empty scenario")
    if (own.sum(1) != np.asarray(scen)[:, 0]).any():
        bad.append("n_nodes mismatch")
    if node_zone is not None:
        nz = int(np.max(node_zone)) + 1 if n_zones is None else n_zones
        if nz < 1 or nz > capi.MAX_ZONES:
            bad.append("n_zones")
        elif (np.asarray(node_zone) < 0).any() or (np.asarray(node_zone) >= nz).any():
            bad.append("zone ids")
    lost = ~own.all(0)                                       # nodes that some scenario lacks
    for name in ("init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem", "init_npods", "init_gpu_used", "init_vg_req",
                 "init_dev_alloc"):
        v = getattr(prob, name)
        if v is not None and np.asarray(v).reshape(N, -1)[lost].any():
            bad.append("init state")
            break
    else:
        if prob.init_scalar_req is not None and prob.init_scalar_req[:, lost].any():
            bad.append("init state")
    if prob.preset_node is not None:
        pre = np.asarray(prob.preset_node)
        gate = np.asarray(prob.gate_node) if prob.gate_node is not None else np.full(len(pre), -1)
        if ((pre >= 0) & lost[np.maximum(pre, 0)] & (gate != pre)).any():
            bad.append("preset")
    return bad


def staging_masks(N, node_zone, seed):
    """The 12 presence rows of the staging test: all present, only the first node, only the last, the first node absent, a whole zone
    absent (the zone order shifts), alternating bits, a word of zeros in the middle, and five seeded random rows."""
    rng = np.random.default_rng(seed)
    z = np.zeros(N, np.int64) if node_zone is None else np.asarray(node_zone)
    rows = [np.ones(N, bool), np.arange(N) == 0, np.arange(N) == N - 1, np.arange(N) != 0, z != z[0], np.arange(N) % 2 == 0,
            ~((np.arange(N) >= 32 * (N // 64)) & (np.arange(N) < 32 * (N // 64) + 32))]
    for k in range(5):
        rows.append(rng.random(N) < (0.2, 0.5, 0.8, 0.5, 0.95)[k])
    rows = np.stack(rows)
    for r in rows:                                           # (a scenario holds one node at least: N = 1, one zone, ...)
        if not r.any():
            r[int(rng.integers(0, N))] = True
    return rows

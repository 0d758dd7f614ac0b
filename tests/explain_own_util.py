"""Shared pieces of the own-nodes explain tests (test_explain_own_host.py, test_gpu_explain_own.py): the yardstick -- the unmodified C
oracle's explain on the scenario's OWN problem (its nodes moved to the front in rank order, mix_util.permute_nodes), its codes mapped
back through the permutation to pool indices -- and test-only engines that implement explain_own_batch through it."""
import numpy as np

import evict_util as EU
import explain_util as XU
import mix_util as MU
import oracle_lib as O
import subset_util as SU
from open_simulator_amd import capi, simulate as sim


def oracle_explain(prob, present, order, ranks=None, max_failed=64):
    """(n_failed, failed pod ids [k], rows [k][N]) of the scenario that holds the pool nodes `present` (bool [N]), k = min(n_failed,
    max_failed): rows are indexed by POOL node, 0 on the nodes the scenario lacks."""
    present = np.asarray(present, bool)
    own = np.flatnonzero(present)
    if ranks is not None:
        own = own[np.argsort(np.asarray(ranks)[own], kind="stable")]
    perm = np.concatenate([own, np.flatnonzero(~present)])
    _, (nf, failed, codes) = O.run(MU.permute_nodes(prob, perm), [[len(own), 0]], np.asarray(order, np.int32)[None], explain_scenario=0,
                                   max_failed=max_failed)
    rows = np.zeros((len(failed), prob.n_nodes), np.uint16)
    rows[:, own] = np.asarray(codes)[:, :len(own)]
    return int(nf), np.asarray(failed, np.int32), rows


def oracle_bins(row, present):
    """(codes ascending, counts) over the scenario's present nodes: what simon_explain_own_batch's bins must hold."""
    return XU.binned(np.asarray(row)[np.asarray(present, bool)])


def assert_explained(eb, k, prob, present, order, ranks, max_failed, max_bins, want_rows):
    """Listed scenario k of an ExplainBatch from explain_own_batch against the oracle: the count, the recorded pods, pool-indexed rows
    with 0 on absent nodes and nowhere else, the bins over present nodes and their sum.  Returns the oracle's (n_failed, rows)."""
    present = np.asarray(present, bool)
    nf, failed, rows = oracle_explain(prob, present, order, ranks, max_failed)
    assert int(eb.n_failed[k]) == nf, (k, int(eb.n_failed[k]), nf)
    rec = eb.recorded(k)
    assert rec == len(failed) and eb.failed_pods[k, :rec].tolist() == failed.tolist(), k
    assert int(eb.n_nodes[k]) == int(present.sum())
    if want_rows:
        got = eb.rows[k, :rec, :prob.n_nodes]
        assert (got == rows).all(), (k, np.argwhere(got != rows)[:4].tolist())
        assert not got[:, ~present].any() and got[:, present].all()
        assert not eb.rows[k, rec:].any() and not eb.rows[k, :, prob.n_nodes:].any()
    for i in range(rec):
        codes, counts = oracle_bins(rows[i], present)
        assert 0 not in codes, (k, i)                                 # no present node of a failed pod carries 0
        assert sum(counts) == int(present.sum())
        nb = int(eb.n_bins[k, i])
        assert nb == (len(codes) if len(codes) <= capi.EXPLAIN_BINS else -1), (k, i, nb, len(codes))
        if 0 <= nb <= max_bins:
            assert eb.pod_bins(k, i) == list(zip(codes, counts)), (k, i)
            assert sum(c for _, c in eb.pod_bins(k, i)) == int(eb.n_nodes[k])
        else:
            assert eb.pod_bins(k, i) is None
    return nf, rows


def families(rows):
    """The failure families (highest set bit of a code) seen in code rows."""
    return {1 << (int(c).bit_length() - 1) for c in np.unique(rows).tolist() if c}


class _OwnExplain:
    """explain_own_batch through the oracle, in HipEngine's shape: ExplainedScenario per listed id with bins over present nodes and, for
    every scenario, its pool-indexed rows (the histogram road and the row road of HipEngine both end in the same texts)."""
    supports_explain_own = True
    own_calls = 0

    def explain_own_batch(self, prob, scen, orders, node_ranks, ids, max_failed, max_bins=32, *, present=None, segments=None, evict=None):
        type(self).own_calls += 1
        scen = capi.scenarios_array(scen)
        if segments is not None:
            mask = np.stack([MU.present_mask(prob.n_nodes, segments[0], np.asarray(segments[1])[s]) for s in range(len(scen))])
            zone = None
        else:
            mask, zone = present
        mask = np.asarray(mask, bool)
        ranks = node_ranks if node_ranks is not None else SU.zone_ranks(mask, zone)
        out = []
        for s in [int(s) for s in ids]:
            ps = EU.scenario_problem(prob, evict, mask[s])[0] if evict is not None else prob
            nf, failed, rows = oracle_explain(ps, mask[s], np.asarray(orders)[scen[s, 1]], ranks[s], max_failed)
            bins = [list(zip(*oracle_bins(r, mask[s]))) for r in rows]
            out.append(sim.ExplainedScenario(s, int(mask[s].sum()), nf, failed, bins, rows))
        return out


class OwnSubsetOracleEngine(_OwnExplain, EU.EvictOracleEngine):
    """Node subsets, evictions and explain_own_batch, all on the oracle."""


class OwnSegmentOracleEngine(_OwnExplain, MU.SegmentOracleEngine):
    """Pool segments and explain_own_batch, all on the oracle."""

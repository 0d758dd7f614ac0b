"""CPU-only checks behind tests/test_gpu_step_waits.py: the stream layouts do put the rare pods on the chunk edges, the rare paths occur in
the oracle's results, and the plan the GPU tests recompute from fetched results is the oracle's plan."""
import numpy as np
import pytest

import oracle_lib as O
from open_simulator_amd import synth

import test_gpu_step_waits as T


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 128, 129, 191, 193])
def test_rare_pods_sit_on_the_chunk_edges(P):
    orders, steps = T.chunk_orders(P)
    want = sorted({e % P for e in T.EDGES if -P <= e < P})
    assert steps == want[:6] and len(orders) == 4
    special = set(range(min(P, 6)))
    at_edge = [set() for _ in steps]
    for order in orders:
        assert sorted(order.tolist()) == list(range(P))
        for i, s in enumerate(steps):
            assert int(order[s]) in special
            at_edge[i].add(T.KINDS[int(order[s]) % 3])
    if P >= 6:
        assert all(len(k) == 3 for k in at_edge)           # every kind meets every edge over the four orders


def test_rare_paths_occur_in_the_oracle():
    prob, scen, orders, steps, ref = T.chunk_case(129)
    pinned = [i for i in range(6) if T.KINDS[i % 3] == "pinned"]
    gated = [i for i in range(6) if T.KINDS[i % 3] == "gated"]
    pl = ref.placement[:, pinned]
    assert (pl == np.asarray(prob.pin_node)[pinned]).any() and (pl == -1).any()        # pinned pods that land and that do not
    assert (ref.placement[scen[:, 0] < T.N_NODES][:, gated] == -2).all()
    assert ((ref.placement == -1).sum(axis=1) == ref.unscheduled).all()


def test_recomputed_plan_is_the_oracles_plan():
    prob, scen, orders = synth.config3(n_counts=8, n_orders=3, n_pods=600, n_het=40)
    res = O.run(prob, scen, orders, want_placement=False)
    seen = set()
    for caps in ((100, 100), (60, 100), (100, 50), (1, 1)):
        want, plan = T.parent_plan(prob, scen, res, None, caps), O.min_plan(prob, scen, res, *caps).as_dict()
        seen.add(want is not None)
        if want is None:
            assert plan["found"] == 0 and plan["scenario"] == -1
        else:
            assert {k: plan[k] for k in want} == want
    assert seen == {True, False}
    present = np.arange(prob.n_nodes)[None, :] < scen[:, :1]                            # prefix scenarios as node subsets: the same plan
    assert T.parent_plan(prob, scen, res, present) == T.parent_plan(prob, scen, res)

"""The duel fixtures of tests/duel_util.py, proven on the CPU before any kernel sees them (tests/test_gpu_duels.py): the C oracle
and the Python reference -- written independently -- agree on them, every near-miss model loses every duel of the kinds it targets,
every problem holds enough duels of every kind it claims, and the pair of problems at the narrow route's range edge sits where
it should.  The domain assertions (cpu and memory gcd 1, largest node + all pods < 2^31) are part of duel_util.build.

Kinds dropped under the search rule of duel_util: none (ba_int and ba_contracted are kept: test_ba_contracted_search)."""
import numpy as np
import pytest

import duel_util as U
import oracle_lib as O

NAMES = list(U.FIXTURES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_python_reference_agree(name):
    fx = U.fixture(name)
    ref = O.run(fx.prob, fx.scen, fx.orders)
    N = fx.prob.n_nodes
    for s, (n, o) in enumerate(fx.scen.tolist()):
        place, unsched, used_c, used_m = U.schedule(fx.prob, fx.orders[o], n)
        assert ref.placement[s].tolist() == place, (name, s)
        assert (int(ref.unscheduled[s]), int(ref.used_cpu[s]), int(ref.used_mem[s])) == (unsched, used_c, used_m), (name, s)
        assert unsched == 0
        if n == N:
            assert place == fx.expected.tolist(), (name, s)
        else:                                                   # a prefix scenario holds whole duels: the others' pods are gated, not failed
            inside = np.asarray(fx.prob.gate_node) < n
            assert inside.any() and not inside.all()
            assert np.array_equal(np.where(inside, fx.expected, U.capi.GATED), np.array(place))


@pytest.mark.parametrize("name", NAMES)
def test_the_kernels_own_forms_equal_the_exact_reference(name):
    """la_term / la_term_t, div_by_rcp / div_by_rcp1 and the class term as the proofs state them, in correctly rounded Python"""
    fx = U.fixture(name)
    for ar in U.KERNEL_FORMS:
        assert U.schedule(fx.prob, fx.orders[3], fx.prob.n_nodes, ar)[0] == fx.expected.tolist(), ar.name


def _duel_pods(fx):
    per = fx.prob.n_pods // len(fx.duels)
    return [per * d + per - 1 for d in range(len(fx.duels))]


@pytest.mark.parametrize("model", list(U.MODELS))
def test_every_near_miss_model_loses_every_duel_of_its_kinds(model):
    ar, kinds = U.MODELS[model]
    seen = 0
    for name in NAMES:
        fx = U.fixture(name)
        mine = [d for d, duel in enumerate(fx.duels) if duel.kind in kinds or duel.base_kind in kinds]
        if not mine:
            continue
        pods = _duel_pods(fx)
        for o in (0, 2):
            place = U.schedule(fx.prob, fx.orders[o], fx.prob.n_nodes, ar)[0]
            wrong = [d for d in mine if place[pods[d]] != fx.expected[pods[d]]]
            assert wrong == mine, (model, name, sorted(set(mine) - set(wrong)))
        seen += len(mine)
    assert seen >= 8, (model, seen)


@pytest.mark.parametrize("name", NAMES)
def test_kind_counts(name):
    fx = U.fixture(name)
    count = {}
    for duel in fx.duels:
        count[duel.base_kind] = count.get(duel.base_kind, 0) + 1
    claimed = {k.split(":")[0] for k in fx.kinds}
    assert set(count) == claimed
    assert all(v >= 8 for v in count.values()), count
    for kind in ("la_edge", "la_int"):                          # both sub-kinds of the kinds that have two
        if kind in claimed:
            assert len({d.kind for d in fx.duels if d.base_kind == kind}) == 2


def test_problem_sizes_reach_the_instantiations():
    """60 signatures on 60 internal node classes; 100 signatures (two per lane) on 50 shapes; class-term problems of 64 internal classes"""
    fx = U.fixture("laba60_refresh")
    assert (fx.prob.n_nodes, fx.prob.n_pods, fx.prob.n_pod_classes) == (120, 180, 60)
    fx = U.fixture("laba100_two_per_shape")
    assert len({(int(a), int(b)) for a, b in zip(fx.prob.alloc_cpu, fx.prob.alloc_mem)}) == 50 and fx.prob.n_pod_classes == 100
    assert len({(int(a), int(b)) for a, b in zip(fx.prob.req_cpu, fx.prob.req_mem)}) == 100
    for name in ("simon16", "na16", "tt16"):
        fx = U.fixture(name)
        assert fx.prob.n_nodes == 64 and fx.prob.n_node_classes == 4
    fx = U.fixture("laba60_nz")
    assert (fx.prob.nz_cpu != fx.prob.req_cpu).all() and (fx.prob.init_nz_mem != fx.prob.init_req_mem).all()


def test_class_term_raw_scores_span_30_bits():
    for name, tab in (("simon16", "simon_raw"), ("na16", "node_affinity_raw"), ("tt16", "taint_prefer_raw")):
        t = getattr(U.fixture(name).prob, tab)
        assert (t >= 0).all() and (t <= U.RAW_MAX).all() and (t.max(axis=1) >= 1 << 29).all()


def test_range_edge_pair():
    inside, outside = U.fixture("edge_inside"), U.fixture("edge_outside")
    assert U.route_bound(inside.prob) == (1 << 31) - 1
    assert U.route_bound(outside.prob) == 1 << 31
    assert inside.expected.tolist() == outside.expected.tolist()
    for fx in (inside, outside):
        ref = O.run(fx.prob, fx.scen[:1], fx.orders)
        assert ref.placement[0].tolist() == fx.expected.tolist() and ref.unscheduled.tolist() == [0]


def test_ba_contracted_search():
    """The directed search for states on which one fma truncates (1 - diff) 100 differently from the two-rounding form: how often it
    succeeds (the issue's rule: none within 10^6 candidates would drop ba_contracted and ba_int)"""
    for name in NAMES:
        U.fixture(name)
    tried, found = U.BA_INT_TRIED
    print(f"ba_int search: {found} states among {tried} candidates")
    assert found >= 56 and tried <= 10 ** 6

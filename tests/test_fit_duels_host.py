"""The fit-duel fixtures of tests/fit_duel_util.py, proven on the CPU before any kernel sees them (tests/test_gpu_fit_duels.py): the C oracle
and the Python reference -- written independently -- agree on them with no pod left unscheduled, and every near-miss model loses EVERY duel
of the kinds it is listed for and wins every other one, on the whole problem and under two orders.  Run with -s for the table: per fixture
the kinds, and per model the duels it loses out of the duels of its kinds.  The domain assertions (gcds, quotients below 2^31, used <= alloc,
at most 32 requests of either sort, no presets, the cpu / memory bound of choose_variant) are part of fit_duel_util.build.

Models and kinds dropped under the rule of fit_duel_util: gpu_floor_late (dead on every input: the module's docstring has the argument)."""
import numpy as np
import pytest

import fit_duel_util as F
import oracle_lib as O

NAMES = list(F.FIXTURES)


def _oracle(fx):
    return O.run(fx.prob, fx.scen, fx.orders, want_gpu_slices=fx.ft.gpu)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_python_reference_agree(name):
    fx = F.fixture(name)
    ref = _oracle(fx)
    N = fx.prob.n_nodes
    for s, (n, o) in enumerate(fx.scen.tolist()):
        place, unsched, used_c, used_m, slices = F.schedule(fx.prob, fx.orders[o], n)
        assert ref.placement[s].tolist() == place, (name, s)
        assert (int(ref.unscheduled[s]), int(ref.used_cpu[s]), int(ref.used_mem[s])) == (unsched, used_c, used_m) and unsched == 0, (name, s)
        if fx.ft.gpu:
            assert [int(v) for v in ref.gpu_slices[s]] == slices, (name, s)
        if n == N:
            assert place == fx.expected.tolist() and slices == [int(v) for v in fx.slices], (name, s)
        else:                                                   # a prefix scenario holds whole duels: the others' pods are gated, not failed
            inside = np.asarray(fx.prob.gate_node) < n
            assert inside.any() and not inside.all()
            assert np.array_equal(np.where(inside, fx.expected, F.capi.GATED), np.array(place))


@pytest.mark.parametrize("name", NAMES)
def test_every_model_loses_every_duel_of_its_kinds_and_no_other(name):
    fx = F.fixture(name)
    D = len(fx.duels)
    kinds = sorted({d.kind for d in fx.duels})
    print(f"\n{name}: {D} duels, kinds {', '.join(kinds)}")
    want = (fx.expected.tolist(), [int(v) for v in fx.slices])
    for model, (fit, _) in F.MODELS.items():
        mine = [d for d, duel in enumerate(fx.duels) if model in F.targets(duel.kind)]
        for o in (0, 2):
            place, _, _, _, slices = F.schedule(fx.prob, fx.orders[o], fx.prob.n_nodes, fit)
            lost = [d for d in range(D) if any(place[p] != want[0][p] or slices[p] != want[1][p] for p in fx.duel_pods(d))]
            assert lost == mine, (model, name, o, sorted(set(lost) ^ set(mine)))
        print(f"  {model:16s} loses {len(mine):2d} of {len(mine):2d} duels of its kinds, none of the other {D - len(mine)}")


def test_every_kind_has_teeth_and_every_model_bites():
    """over all fixtures: a kind some model loses, a model that loses some kind, and both sub-forms / all components / all counts are there"""
    kinds = {d.kind for n in F.DUEL_FIXTURES for d in F.fixture(n).duels}
    assert kinds == set(F.XRES_LIST + F.GCD_KINDS + F.GPU_LIST)
    assert all(F.targets(k) for k in kinds)
    for model in F.MODELS:
        seen = sum(model in F.targets(d.kind) for n in F.DUEL_FIXTURES for d in F.fixture(n).duels)
        assert seen >= 8, (model, seen)


@pytest.mark.parametrize("name", F.DUEL_FIXTURES)
def test_shape_of_a_fixture(name):
    fx = F.fixture(name)
    _, kinds, D, flavour, ft, _ = F.FIXTURES[name]
    assert fx.prob.n_nodes <= 200 and fx.prob.n_pods <= 200 and len(fx.scen) == 6 and len(fx.duels) == D
    assert {d.kind for d in fx.duels} == set(kinds)
    assert (fx.prob.preset_node is None) and (fx.prob.gate_node >= 0).all()
    classes = {(int(c), int(a), int(b)) for c, a, b in zip(fx.prob.node_class, fx.prob.alloc_cpu, fx.prob.alloc_mem)}
    assert len(classes) >= 70 if name.endswith("70classes") else len(classes) <= 8
    for d, duel in enumerate(fx.duels):
        roles = [pd.role for pd in duel.pods]
        assert roles.count("probe") == 1 and ("setter" in roles) == (flavour == "refresh")
        probe = duel.pods[roles.index("probe")]
        assert len(probe.admit) == (4 if ft.anti else 3)
        for pd in duel.pods:                                    # a setter's request signature differs from the probe's
            if pd.role == "setter":
                assert (pd.x_req, pd.gpu_mem, pd.gpu_cnt) != (probe.x_req, probe.gpu_mem, probe.gpu_cnt) and len(pd.admit) == 1
        for o in fx.orders:                                     # an order keeps a duel's pods together and in their order
            pos = [int(np.nonzero(o == p)[0][0]) for p in fx.duel_pods(d)]
            assert pos == list(range(pos[0], pos[0] + len(pos)))


def test_magnitudes():
    """quantities of 2^27 .. 2^31 - 1 units, 2^31 - 1 itself among them; raw ephemeral values beyond 2^32 on the gcd problems"""
    fx = F.fixture("xres_initial")
    assert int(fx.prob.alloc_eph.max()) == F.LIM31 - 1 and int(fx.prob.scalar_alloc.max()) == F.LIM31 - 1
    assert int(fx.prob.req_eph[fx.prob.req_eph > 0].min()) >= 1 << 27
    fx = F.fixture("gpu_initial")
    per_dev = fx.prob.gpu_mem_total // np.maximum(fx.prob.gpu_cnt, 1)
    assert int(per_dev.max()) == F.LIM31 - 1 and int(per_dev.min()) >= 1 << 30 and (fx.prob.gpu_mem_total % fx.prob.gpu_cnt != 0).any()
    assert (fx.prob.init_gpu_used.max(axis=1) > per_dev).any()                      # gpu_overbooked
    fx = F.fixture("ephgcd_refresh")
    assert F.staging_gcds(fx.prob)[0] == F.EPH_G and int(fx.prob.alloc_eph.min()) > 1 << 32
    assert int(fx.prob.alloc_eph.max()) // F.EPH_G == F.LIM31 - 1


@pytest.mark.parametrize("res", ["eph", "scalar", "gpu"], ids=["ephemeral", "extended", "device_total"])
def test_range_edge_of_the_restated_domain(res):
    """a quotient of 2^31 - 1 is inside the domain of the mask rows, 2^31 is outside it; the two problems differ in that one value"""
    inside, outside = F.fixture(f"edge_{res}_inside"), F.fixture(f"edge_{res}_outside")
    assert F.check_domain(inside.prob) == [] and len(F.check_domain(outside.prob)) == 1
    field = {"eph": "alloc_eph", "scalar": "scalar_alloc", "gpu": "gpu_mem_total"}[res]
    a, b = getattr(inside.prob, field), getattr(outside.prob, field)
    if res == "gpu":                                            # the per-device total is what is staged
        a, b = a // np.maximum(inside.prob.gpu_cnt, 1), b // np.maximum(outside.prob.gpu_cnt, 1)
    assert int(a.max()) == F.LIM31 - 1 and int(b.max()) == F.LIM31 and int((a != b).sum()) == 1
    assert inside.expected.tolist() == outside.expected.tolist()

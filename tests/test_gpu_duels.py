"""Score duels (tests/duel_util.py) through every kernel route that shares the narrow arithmetic: LeastAllocated as
trunc(fma(-r, RN(100 RN(1 / cap)), 100 + 2^-33)) (la_term, la_term_f, la_term_t), BalancedAllocation on quotients from a stored reciprocal
with Markstein corrections (div_by_rcp, div_by_rcp1), and the class term floor(100 x / m) = (int)fma(100 x, 1 / m, 0.5 / m)
(class_term, class_term2, renormalise) -- on gcd-1 quantities up to 2^31 and raw scores up to 2^30 - 1, where a wrong bias
constant, a dropped correction step, a contraction or an int32 intermediate sends a duel's pod to the wrong node
(tests/test_duels_host.py proves that for every fixture, on the CPU).

Every case is (fixture, route): the result must equal the CPU oracle's, and the route must be the one meant -- simon_stats'
kernel_variant and kernel_generation, and what SIMON_DEBUG_ROUTE prints of it (unit, prologue, signature count).  Each route sets its
knobs itself, SIMON_LDS_WS included.  The all-feature kernel is the control: its class terms are int64 divisions (divq) and its
LeastAllocated an int64 quotient seeded by the fp64 fraction and corrected in integers (la_from_frac) -- but its BalancedAllocation is
div_by_rcp like the others', and its InterPodAffinity term, which these problems do not have, is fp64 on a stored reciprocal
(tests/test_gpu_term_duels.py).

Sizes: at most 200 nodes (the 100-duel problem: two nodes per duel; every other problem at most 120), 180 pods and 6 scenarios per case --
the full pool under four orders and two prefix scenarios that end behind a whole duel, so the shared initial image's prefix copy runs.
NodeAffinity / TaintToleration tables keep a problem off generations 1 and 2 (simon_hip.hip: route_batch, needs_table_or_wide): their
fixtures run on the score-table routes and the control.  Run with -m gpu on an MI355X."""
import functools
import re

import pytest

import duel_util as U
import oracle_lib as O
from open_simulator_amd import capi

pytestmark = pytest.mark.gpu

KNOBS = ("SIMON_NARROW_V1", "SIMON_NO_CACHE", "SIMON_RCP_DIV", "SIMON_WG", "SIMON_LDS_WS", "SIMON_TABLE_COARSE", "SIMON_FORCE_WIDE",
         "SIMON_NO_SHARED_PROLOGUE", "SIMON_NO_SIZE_DISPATCH", "SIMON_FORCE_TABLE", "SIMON_TABLE_NO_TWINS", "SIMON_TABLE_NO_CLASS_CONTENT")
NARROW, WIDE, FAST, TABLE = capi.KERNEL_NARROW, capi.KERNEL_WIDE, capi.KERNEL_NARROW_FAST, capi.KERNEL_NARROW_CACHE

# route -> (environment, kernel_variant, kernel_generation, what the `[route] unit` line must hold).  SIMON_NO_SIZE_DISPATCH shows in that line
# only for launches with two entries per lane (more than 1 024 padded positions: none of these problems), so its route is told by the
# statistics and the unit alone.
ROUTES = {
    "table_hbm": ({"SIMON_LDS_WS": "0"}, TABLE, 4, ("unit simon_table ", "prologue shared-image")),
    "table_ldsws": ({"SIMON_LDS_WS": "1"}, TABLE, 4, ("unit simon_table_lds ",)),
    "table_own_prologue": ({"SIMON_LDS_WS": "0", "SIMON_NO_SHARED_PROLOGUE": "1"}, TABLE, 4, ("unit simon_table ", "prologue per-scenario")),
    "table_coarse": ({"SIMON_LDS_WS": "0", "SIMON_TABLE_COARSE": "1"}, TABLE, 5, ("unit simon_table ", "prologue per-scenario")),
    "table_one_size": ({"SIMON_LDS_WS": "0", "SIMON_NO_SIZE_DISPATCH": "1"}, TABLE, 4, ("unit simon_table ", "prologue shared-image")),
    "generation2": ({"SIMON_NO_CACHE": "1"}, FAST, 2, ()),
    "generation1_div": ({"SIMON_NARROW_V1": "1", "SIMON_RCP_DIV": "0"}, NARROW, 1, ()),
    "generation1_rcp": ({"SIMON_NARROW_V1": "1", "SIMON_RCP_DIV": "1"}, NARROW, 1, ()),
    "wide": ({"SIMON_FORCE_WIDE": "1"}, WIDE, 0, ()),
}
TABLE_ROUTES = [r for r in ROUTES if r.startswith("table_")]
# fixture -> signatures the score table must report (the 100-signature problem keeps two per lane: KQ = 2)
N_SIGS = {"laba60_initial": 60, "laba60_refresh": 60, "laba60_nz": 60, "laba100_two_per_shape": 100, "simon16": 16, "na16": 16, "tt16": 16}
CASES = [(fx, r) for fx in N_SIGS for r in ROUTES if r in TABLE_ROUTES or r == "wide" or not U.FIXTURES[fx][1][0].startswith(("na_", "tt_"))]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the oracle's result of a fixture: once, shared by its routes, never modified"""
    fx = U.fixture(name)
    ref = O.run(fx.prob, fx.scen, fx.orders)
    full = fx.scen[:, 0] == fx.prob.n_nodes
    assert (ref.placement[full] == fx.expected).all() and ref.unscheduled.tolist() == [0] * len(fx.scen)
    return fx, ref


def _run(fx, env, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SIMON_DEBUG_ROUTE", "1")
    with capi.Context(0) as ctx:
        ctx.load_problem(fx.prob)
        ctx.load_scenarios(fx.scen, fx.orders)
        ctx.run_loaded(True)
        st = ctx.stats()
        return ctx.fetch(True), (st.kernel_variant, st.kernel_generation)


def _assert_same(res, ref, fx):
    bad = (res.placement != ref.placement).nonzero()
    if len(bad[0]):
        s, p = int(bad[0][0]), int(bad[1][0])
        per = fx.prob.n_pods // len(fx.duels)
        pytest.fail(f"{len(bad[0])} placements differ; first: scenario {s} pod {p} (duel {p // per}, kind {fx.duels[p // per].kind}): "
                    f"{res.placement[s, p]} for {ref.placement[s, p]}")
    assert res.unscheduled.tolist() == ref.unscheduled.tolist()
    assert res.used_cpu.tolist() == ref.used_cpu.tolist() and res.used_mem.tolist() == ref.used_mem.tolist()


@pytest.mark.parametrize("name,route", CASES, ids=[f"{fx}-{r}" for fx, r in CASES])
def test_duels(name, route, monkeypatch, capfd):
    fx, ref = _reference(name)
    env, variant, generation, unit_line = ROUTES[route]
    res, got = _run(fx, env, monkeypatch)
    err = capfd.readouterr().err
    print(err)
    assert got == (variant, generation), err
    if variant == TABLE:
        line = [l for l in err.splitlines() if l.startswith("[route] variant")][-1]
        assert int(re.search(r"n_sigs (\d+)", line).group(1)) == N_SIGS[name], line
        nzeq = 0 if name.endswith("_nz") else 1
        unit = [l for l in err.splitlines() if l.startswith("[route] unit")][-1]
        for want in unit_line + (f"nzeq {nzeq} ",):
            assert want in unit, unit
    _assert_same(res, ref, fx)


@pytest.mark.parametrize("name,variant,generation", [("edge_inside", TABLE, 4), ("edge_outside", WIDE, 0)])
def test_range_edge_of_the_narrow_route(name, variant, generation, monkeypatch, capfd):
    """largest node + all pods == 2^31 - 1 cpu units: the score table; one unit more: the all-feature kernel.  Both equal the oracle."""
    fx, ref = _reference(name)
    assert U.route_bound(fx.prob) == (1 << 31) - (1 if name == "edge_inside" else 0)
    res, got = _run(fx, {"SIMON_LDS_WS": "0"}, monkeypatch)
    print(capfd.readouterr().err)
    assert got == (variant, generation)
    _assert_same(res, ref, fx)

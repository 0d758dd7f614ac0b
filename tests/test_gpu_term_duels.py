"""Score duels on the two float normalisations (tests/term_duel_util.py) through every kernel path that computes them:
InterPodAffinity's int64(100.0 * (float64(raw - min) / float64(max - min))) -- the all-feature kernel's 100.0 * div_by_rcp(x - min, diff,
1 / diff) on raw scores cached in LDS and gathered again (SIMON_WIDE_NO_CACHE_B), generation 7's true division in spread_select's
tabulated path and in its general walk, both once more with 65 .. 128 node classes (CN2) and in team mode (team_extremes) -- and
PodTopologySpread's 100 (max + min - raw) / max -- divq_r there, (int)fma(100 y, 1 / max, 0.5 / max) here.  A dropped correction step, a
dropped bias, an integer division for the float one, a rounding conversion or extremes not taken from 0 send a duel's pod to the wrong
node (tests/test_term_duels_host.py proves that for every fixture, on the CPU).

Every case is (fixture, route): the result must equal the CPU oracle's (placements, unscheduled, used cpu / memory), and the route must be
the one meant -- simon_stats' kernel_variant, kernel_generation and workgroup_size (64: one wave per scenario, 256: a team of four), and
the internal node classes that SIMON_DEBUG_ROUTE's `[route] variant` line reports against term_duel_util.route_facts.  Which of
spread_select's two paths a pod takes is decided per pod inside the kernel and cannot be seen from outside: the fixtures are built for
one or the other, and tests/test_term_duels_host.py checks the predicates (`simple`, classes << lg <= SIMON_SPREAD_TAB_MAX) on them.
Fixtures in the general form (several preferred terms and owner weights per class, negative weights) run on the all-feature kernel only.

Sizes: at most 16 duels, 130 nodes, 1 500 pods and 6 scenarios per case.  Run with -m gpu on an MI355X."""
import functools
import re

import numpy as np
import pytest

import oracle_lib as O
import term_duel_util as T
from open_simulator_amd import capi

pytestmark = pytest.mark.gpu

KNOBS = ("SIMON_NARROW_V1", "SIMON_NO_CACHE", "SIMON_RCP_DIV", "SIMON_WG", "SIMON_LDS_WS", "SIMON_TABLE_COARSE", "SIMON_FORCE_WIDE",
         "SIMON_NO_SHARED_PROLOGUE", "SIMON_NO_SIZE_DISPATCH", "SIMON_FORCE_TABLE", "SIMON_TABLE_NO_TWINS", "SIMON_TABLE_NO_CLASS_CONTENT",
         "SIMON_TEAM", "SIMON_TEAM_MAX_S", "SIMON_NO_SPREAD", "SIMON_NO_IPA_FOLD", "SIMON_NO_HARD_FOLD", "SIMON_NO_FOLD", "SIMON_NO_RS", "SIMON_NO_REST",
         "SIMON_NO_CN2", "SIMON_WIDE_NO_CACHE_B")
WIDE, TABLE = capi.KERNEL_WIDE, capi.KERNEL_NARROW_CACHE

# route -> (environment, kernel_variant, kernel_generation, workgroup_size where it tells routes apart)
ROUTES = {
    "wide_cached": ({"SIMON_FORCE_WIDE": "1"}, WIDE, 0, None),
    "wide_regather": ({"SIMON_FORCE_WIDE": "1", "SIMON_WIDE_NO_CACHE_B": "3"}, WIDE, 0, None),
    "gen7_wave": ({"SIMON_TEAM": "0"}, TABLE, 7, 64),
    "gen7_team": ({"SIMON_TEAM": "1"}, TABLE, 7, 256),
    "gen7_cn2": ({}, TABLE, 7, None),                # the library's own choice for a batch of 6 scenarios; 65 .. 128 classes asserted below
}
WIDE_ROUTES = ("wide_cached", "wide_regather")
CASES = [(fx, r) for fx, spec in T.FIXTURES.items() for r in ROUTES
         if (r in WIDE_ROUTES or spec[3].get("form", "self") == "self") and (r != "gen7_cn2" or fx == "cn2")]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the oracle's result of a fixture: once, shared by its routes, never modified"""
    fx = T.fixture(name)
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
        return ctx.fetch(True), (st.kernel_variant, st.kernel_generation, st.workgroup_size)


def _assert_same(res, ref, fx):
    bad = (res.placement != ref.placement).nonzero()
    if len(bad[0]):
        starts = np.concatenate([[0], np.cumsum([len(d.nodes) for d in fx.duels])])
        lines = []
        for s, p in list(zip(bad[0].tolist(), bad[1].tolist()))[:8]:
            d = int(fx.pod_duel[p])
            lines.append(f"scenario {s} pod {p}: duel {d} ({T.describe(fx.duels[d])}; its nodes start at {starts[d]}): "
                         f"node {res.placement[s, p]} for {ref.placement[s, p]}")
        pytest.fail(f"{fx.name}: {len(bad[0])} placements differ\n" + "\n".join(lines))
    assert res.unscheduled.tolist() == ref.unscheduled.tolist()
    assert res.used_cpu.tolist() == ref.used_cpu.tolist() and res.used_mem.tolist() == ref.used_mem.tolist()


@pytest.mark.parametrize("name,route", CASES, ids=[f"{fx}-{r}" for fx, r in CASES])
def test_term_duels(name, route, monkeypatch, capfd):
    fx, ref = _reference(name)
    assert len(fx.scen) <= 6
    env, variant, generation, wg = ROUTES[route]
    res, got = _run(fx, env, monkeypatch)
    err = capfd.readouterr().err
    print(err)
    assert got[:2] == (variant, generation), (got, err)
    if wg is not None:
        assert got[2] == wg, (got, err)
    if variant == TABLE:
        line = [l for l in err.splitlines() if l.startswith("[route] variant")][-1]
        facts = T.route_facts(fx)
        assert int(re.search(r"Cn_t (\d+)", line).group(1)) == facts["classes"], line
        assert (facts["classes"] > 64) == (name == "cn2")
        assert " spread 1 " in line, line
    _assert_same(res, ref, fx)


def test_the_general_form_stays_off_generation_7(monkeypatch, capfd):
    """two hostname-like rows per class / owners of one term with different weights: spread_supported refuses, without any knob"""
    fx, ref = _reference("ipa_general")
    res, got = _run(fx, {}, monkeypatch)
    print(capfd.readouterr().err)
    assert got[:2] == (WIDE, 0), got
    _assert_same(res, ref, fx)

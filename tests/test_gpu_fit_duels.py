"""Fit duels (tests/fit_duel_util.py) through every kernel route that holds the 32-bit arithmetic of the score table's mask rows:
xres_fits_t (`alloc < req + used` in unsigned, the sum up to 2^32 - 2), gpu_fits_t and gpu_commit_t (signed `tot - used`, per-device
slices, tightest fit) in the REST prologue, in rest_assume_store and in the GPU fold's refresh, behind stage_narrow's uint32 staging on
the gcds of rest_supported / gfold_supported (simon_hip.hip) -- on quantities up to 2^31 - 1, where a signed sum, a trip through fp32, `>`
for `>=`, an unsigned difference, pooled device memory, first fit or a lost gcd sends a duel's pod to the wrong node
(tests/test_fit_duels_host.py proves that for every fixture, on the CPU).  The all-feature kernel (int64 arithmetic) is the control.

Every case is (fixture, route): placements, unscheduled counts, used cpu and memory, and gpu_slices where the fixture books devices must
equal the CPU oracle's, and the route must be the one meant -- simon_stats' kernel_variant and kernel_generation, `rest 1` / `gfold 1` in the
`[route] variant` line and the unit in the `[route] unit` line that SIMON_DEBUG_ROUTE prints.  Each route deletes every knob and sets its own.

Sizes: at most 73 nodes, 73 pods and 6 scenarios per case (the full pool under four orders, two prefix scenarios that end behind a whole
duel).  Six scenarios are at most one per CU, so the mask rows live in LDS unless SIMON_LDS_WS=0 says no, and generation 7 would run teams
of four waves: SIMON_TEAM=0 keeps the walks on the one-wave unit (SIMON_TEAM=1, the teams, is a route of its own).  The GPU fold has no
LDS home today (route_batch keeps LDSWS for generation 4 without folds), so gpu_fold and gpu_fold_hbm launch alike; the second stays for the
day that changes.  Nothing here has a tolerance.  Run with -m gpu on an MI355X."""
import functools

import pytest

import fit_duel_util as F
import oracle_lib as O
from open_simulator_amd import capi

pytestmark = pytest.mark.gpu

KNOBS = ("SIMON_NARROW_V1", "SIMON_NO_CACHE", "SIMON_RCP_DIV", "SIMON_WG", "SIMON_LDS_WS", "SIMON_TABLE_COARSE", "SIMON_FORCE_WIDE", "SIMON_NO_SHARED_PROLOGUE",
         "SIMON_NO_SIZE_DISPATCH", "SIMON_FORCE_TABLE", "SIMON_TABLE_NO_TWINS", "SIMON_TABLE_NO_CLASS_CONTENT", "SIMON_NO_GPU_FOLD", "SIMON_NO_REST", "SIMON_NO_FOLD",
         "SIMON_NO_RS", "SIMON_NO_SPREAD", "SIMON_NO_CN2", "SIMON_TEAM", "SIMON_TEAM_MAX_S", "SIMON_TABLE_NO_GPU_SPLIT")
WIDE, TABLE = capi.KERNEL_WIDE, capi.KERNEL_NARROW_CACHE

# route -> (environment, kernel_variant, kernel_generation, what the `[route] variant` line must hold, what the `[route] unit` line must hold)
ROUTES = {
    "rows_hbm": ({"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "0"}, TABLE, 6, "rest 1 ", "unit simon_table_rest "),
    "rows_lds": ({"SIMON_NO_GPU_FOLD": "1"}, TABLE, 6, "rest 1 ", "unit simon_table_restlds "),
    "two_classes_per_lane": ({"SIMON_NO_GPU_FOLD": "1"}, TABLE, 6, "rest 1 ", "unit simon_table_rest2 "),
    "walks": ({"SIMON_NO_GPU_FOLD": "1", "SIMON_TEAM": "0"}, TABLE, 7, "rest 1 ", "unit simon_table_rs "),
    "walks_team": ({"SIMON_NO_GPU_FOLD": "1", "SIMON_TEAM": "1"}, TABLE, 7, "rest 1 ", "unit simon_table_team4 "),
    "gpu_fold": ({}, TABLE, 5, "gfold 1 ", "unit simon_table "),
    "gpu_fold_hbm": ({"SIMON_LDS_WS": "0"}, TABLE, 5, "gfold 1 ", "unit simon_table "),
    "wide": ({"SIMON_FORCE_WIDE": "1"}, WIDE, 0, None, None),
}


def _routes_of(name):
    if name.endswith("_70classes"):
        return ("two_classes_per_lane", "wide")
    if name.endswith("_spread"):
        return ("walks", "walks_team", "wide")
    fold = ("gpu_fold", "gpu_fold_hbm") if name in ("gpu_initial", "gpu_refresh") else ()
    return ("rows_hbm", "rows_lds") + fold + ("wide",)


CASES = [(fx, r) for fx in F.DUEL_FIXTURES for r in _routes_of(fx)]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the oracle's result of a fixture: once, shared by its routes, never modified"""
    fx = F.fixture(name)
    ref = O.run(fx.prob, fx.scen, fx.orders, want_gpu_slices=fx.ft.gpu)
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
        ctx.run_loaded(True, fx.ft.gpu)
        st = ctx.stats()
        return ctx.fetch(True, fx.ft.gpu), (st.kernel_variant, st.kernel_generation)


def _assert_same(res, ref, fx):
    duel_of = [d for d in range(len(fx.duels)) for _ in fx.duel_pods(d)]
    bad = (res.placement != ref.placement).nonzero()
    if len(bad[0]):
        s, p = int(bad[0][0]), int(bad[1][0])
        pytest.fail(f"{len(bad[0])} placements differ; first: scenario {s} pod {p} (duel {duel_of[p]}, kind {fx.duels[duel_of[p]].kind}, "
                    f"{fx.duels[duel_of[p]].pods[p - fx.pod0[duel_of[p]]].role}): {res.placement[s, p]} for {ref.placement[s, p]}")
    assert res.unscheduled.tolist() == ref.unscheduled.tolist()
    assert res.used_cpu.tolist() == ref.used_cpu.tolist() and res.used_mem.tolist() == ref.used_mem.tolist()
    if fx.ft.gpu:
        bad = (res.gpu_slices != ref.gpu_slices).nonzero()
        if len(bad[0]):
            s, p = int(bad[0][0]), int(bad[1][0])
            pytest.fail(f"{len(bad[0])} device bookings differ; first: scenario {s} pod {p} (duel {duel_of[p]}, kind {fx.duels[duel_of[p]].kind}): "
                        f"{int(res.gpu_slices[s, p]):#x} for {int(ref.gpu_slices[s, p]):#x}")


def _line(err, head):
    return [l for l in err.splitlines() if l.startswith(head)][-1]


@pytest.mark.parametrize("name,route", CASES, ids=[f"{fx}-{r}" for fx, r in CASES])
def test_fit_duels(name, route, monkeypatch, capfd):
    fx, ref = _reference(name)
    env, variant, generation, in_variant, in_unit = ROUTES[route]
    res, got = _run(fx, env, monkeypatch)
    err = capfd.readouterr().err
    print(err)
    assert got == (variant, generation), err
    if variant == TABLE:
        assert in_variant in _line(err, "[route] variant"), err
        assert in_unit in _line(err, "[route] unit"), err
    _assert_same(res, ref, fx)


@pytest.mark.parametrize("res", ["eph", "scalar", "gpu"], ids=["ephemeral", "extended", "device_total"])
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_range_edge_of_the_mask_rows(res, side, monkeypatch, capfd):
    """the largest quotient is 2^31 - 1: generation 6; the same problem with one unit more: the mask rows are refused and the all-feature
    kernel runs.  Both equal the oracle."""
    fx, ref = _reference(f"edge_{res}_{side}")
    assert len(F.check_domain(fx.prob)) == (side == "outside")
    out, got = _run(fx, {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "0"}, monkeypatch)
    err = capfd.readouterr().err
    print(err)
    assert got == ((TABLE, 6) if side == "inside" else (WIDE, 0)), err
    assert ("[route] mask rows refused" in err) == (side == "outside"), err
    if side == "inside":
        assert "rest 1 " in _line(err, "[route] variant") and "unit simon_table_rest " in _line(err, "[route] unit"), err
    _assert_same(out, ref, fx)

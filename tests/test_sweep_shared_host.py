"""The pieces the four sweeps share on the host (no GPU): the occupancy-row builder and its two ways to total a scenario's allocatable
against the definition written as a plain loop, the carrier of the five usage results, and one batched-against-one-by-one case per sweep."""
import dataclasses
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest

import explain_own_util as OU
import local_usage_util as LU
import mix_util as MU
import test_usage_host as TU
from open_simulator_amd import capi, simulate as sim

N = 37


def _problem(rng, local=True):
    """Node arrays only: allocatable memory near 2^40 (a float32 or int32 path shows), volume groups on some nodes, none on others."""
    cnt = rng.integers(0, capi.MAX_VG + 1, N)
    cnt[:3] = 0                                                      # (the first nodes carry no volume group: a capacity of 0)
    return NS(alloc_cpu=rng.integers(1000, 256000, N).astype(np.int64), alloc_mem=(1 << 40) - rng.integers(0, 1 << 20, N).astype(np.int64),
              local_flags=np.ones(N, np.uint8) if local else None, local_vg_cnt=cnt.astype(np.int32) if local else None,
              local_vg_cap=rng.integers(1, 1 << 42, (N, capi.MAX_VG)).astype(np.int64) if local else None)


def _result(rng, pr, held, local=True):
    """An engine result whose used sums are fractions of what the scenario's nodes hold (some scenarios leave pods, some are at risk)."""
    S = len(held)
    tot = lambda v: np.array([sum(int(x) for x in np.asarray(v)[h]) for h in held], np.int64)                # noqa: E731
    vg = tot([sum(int(pr.local_vg_cap[j][v]) for v in range(int(pr.local_vg_cnt[j]))) for j in range(N)]) if local else None
    return NS(unscheduled=rng.integers(0, 3, S).astype(np.int32), used_cpu=tot(pr.alloc_cpu) * rng.integers(0, 101, S) // 100,
              used_mem=tot(pr.alloc_mem) * rng.integers(0, 101, S) // 100, used_vg=vg * rng.integers(0, 101, S) // 100 if local else None,
              preempt_risk=rng.integers(0, 2, S).astype(np.uint8))


def _rows_by_definition(pr, out, held):
    rows = []
    for s, h in enumerate(held):
        cpu = mem = vg = 0
        for j in np.flatnonzero(h).tolist():
            cpu += int(pr.alloc_cpu[j])
            mem += int(pr.alloc_mem[j])
            if pr.local_flags is not None:
                vg += sum(int(pr.local_vg_cap[j][v]) for v in range(int(pr.local_vg_cnt[j])))
        rows.append((int(out.unscheduled[s]), sim.occupancy_pct(int(out.used_cpu[s]), cpu), sim.occupancy_pct(int(out.used_mem[s]) * 1000, mem * 1000),
                     sim.occupancy_pct(int(out.used_vg[s]), vg) if pr.local_flags is not None and out.used_vg is not None else 0,
                     bool(out.preempt_risk[s])))
    return rows


def _prefixes():
    sizes = np.array([1, 2, 3, 4, 17, N - 1, N], np.int32)
    return sizes, np.arange(N)[None, :] < sizes[:, None]


def _subsets(rng):
    held = rng.random((24, N)) < 0.4
    held[0] = False
    held[0, :3] = True                                               # only nodes without a volume group
    held[1] = True
    held[np.arange(len(held)), rng.integers(0, N, len(held))] |= ~held.any(1)
    return held


@pytest.mark.parametrize("local", [True, False])
def test_rows_of_prefix_scenarios_are_the_plain_loop_s(local):
    rng = np.random.default_rng(11)
    pr = _problem(rng, local)
    sizes, held = _prefixes()
    out = _result(rng, pr, held, local)
    rows = sim._scenario_rows(out, *sim._alloc_of_prefixes(pr, out, sizes))
    assert rows == _rows_by_definition(pr, out, held)
    assert all(type(v) in (int, bool) for r in rows for v in r)
    if local:
        assert [r[3] for r in rows[:3]] == [0, 0, 0] and any(r[3] > 0 for r in rows)        # no capacity: pct 0, never a division
    else:
        assert [r[3] for r in rows] == [0] * len(rows)
    assert any(r[2] > 0 for r in rows) and any(r[4] for r in rows) and not all(r[4] for r in rows)


@pytest.mark.parametrize("local", [True, False])
def test_rows_of_arbitrary_subsets_are_the_plain_loop_s(local):
    rng = np.random.default_rng(12)
    pr = _problem(rng, local)
    held = _subsets(rng)
    out = _result(rng, pr, held, local)
    rows = sim._scenario_rows(out, *sim._alloc_of_subsets(pr, out, held))
    assert rows == _rows_by_definition(pr, out, held)
    assert rows[0][3] == 0 and ((not local) or any(r[3] > 0 for r in rows))


def test_used_vg_missing_gives_a_vg_column_of_zeros():
    rng = np.random.default_rng(13)
    pr = _problem(rng)
    sizes, held = _prefixes()
    out = _result(rng, pr, held)
    out.used_vg = None
    assert sim._vg_caps(pr, out) is None
    assert [r[3] for r in sim._scenario_rows(out, *sim._alloc_of_subsets(pr, out, held))] == [0] * len(held)


def test_the_two_totals_agree_on_prefix_masks_and_stay_int64():
    rng = np.random.default_rng(14)
    pr = _problem(rng)
    pr.alloc_cpu = pr.alloc_cpu.astype(np.int32)                      # (a narrow input must not narrow the sums)
    sizes, held = _prefixes()
    out = NS(used_vg=np.zeros(len(sizes), np.int64))
    a, b = sim._alloc_of_prefixes(pr, out, sizes), sim._alloc_of_subsets(pr, out, held)
    for x, y in zip(a, b):
        assert x.dtype == np.int64 and y.dtype == np.int64 and x.tolist() == y.tolist()
    assert int(a[1][-1]) == sum(int(v) for v in pr.alloc_mem) > 1 << 45
    # sweep_mix's scenarios: the fixed nodes and a prefix of every segment, the cumulative sum's prefix differences against held @ v
    fixed, seg_start, top = 5, np.array([5, 16], np.int32), [11, N - 16]
    cnt = np.array([(x, y) for x in (0, 1, 11) for y in (0, 7, N - 16)], np.int32)
    held = np.zeros((len(cnt), N), bool)
    held[:, :fixed] = True
    for g, st in enumerate(seg_start.tolist()):
        held[:, st:st + top[g]] = np.arange(top[g])[None, :] < cnt[:, g:g + 1]
    out = NS(used_vg=np.zeros(len(cnt), np.int64))
    for x, y in zip(sim._alloc_of_prefixes(pr, out, np.full(len(cnt), fixed), (seg_start, cnt)), sim._alloc_of_subsets(pr, out, held)):
        assert x.dtype == np.int64 and x.tolist() == y.tolist()
    pr.local_flags = None
    assert sim._alloc_of_prefixes(pr, out, sizes)[2] is None and sim._alloc_of_subsets(pr, out, held)[2] is None


# ---- the carrier of the five usage results ------------------------------------------------------------------------------------------

def _exact_by_definition(rows):
    """headroom_exact over scenarios that ran as their own problems: exact where every one of them says so (None: no probes)."""
    rows = [r for r in rows if r is not None]
    return [all(r[k] for r in rows) for k in range(len(rows[0]))] if rows else None


def _fields(u):
    return u.onto(NS())


def test_one_scenario_tuples_become_lists_and_the_and_of_the_exact_flags():
    each = [([3, 0], [True, True], [{"node": "a"}], None, [{"node": "a", "kind": "VG"}]),
            ([1, 2], [True, False], [{"node": "a"}, {"node": "b"}], None, []),
            ([0, 0], [True, True], [], None, [])]
    u = sim._Usage([("ns", "p"), ("ns", "q")], node_table=True, storage=True)
    for five in each:
        u.take(five, launch=False)
    res = _fields(u)
    assert res.headroom == [e[0] for e in each] and res.node_table == [e[2] for e in each] and res.storage_table == [e[4] for e in each]
    assert res.gpu_table is None
    assert res.headroom_exact == _exact_by_definition([e[1] for e in each]) == [True, False]
    # tables without probes: lists, and no flags
    u = sim._Usage(None, devices=True)
    for five in [(None, None, None, [{"node": "g"}], None), (None, None, None, [], None)]:
        u.take(five, launch=False)
    res = _fields(u)
    assert (res.headroom, res.headroom_exact, res.node_table, res.gpu_table, res.storage_table) == (None, None, None, [[{"node": "g"}], []], None)
    assert u.asked


def test_nothing_asked_for_leaves_every_field_none():
    u = sim._Usage(None)
    assert not u.asked
    for _ in range(3):
        u.take((None, None, None, None, None), launch=False)
    u.take((None, None, None, None, None), launch=True)
    res = _fields(u)
    assert (res.headroom, res.headroom_exact, res.node_table, res.gpu_table, res.storage_table) == (None,) * 5
    assert _exact_by_definition([None] * 3) is None


def test_launch_lists_concatenate_in_order_and_the_last_launch_s_flags_stand():
    u = sim._Usage([0], node_table=True, devices=True)
    u.take(([[1], [2]], [True], [["t0"], ["t1"]], [["g0"], ["g1"]], None), launch=True)
    u.take(([[3]], [False], [["t2"]], [["g2"]], None), launch=True)
    res = _fields(u)
    assert res.headroom == [[1], [2], [3]] and res.node_table == [["t0"], ["t1"], ["t2"]] and res.gpu_table == [["g0"], ["g1"], ["g2"]]
    assert res.headroom_exact == [False] and res.storage_table is None
    nested = u.onto(NS(), K=3)                                        # sweep_apps: [U][K]
    assert nested.headroom == [[[1], [2], [3]]] and nested.gpu_table == [[["g0"], ["g1"], ["g2"]]] and nested.headroom_exact == [False]


# ---- both roads of every sweep --------------------------------------------------------------------------------------------------------

ON = dict(reasons=True, node_table=True)


def _simple():
    cluster, apps, types = TU._simple_without_app_daemonset()        # (no app DaemonSet: every scenario's own stream is the pool's)
    return cluster, apps, types, TU._app_refs(cluster, apps)


def _agree(a, b, skip=("batched", "fallback")):
    assert type(a) is type(b)
    for f in dataclasses.fields(a):
        if f.name not in skip:
            assert getattr(a, f.name) == getattr(b, f.name), f.name
    return True


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


def test_sweep_batched_and_size_by_size_agree():
    cluster, apps, types, refs = _simple()
    counts = [0, 1, 4, 6]                                             # (4 new nodes schedule every pod; the cap asks for 6)
    a = _quiet(lambda: sim.sweep(cluster, apps, types[0], counts, engine=MU.OracleEngine(), headroom=refs, max_cpu=9, **ON))
    b = _quiet(lambda: sim._sweep_per_size(cluster, apps, types[0], counts, MU.OracleEngine(), 9, 100, 100, True, refs, True))
    assert _agree(a, b) and a.best == 6 and a.result is not None and any(a.unscheduled_pods) and a.headroom_exact is not None


def test_sweep_mix_batched_and_mix_by_mix_agree():
    cluster, apps, types, refs = _simple()
    grid = [[0, 2, 4], [0, 3]]
    a = _quiet(lambda: sim.sweep_mix(cluster, apps, types, grid, costs=[3, 2], engine=OU.OwnSegmentOracleEngine(), headroom=refs, **ON))
    b = _quiet(lambda: sim.sweep_mix(cluster, apps, types, grid, costs=[3, 2], engine=MU.OracleEngine(), headroom=refs, **ON))
    assert a.batched and not b.batched and b.fallback and a.fallback is None
    assert _agree(a, b) and a.result is not None and any(a.unscheduled_pods)


def test_sweep_failures_batched_and_scenario_by_scenario_agree():
    cluster, apps, types, refs = _simple()
    a = _quiet(lambda: sim.sweep_failures(cluster, apps, "node", engine=LU.LocalUsageOracleEngine(), headroom=refs, max_cpu=80, **ON))
    b = _quiet(lambda: sim.sweep_failures(cluster, apps, "node", engine=MU.OracleEngine(), headroom=refs, max_cpu=80, **ON))
    assert a.batched and not b.batched
    # `rows` holds each road's own problem (the pool's, or the reduced cluster's): what they place is compared by object names
    assert _agree(a, b, skip=("batched", "fallback", "rows")) and a.placements == b.placements and any(a.unscheduled_pods)


def test_sweep_apps_batched_and_scenario_by_scenario_agree():
    cluster, apps, types, refs = _simple()
    split = [sim.AppResource(f"{k.lower()}-{o['metadata']['name']}", {k: [o]}) for a in apps for k, v in a.resource.items()
             if k in ("Deployment", "StatefulSet", "ReplicaSet", "Job") for o in v][:3]
    prefs = TU._app_refs(cluster, split[:1], 1)                       # a probe of the first app: named in every subset below
    subsets = [[a.name for a in split], [split[0].name], [split[0].name, split[2].name]]
    kw = dict(subsets=subsets, new_node=types[0], counts=[0, 2], headroom=prefs, **ON)
    a = _quiet(lambda: sim.sweep_apps(cluster, split, engine=LU.LocalUsageOracleEngine(), **kw))
    b = _quiet(lambda: sim.sweep_apps(cluster, split, engine=MU.OracleEngine(), **kw))
    assert a.batched and not b.batched
    assert _agree(a, b) and np.asarray(a.headroom).shape == (3, 2, 1)

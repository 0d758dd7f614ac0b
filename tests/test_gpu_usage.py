"""Per-node usage and headroom on the device (simon_fetch_node_usage, simon_fetch_headroom): both calls against the numpy restatement
(usage_util) of the placements the device itself fetched, and those placements against the unmodified oracle -- on every kernel route,
for every kind of batch, on pools around the 64-node tile edge with the tile unset and forced to 64 nodes; headroom end to end against
the oracle (appended probes); every refusal; the sweeps on HipEngine against the oracle-backed engine.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import evict_util as EU
import mix_util as MU
import oracle_lib as O
import podset_util as PU
import randprob
import subset_util as SU
import usage_util as UU
from open_simulator_amd import capi, simulate as sim

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 130]
KINDS = ["prefix", "ranked", "segmented", "subset", "subset_evict", "podset", "own_podset"]
TILES = [None, 64]                         # SIMON_USAGE_TILE unset / 64: at N = 65 and 130 a tile edge inside the pool, a last tile of 1 or 2 nodes


def _tile(monkeypatch, tile):
    """The knob is read once, when the context is made."""
    if tile is None:
        monkeypatch.delenv("SIMON_USAGE_TILE", raising=False)
    else:
        monkeypatch.setenv("SIMON_USAGE_TILE", str(tile))


def _scen_of(mask, order_ids):
    return np.stack([np.asarray(mask, bool).sum(1), order_ids], 1).astype(np.int32)


def _probe_pods(prob, n=8):
    """n probe pods: exact ones first (one per class), then pinned / preset / other pods, so that both values of `exact` occur."""
    exact = [p for p in range(prob.n_pods) if UU.probe_exact(prob, p)]
    seen, out = set(), []
    for p in exact:
        if int(prob.pod_class[p]) not in seen:
            seen.add(int(prob.pod_class[p]))
            out.append(p)
    rest = [p for p in range(prob.n_pods) if not UU.probe_exact(prob, p)]
    return (out[:n - 2] + rest[:2] + out[n - 2:])[:n]


@functools.lru_cache(maxsize=None)
def _batch(kind, N, extras=False):
    """One batch of `kind` over a pool of N nodes, P = 300: (problem, scen, orders, setup(ctx) -> None, held bool [S][N], oracle placement
    rows [S][P]).  extras: ephemeral storage, K = 2 scalars, state before the stream and zero-quantity scalar entries (prefix only)."""
    seed = 7 * N + KINDS.index(kind)
    rng = np.random.default_rng(seed)
    P, S = 300, 8
    kw = dict(N=N, P=P, gates=True, pins=True, nz_differs=True, static_mask=True, tight_pods=N >= 63, n_node_classes=min(5, N))
    if kind == "prefix":
        prob = randprob.rand_problem(seed, presets=True, init_state=True, **(dict(eph=True, scalars=2) if extras else {}), **kw)
        if extras:
            ent = ((rng.random(P) < 0.2) * rng.integers(1, 4, P)).astype(np.uint8)
            prob = EU.replaced(prob, scalar_entries=ent)
    else:
        prob, _ = MU.segmentable(randprob.rand_problem(seed, presets=True, **kw), fixed=0)
    orders = np.stack([np.arange(P), rng.permutation(P)]).astype(np.int32)
    oid = rng.integers(0, 2, S)
    sizes = np.unique(np.concatenate([[N, max(1, N - 1), max(1, N // 2)], rng.integers(1, N + 1, S)]))[::-1][:S]
    sizes = np.resize(sizes, S)
    prefix = np.arange(N)[None, :] < sizes[:, None]
    zone = rng.integers(0, 3, N).astype(np.int32)
    evict = None
    if kind in ("prefix", "podset"):
        held, setup, ranks = prefix, (lambda ctx: None), None
    elif kind == "ranked":
        held, ranks = prefix, SU.zone_ranks(prefix, zone)
        setup = lambda ctx: ctx.set_node_ranks(np.where(ranks < 0, 0, ranks))                            # noqa: E731
    elif kind == "segmented":
        F = N // 3
        starts = np.array([F, F + (N - F) // 2], np.int32)
        room = [int(starts[1] - starts[0]), int(N - starts[1])]
        cnt = np.stack([rng.integers(0, r + 1, S) for r in room], 1).astype(np.int32)
        cnt[0] = room                                                                                  # the whole pool
        if F == 0:
            cnt[cnt.sum(1) == 0] = room                                                                # (a scenario holds one node at least)
        held, ranks = np.stack([MU.present_mask(N, starts, cnt[s]) for s in range(S)]), None
        setup = lambda ctx: ctx.set_scenario_segments(starts, cnt)                                      # noqa: E731
    else:
        held = SU.staging_masks(N, zone, seed)[:S] if kind != "own_podset" else SU.staging_masks(N, zone, seed)[4:4 + S]
        S = len(held)
        oid = oid[:S]
        ranks = SU.zone_ranks(held, zone)
        if kind == "subset_evict":
            ok = EU.eligible(prob)
            prob, evict = EU.flag(prob, {int(ok[i]): int(j) for i, j in enumerate(rng.integers(0, N, 6))})
        setup = lambda ctx: ctx.set_scenario_nodes(held, zone)                                          # noqa: E731
    scen = _scen_of(held, oid[:len(held)])
    rows = None
    if kind in ("podset", "own_podset"):
        rows = rng.random((len(held), P)) < 0.6
        rows[0] = True
        rows[1] = False                                                                                # a scenario holding no pod
    want = []
    for s in range(len(held)):
        order = orders[scen[s, 1]]
        if rows is not None:
            one = PU.oracle_prefix(prob, rows[s], int(scen[s, 0]), order) if kind == "podset" else PU.oracle_nodes(prob, rows[s], held[s], order, ranks[s])
            want.append(one.placement)
        elif evict is not None:
            want.append(EU.oracle_rows(prob, evict, held[s:s + 1], scen[s:s + 1], orders, ranks[s:s + 1])[0][0])
        elif kind == "prefix":
            want.append(O.run(prob, scen[s:s + 1], orders).placement[0])
        else:
            want.append(MU.oracle_of_scenario(prob, held[s], order, None if ranks is None else ranks[s])[0])
    return prob, scen, orders, setup, held, np.stack(want), rows, evict


def _load(ctx, batch):
    prob, scen, orders, setup, held, want, rows, evict = batch
    ctx.load_problem(prob)
    if evict is not None:
        ctx.set_pod_eviction(evict)
    ctx.load_scenarios(scen, orders)
    if rows is not None:
        ctx.set_scenario_pods(rows)
    setup(ctx)
    ctx.run_loaded(True)
    return ctx.fetch(True)


def _check_both_calls(ctx, batch, res, extras=False):
    """Both calls on `ctx` (which has just run the batch) against the restatement of the placements `res` holds."""
    prob, scen, orders, setup, held, want, rows, evict = batch
    S, N = held.shape
    ref = UU.node_usage(prob, res.placement, held)
    rng = np.random.default_rng(S + N)
    sub = rng.permutation(S)[:max(1, S - 3)].astype(np.int32)                      # a permuted sub-list
    dup = np.array([S - 1, 0, S - 1, 0], np.int32)                                 # a list with duplicates
    for ids in (None, sub, dup):
        pick = np.arange(S) if ids is None else ids
        u = ctx.fetch_node_usage(ids, eph=True, scalars=True)
        assert u.req_cpu.tolist() == ref.req_cpu[pick].tolist() and u.req_mem.tolist() == ref.req_mem[pick].tolist()
        assert u.npods.tolist() == ref.npods[pick].tolist()
        assert u.req_eph.tolist() == ref.req_eph[pick].tolist() and u.scalar_req.tolist() == ref.scalar_req[pick].tolist()
        lean = ctx.fetch_node_usage(ids)                                           # the optional arrays NULL
        assert lean.req_cpu.tolist() == u.req_cpu.tolist() and lean.npods.tolist() == u.npods.tolist() and lean.req_eph is None
    assert ((ref.npods == -1) == ~held).all()
    assert ref.req_cpu.sum(1).tolist() == res.used_cpu.tolist() and ref.req_mem.sum(1).tolist() == res.used_mem.tolist()
    probes = _probe_pods(prob)
    fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True)
    rf, rn, rx = UU.headroom(prob, res.placement, held, probes, ref)
    assert fit.tolist() == rf.tolist() and nodes.tolist() == rn.tolist() and exact.tolist() == rx.tolist()
    only, none_, _ = ctx.fetch_headroom(probes)                                    # fit_nodes NULL
    assert none_ is None and only.tolist() == rf.tolist()
    if extras:
        assert ref.req_eph.any() and ref.scalar_req.any()
    return rf, rx


ROUTE_ENVS = [("table", {}), ("narrow_v1", {"SIMON_NARROW_V1": "1"}), ("no_cache", {"SIMON_NO_CACHE": "1"}), ("force_wide", {"SIMON_FORCE_WIDE": "1"})]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("route,env", ROUTE_ENVS, ids=[r[0] for r in ROUTE_ENVS])
def test_both_calls_on_every_route_of_a_prefix_batch(route, env, tile, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _tile(monkeypatch, tile)
    batch = _batch("prefix", 130)
    with capi.Context(0) as ctx:
        res = _load(ctx, batch)
        st = ctx.stats()
        if route == "table":
            assert st.kernel_variant == capi.KERNEL_NARROW_CACHE
        if route == "force_wide":
            assert st.kernel_variant == capi.KERNEL_WIDE
        assert res.placement.tolist() == batch[5].tolist()
        fit, exact = _check_both_calls(ctx, batch, res)
    assert exact.any() and not exact.all() and (fit > 0).any()


def test_own_nodes_batches_are_still_refused_on_the_all_feature_kernel(monkeypatch):
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    prob, scen, orders, setup, held, want, rows, evict = _batch("subset", 65)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        setup(ctx)
        with pytest.raises(capi.SimonError) as e:
            ctx.run_loaded(True)
        assert e.value.code == capi.ESTATE
        for call in (lambda: ctx.fetch_node_usage(), lambda: ctx.fetch_headroom([0])):
            with pytest.raises(capi.SimonError) as e:
                call()
            assert e.value.code == capi.ESTATE and "no placements" in str(e.value)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_both_calls_on_every_kind_of_batch_with_and_without_tiles(kind, N, monkeypatch):
    batch = _batch(kind, N)
    prob, scen, orders, setup, held, want, rows, evict = batch
    assert 6 <= len(scen) <= 12
    if kind in ("podset", "own_podset"):
        assert not rows[1].any()
    first = None
    for tile in TILES:
        _tile(monkeypatch, tile)
        with capi.Context(0) as ctx:
            res = _load(ctx, batch)
            assert res.placement.tolist() == want.tolist(), (kind, N, tile)
            fit, _ = _check_both_calls(ctx, batch, res)
        assert first is None or fit.tolist() == first.tolist()
        first = fit


@pytest.mark.parametrize("tile", TILES)
def test_ephemeral_storage_and_two_scalars_with_zero_quantity_entries(tile, monkeypatch):
    _tile(monkeypatch, tile)
    batch = _batch("prefix", 130, True)
    prob = batch[0]
    assert prob.req_eph is not None and len(prob.scalar_alloc) == 2 and prob.scalar_entries is not None
    with capi.Context(0) as ctx:
        res = _load(ctx, batch)
        assert res.placement.tolist() == batch[5].tolist()
        _check_both_calls(ctx, batch, res, extras=True)
        # probes that carry a scalar ENTRY of quantity 0 (the shortcut is off for them) and probes that request scalars
        ent = np.asarray(prob.scalar_entries)
        zero_entry = np.flatnonzero((ent != 0) & (np.asarray(prob.scalar_req) == 0).all(0))[:4]
        with_scalar = np.flatnonzero((np.asarray(prob.scalar_req) != 0).any(0))[:4]
        assert len(zero_entry) and len(with_scalar)
        probes = np.concatenate([zero_entry, with_scalar])
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True)
        rf, rn, rx = UU.headroom(prob, res.placement, batch[4], probes)
        assert fit.tolist() == rf.tolist() and nodes.tolist() == rn.tolist() and exact.tolist() == rx.tolist()


@pytest.mark.parametrize("N", [5, 70])
def test_headroom_is_what_the_oracle_places_after_the_device_s_own_stream(N):
    """The appended-probes check of test_usage_host.py on the device's own placements: fit + 3 copies of every exact probe behind the
    stream, exactly fit of them placed by the oracle, no earlier pod moved."""
    prob, named = UU.constructed_problem(3, N)
    order = np.random.default_rng(3).permutation(prob.n_pods).astype(np.int32)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch([[N, 0]], order[None])
        probes = list(named.values())
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True)
    assert res.placement[0].tolist() == O.run(prob, [[N, 0]], order[None]).placement[0].tolist()
    assert exact.all() and (fit[0] > 0).any() and (fit[0] == 0).any()
    for k, p in enumerate(probes):
        UU.check_probe_against_oracle(prob, N, order, res.placement[0], p, fit[0, k])


def _expect(rc, code, ctx, text):
    assert rc == code, (rc, ctx.lib.simon_last_error(ctx.h))
    assert text in ctx.lib.simon_last_error(ctx.h).decode(), ctx.lib.simon_last_error(ctx.h)


def test_refusals_by_code_and_message_and_what_they_leave_behind():
    batch = _batch("prefix", 65)
    prob, scen = batch[0], batch[1]
    S, N, P = len(scen), prob.n_nodes, prob.n_pods
    i32 = lambda a: capi._ptr(a, C.c_int32)                                                            # noqa: E731
    i64 = lambda a: capi._ptr(a, C.c_int64)                                                            # noqa: E731
    cpu, mem, npods = np.zeros((S, N), np.int64), np.zeros((S, N), np.int64), np.zeros((S, N), np.int32)
    fit = np.zeros((S, 70), np.int64)

    def usage_struct(size=None, have=("req_cpu", "req_mem", "npods")):
        o = capi.NodeUsageC()
        o.struct_size = C.sizeof(capi.NodeUsageC) if size is None else size
        o.req_cpu = i64(cpu if "req_cpu" in have else None)
        o.req_mem = i64(mem if "req_mem" in have else None)
        o.npods = i32(npods if "npods" in have else None)
        return o

    with capi.Context(0) as ctx:
        lib, h = ctx.lib, ctx.h
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, batch[2])
        good = usage_struct()
        probes = np.array(_probe_pods(prob), np.int32)
        # nothing has run; a run that stored no placements
        _expect(lib.simon_fetch_node_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom(h, i32(probes), len(probes), i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(False)
        assert UU.usage_errors(S, None, S, have_placement=False) == ["no placements"]
        _expect(lib.simon_fetch_node_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom(h, i32(probes), len(probes), i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(True)
        res = ctx.fetch(True)
        before_u = ctx.fetch_node_usage()
        before_h = ctx.fetch_headroom(probes, nodes=True)
        bad_ids = np.array([0, S], np.int32)
        neg_ids = np.array([-1], np.int32)
        for what, n, ids, o, text in (("n", 0, None, good, "scenarios listed"), ("n", -3, None, good, "scenarios listed"),
                                      ("scenario id", 2, bad_ids, good, "outside [0,"), ("scenario id", 1, neg_ids, good, "outside [0,"),
                                      ("scenario id", S + 1, None, good, "outside [0,"),
                                      ("missing array", S, None, usage_struct(have=("req_cpu", "npods")), "missing required arrays"),
                                      ("missing array", S, None, usage_struct(have=("req_cpu", "req_mem")), "missing required arrays"),
                                      ("missing array", S, None, usage_struct(have=("req_mem", "npods")), "missing required arrays"),
                                      ("struct_size", S, None, usage_struct(size=40), "size mismatch")):
            assert what in UU.usage_errors(S, ids, n, have=tuple(k for k in ("req_cpu", "req_mem", "npods") if getattr(o, k)),
                                           struct_ok=o.struct_size == C.sizeof(capi.NodeUsageC))
            _expect(lib.simon_fetch_node_usage(h, None if ids is None else i32(ids), n, C.byref(o)), capi.EINVAL, ctx, text)
        for what, K, pp, f, text in (("K", 0, probes, fit, "probes outside [1, 64]"), ("K", 65, np.zeros(65, np.int32), fit, "probes outside [1, 64]"),
                                     ("pod id", 2, np.array([0, P], np.int32), fit, "outside [0,"), ("pod id", 1, np.array([-1], np.int32), fit, "outside [0,"),
                                     ("missing array", 1, probes, None, "missing required arrays")):
            assert what in UU.headroom_errors(P, pp, K, have_fit=f is not None)
            _expect(lib.simon_fetch_headroom(h, i32(pp), K, i64(f), None, None), capi.EINVAL, ctx, text)
        # a refused call leaves results and batch alone: the same good calls give the same answers, the results are still there
        after_u = ctx.fetch_node_usage()
        after_h = ctx.fetch_headroom(probes, nodes=True)
        assert after_u.req_cpu.tolist() == before_u.req_cpu.tolist() and after_u.npods.tolist() == before_u.npods.tolist()
        assert all(np.asarray(a).tolist() == np.asarray(b).tolist() for a, b in zip(after_h, before_h))
        assert ctx.fetch(True).placement.tolist() == res.placement.tolist()
        # a reload since the run: the placements no longer belong to what is loaded
        p = prob.c_pods()
        assert lib.simon_load_pods(h, C.byref(p)) == 0
        assert UU.usage_errors(S, None, S, reloaded=True) == ["no placements"] == UU.headroom_errors(P, probes, len(probes), reloaded=True)
        _expect(lib.simon_fetch_node_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom(h, i32(probes), len(probes), i64(fit), None, None), capi.ESTATE, ctx, "no placements")


def test_sweeps_on_the_device_equal_the_oracle_backed_engine():
    cluster, apps, types = MU.example_simple()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    pods, _ = sim.build_stream(cluster, apps, list(cluster["Node"]), len(cluster["Node"]))
    refs, seen = [], set()
    for p in pods:
        owner = (p["metadata"].get("ownerReferences") or [{}])[0].get("name")
        if owner and owner not in seen and not (p.get("spec") or {}).get("nodeName"):
            seen.add(owner)
            refs.append((p["metadata"]["namespace"], p["metadata"]["name"]))
    refs = refs[:3]
    a = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=sim.HipEngine(), headroom=refs, node_table=True)
    b = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
    assert a.unscheduled == b.unscheduled
    assert a.headroom == b.headroom and a.headroom_exact == b.headroom_exact and a.node_table == b.node_table
    assert any(v > 0 for row in a.headroom for v in row)
    fa = sim.sweep_failures(cluster, apps, "node", engine=sim.HipEngine(), headroom=refs, node_table=True)
    fb = sim.sweep_failures(cluster, apps, "node", engine=UU.UsageOracleEngine(), headroom=refs, node_table=True)
    assert fa.batched and fb.batched and fa.unscheduled == fb.unscheduled
    assert fa.headroom == fb.headroom and fa.headroom_exact == fb.headroom_exact and fa.node_table == fb.node_table

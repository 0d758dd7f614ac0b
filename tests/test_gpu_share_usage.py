"""GPU-share device usage and the device bound of headroom on the device (simon_fetch_gpu_usage, simon_fetch_headroom_gpu): both calls
against the plain-loop restatement (gpu_usage_util) of the placements and slices the device itself fetched, and those against the
unmodified oracle -- on every kernel route that records devices, for every kind of batch, on pools around the 64-node tile edge with
the tile unset and forced to 64 nodes; headroom end to end against the oracle (appended probes); parity with simon_fetch_headroom;
every refusal; problems without GPU requests; the sweeps on HipEngine against the oracle-backed engine.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import evict_util as EU
import gpu_usage_util as GU
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


def _probe_pods(prob, n=10):
    """Probe pods: exact GPU probes first (distinct memory / count / class), then GPU pods that are pinned or preset (bounded, not exact),
    then pods without a GPU request (one per class)."""
    seen, gpu, rest, plain = set(), [], [], []
    for p in range(prob.n_pods):
        key = (int(prob.pod_class[p]), int(prob.gpu_mem[p]), int(prob.pod_gpu_cnt[p]))
        if key in seen:
            continue
        if prob.gpu_mem[p] > 0:
            (gpu if GU.probe_exact_gpu(prob, p) else rest).append(p)
            seen.add(key)
        elif prob.pod_gpu_cnt[p] == 0 and ("plain", key[0]) not in seen:
            plain.append(p)
            seen.add(("plain", key[0]))
    by_shape = {}
    for p in gpu:                                                                 # spread over the (memory, count) shapes
        by_shape.setdefault((int(prob.gpu_mem[p]), int(prob.pod_gpu_cnt[p])), p)
    gpu = list(by_shape.values())
    return (gpu[:n - 4] + rest[:2] + plain[:2])[:n]


@functools.lru_cache(maxsize=None)
def _batch(kind, N):
    """One batch of `kind` over a pool of N nodes with GPU-share nodes and pods, P = 300: (problem, scen, orders, setup(ctx) -> None, held
    bool [S][N], oracle placement rows [S][P], oracle slices rows [S][P], pod rows, evict flags)."""
    seed = 11 * N + KINDS.index(kind)
    rng = np.random.default_rng(seed)
    P, S = 300, 8
    kw = dict(N=N, P=P, gpu=True, gates=True, presets=True, static_mask=True, n_node_classes=min(5, N))
    if kind == "prefix":
        prob = randprob.rand_problem(seed, init_state=True, **kw)
    else:
        prob, _ = MU.segmentable(randprob.rand_problem(seed, **kw), fixed=0)
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
        ranks = SU.zone_ranks(held, zone)
        if kind == "subset_evict":
            ok = EU.eligible(prob)
            prob, evict = EU.flag(prob, {int(ok[i]): int(j) for i, j in enumerate(rng.integers(0, N, 6))})
        setup = lambda ctx: ctx.set_scenario_nodes(held, zone)                                          # noqa: E731
    scen = np.stack([np.asarray(held, bool).sum(1), oid[:len(held)]], 1).astype(np.int32)
    rows = None
    if kind in ("podset", "own_podset"):
        rows = rng.random((len(held), P)) < 0.6
        rows[0] = True
        rows[1] = False                                                                                # a scenario holding no pod
    want, slices = [], []
    for s in range(len(held)):
        order = orders[scen[s, 1]]
        if rows is not None:
            one = PU.oracle_prefix(prob, rows[s], int(scen[s, 0]), order) if kind == "podset" else PU.oracle_nodes(prob, rows[s], held[s], order, ranks[s])
            row, sl = one.placement, one.gpu_slices
        elif evict is not None:
            row, ref, _ = EU.oracle_rows(prob, evict, held[s:s + 1], scen[s:s + 1], orders, ranks[s:s + 1])[0]
            sl = ref.gpu_slices[0]
        elif kind == "prefix":
            ref = O.run(prob, scen[s:s + 1], orders, want_gpu_slices=True)
            row, sl = ref.placement[0], ref.gpu_slices[0]
        else:
            row, ref = MU.oracle_of_scenario(prob, held[s], order, None if ranks is None else ranks[s])
            sl = ref.gpu_slices[0]
        want.append(row)
        slices.append(sl)
    return prob, scen, orders, setup, held, np.stack(want), np.stack(slices).astype(np.uint64), rows, evict


def _load(ctx, batch, slices=True):
    """Run the batch with the devices recorded; None where run_loaded refuses it (SIMON_ESTATE)."""
    prob, scen, orders, setup, held, want, want_sl, rows, evict = batch
    ctx.load_problem(prob)
    if evict is not None:
        ctx.set_pod_eviction(evict)
    ctx.load_scenarios(scen, orders)
    if rows is not None:
        ctx.set_scenario_pods(rows)
    setup(ctx)
    try:
        ctx.run_loaded(True, slices)
    except capi.SimonError as e:
        assert e.code == capi.ESTATE, e
        return None
    return ctx.fetch(True, slices)


def _refused(ctx):
    """A batch run_loaded refused: both calls say that there are no placements."""
    for call in (lambda: ctx.fetch_gpu_usage(), lambda: ctx.fetch_headroom([0], devices=True)):
        with pytest.raises(capi.SimonError) as e:
            call()
        assert e.value.code == capi.ESTATE and "no placements" in str(e.value)


def _check_both_calls(ctx, batch, res):
    """Both calls on `ctx` (which has just run the batch) against the restatement of the placements and slices `res` holds."""
    prob, scen, orders, setup, held, want, want_sl, rows, evict = batch
    S, N = held.shape
    ref = GU.dev_usage(prob, res.placement, res.gpu_slices, held)
    rng = np.random.default_rng(S + N)
    sub = rng.permutation(S)[:max(1, S - 3)].astype(np.int32)                      # a permuted sub-list
    dup = np.array([S - 1, 0, S - 1, 0], np.int32)                                 # a list with duplicates
    for ids in (None, sub, dup):
        pick = np.arange(S) if ids is None else ids
        g = ctx.fetch_gpu_usage(ids, pods=True)
        assert g.dev_used.tolist() == ref.dev_used[pick].tolist(), ids
        assert g.dev_pods.tolist() == ref.dev_pods[pick].tolist(), ids
        lean = ctx.fetch_gpu_usage(ids)                                            # dev_pods NULL
        assert lean.dev_pods is None and lean.dev_used.tolist() == g.dev_used.tolist()
    assert ((ref.dev_pods[:, :, 0] == -1) == ~held).all()
    probes = _probe_pods(prob)
    fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, devices=True)
    rf, rn, rx = GU.headroom_gpu(prob, res.placement, res.gpu_slices, held, probes)
    assert fit.tolist() == rf.tolist() and nodes.tolist() == rn.tolist() and exact.tolist() == rx.tolist()
    only, none_, _ = ctx.fetch_headroom(probes, devices=True)                      # fit_nodes NULL
    assert none_ is None and only.tolist() == rf.tolist()
    # parity with the old call: probes without a GPU request elementwise; GPU probes there keep the resource bound and exact = 0
    plain = [p for p in probes if prob.gpu_mem[p] == 0 and prob.pod_gpu_cnt[p] == 0]
    gpus = [p for p in probes if prob.gpu_mem[p] > 0]
    assert plain and gpus
    a, b = ctx.fetch_headroom(plain, nodes=True, devices=True), ctx.fetch_headroom(plain, nodes=True)
    assert all(np.asarray(x).tolist() == np.asarray(y).tolist() for x, y in zip(a, b))
    of, on_, ox = ctx.fetch_headroom(gpus, nodes=True)
    uf, un, ux = UU.headroom(prob, res.placement, held, gpus)
    assert of.tolist() == uf.tolist() and on_.tolist() == un.tolist() and not ox.any() and not ux.any()
    strict = bool((rf[:, [probes.index(p) for p in gpus]] < uf).any())          # the devices are the bottleneck for some probe and scenario
    return rf, rx, strict


def _against_oracle(batch, res):
    assert res.placement.tolist() == batch[5].tolist()
    assert res.gpu_slices.tolist() == batch[6].tolist()


ROUTE_ENVS = [("gpu_fold", {}, capi.KERNEL_NARROW_CACHE), ("gpu_rows", {"SIMON_NO_GPU_FOLD": "1"}, capi.KERNEL_NARROW_CACHE),
              ("force_wide", {"SIMON_FORCE_WIDE": "1"}, capi.KERNEL_WIDE)]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("route,env,variant", ROUTE_ENVS, ids=[r[0] for r in ROUTE_ENVS])
def test_both_calls_on_every_route_that_records_devices(route, env, variant, tile, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _tile(monkeypatch, tile)
    batch = _batch("prefix", 130)
    with capi.Context(0) as ctx:
        res = _load(ctx, batch)
        assert res is not None
        st = ctx.stats()
        print(f"{route}: variant {st.kernel_variant} generation {st.kernel_generation}")
        assert st.kernel_variant == variant
        _against_oracle(batch, res)
        fit, exact, strict = _check_both_calls(ctx, batch, res)
    assert exact.any() and not exact.all() and (fit > 0).any() and strict


def test_own_nodes_batches_are_still_refused_on_the_all_feature_kernel(monkeypatch):
    monkeypatch.setenv("SIMON_FORCE_WIDE", "1")
    with capi.Context(0) as ctx:
        assert _load(ctx, _batch("subset", 65)) is None
        _refused(ctx)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_both_calls_on_every_kind_of_batch_with_and_without_tiles(kind, N, monkeypatch):
    batch = _batch(kind, N)
    assert 6 <= len(batch[1]) <= 12
    first = None
    for tile in TILES:
        _tile(monkeypatch, tile)
        with capi.Context(0) as ctx:
            res = _load(ctx, batch)
            if res is None:                                                        # run_loaded refuses this kind for a GPU problem
                assert kind != "prefix"
                print(f"{kind} N={N}: refused by run_loaded")
                _refused(ctx)
                continue
            _against_oracle(batch, res)
            fit, _, _ = _check_both_calls(ctx, batch, res)
        assert first is None or fit.tolist() == first.tolist()
        first = fit


@pytest.mark.parametrize("N,P", [(5, 30), (70, 200)])
def test_headroom_is_what_the_oracle_places_after_the_device_s_own_stream(N, P):
    """The appended-probes check of test_gpu_share_usage_host.py on the device's own placements: fit + 3 copies of every exact GPU probe
    behind the stream, exactly fit of them placed by the oracle, no earlier pod moved."""
    prob = randprob.rand_problem(N, N=N, P=P, gpu=True, static_mask=True, init_state=True, gates=True)
    order = np.random.default_rng(N).permutation(P).astype(np.int32)
    probes = [p for p in _probe_pods(prob, 12) if prob.gpu_mem[p] > 0 and GU.probe_exact_gpu(prob, p)]
    assert len(probes) >= 4
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        res = ctx.run_batch([[N, 0]], order[None], True, True)
        fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, devices=True)
        old, _, _ = ctx.fetch_headroom(probes)
    ref = O.run(prob, [[N, 0]], order[None], want_gpu_slices=True)
    assert res.placement[0].tolist() == ref.placement[0].tolist() and res.gpu_slices[0].tolist() == ref.gpu_slices[0].tolist()
    assert exact.all() and (fit[0] > 0).any() and (fit[0] < old[0]).any()
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
    used = np.zeros((S + 1, N, GU.D), np.int64)
    fit = np.zeros((S, 70), np.int64)

    def usage_struct(size=None, have=True):
        o = capi.GpuUsageC()
        o.struct_size = C.sizeof(capi.GpuUsageC) if size is None else size
        o.dev_used = i64(used if have else None)
        return o

    with capi.Context(0) as ctx:
        lib, h = ctx.lib, ctx.h
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, batch[2])
        good = usage_struct()
        probes = np.array(_probe_pods(prob), np.int32)
        K = len(probes)
        # nothing has run; a run that stored no placements
        _expect(lib.simon_fetch_gpu_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_gpu(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(False, False)
        assert GU.gpu_usage_errors(S, None, S, have_placement=False, gpu=True) == ["no placements"]
        _expect(lib.simon_fetch_gpu_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_gpu(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        # placements, but no devices recorded: the message names the flag; the old calls and the results are untouched
        ctx.run_loaded(True, False)
        plain = ctx.fetch(True)
        assert GU.has_gpu(prob) and GU.gpu_usage_errors(S, None, S, gpu=True, have_slices=False) == ["no devices recorded"]
        assert GU.headroom_gpu_errors(P, probes, K, gpu=True, have_slices=False) == ["no devices recorded"]
        _expect(lib.simon_fetch_gpu_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "SIMON_WANT_GPU_SLICES")
        _expect(lib.simon_fetch_headroom_gpu(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "SIMON_WANT_GPU_SLICES")
        assert ctx.fetch(True).placement.tolist() == plain.placement.tolist()
        old_call = ctx.fetch_headroom(probes, nodes=True)                           # simon_fetch_headroom needs no devices
        ctx.run_loaded(True, True)
        res = ctx.fetch(True, True)
        assert res.placement.tolist() == plain.placement.tolist()
        assert all(np.asarray(a).tolist() == np.asarray(b).tolist() for a, b in zip(ctx.fetch_headroom(probes, nodes=True), old_call))
        before_u = ctx.fetch_gpu_usage(pods=True)
        before_h = ctx.fetch_headroom(probes, nodes=True, devices=True)
        bad_ids = np.array([0, S], np.int32)
        neg_ids = np.array([-1], np.int32)
        for what, n, ids, o, text in (("n", 0, None, good, "scenarios listed"), ("n", -3, None, good, "scenarios listed"),
                                      ("scenario id", 2, bad_ids, good, "outside [0,"), ("scenario id", 1, neg_ids, good, "outside [0,"),
                                      ("scenario id", S + 1, None, good, "outside [0,"),
                                      ("missing array", S, None, usage_struct(have=False), "missing required arrays"),
                                      ("struct_size", S, None, usage_struct(size=16), "size mismatch")):
            assert what in GU.gpu_usage_errors(S, ids, n, have_dev_used=bool(o.dev_used), struct_ok=o.struct_size == C.sizeof(capi.GpuUsageC), gpu=True)
            _expect(lib.simon_fetch_gpu_usage(h, None if ids is None else i32(ids), n, C.byref(o)), capi.EINVAL, ctx, text)
        for what, k, pp, f, text in (("K", 0, probes, fit, "probes outside [1, 64]"), ("K", 65, np.zeros(65, np.int32), fit, "probes outside [1, 64]"),
                                     ("pod id", 2, np.array([0, P], np.int32), fit, "outside [0,"), ("pod id", 1, np.array([-1], np.int32), fit, "outside [0,"),
                                     ("missing array", 1, probes, None, "missing required arrays")):
            assert what in GU.headroom_gpu_errors(P, pp, k, have_fit=f is not None, gpu=True)
            _expect(lib.simon_fetch_headroom_gpu(h, i32(pp), k, i64(f), None, None), capi.EINVAL, ctx, text)
            assert "fetch_headroom_gpu" in lib.simon_last_error(h).decode()
        # a refused call leaves results and batch alone: the same good calls give the same answers, the results are still there
        after_u = ctx.fetch_gpu_usage(pods=True)
        after_h = ctx.fetch_headroom(probes, nodes=True, devices=True)
        assert after_u.dev_used.tolist() == before_u.dev_used.tolist() and after_u.dev_pods.tolist() == before_u.dev_pods.tolist()
        assert all(np.asarray(a).tolist() == np.asarray(b).tolist() for a, b in zip(after_h, before_h))
        again = ctx.fetch(True, True)
        assert again.placement.tolist() == res.placement.tolist() and again.gpu_slices.tolist() == res.gpu_slices.tolist()
        # a reload since the run: the placements no longer belong to what is loaded
        p = prob.c_pods()
        assert lib.simon_load_pods(h, C.byref(p)) == 0
        assert GU.gpu_usage_errors(S, None, S, reloaded=True, gpu=True) == ["no placements"] == GU.headroom_gpu_errors(P, probes, K, reloaded=True, gpu=True)
        _expect(lib.simon_fetch_gpu_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_gpu(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")


@pytest.mark.parametrize("N", [65, 130])
def test_a_problem_without_gpu_requests_returns_the_state_before_the_stream(N):
    # no GPU arrays at all: answered without the flag, all zero; headroom with devices is the old call
    prob = randprob.rand_problem(N, N=N, P=300, gates=True, presets=True, static_mask=True, init_state=True)
    scen = np.array([[N, 0], [max(1, N // 2), 0]], np.int32)
    order = np.arange(300, dtype=np.int32)[None]
    assert not GU.has_gpu(prob)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, order)
        ctx.run_loaded(True, False)
        res = ctx.fetch(True)
        g = ctx.fetch_gpu_usage(pods=True)
        held = UU.held_rows(prob, scen)
        assert not g.dev_used.any() and ((g.dev_pods == -1) == ~held[:, :, None]).all() and (g.dev_pods <= 0).all()
        probes = list(range(6))
        a, b = ctx.fetch_headroom(probes, nodes=True, devices=True), ctx.fetch_headroom(probes, nodes=True)
        assert all(np.asarray(x).tolist() == np.asarray(y).tolist() for x, y in zip(a, b))
        assert res.placement.tolist() == O.run(prob, scen, order).placement.tolist()
    # GPU nodes with devices booked before the stream, no pod that asks for one: the state before the stream, node by node
    gp = randprob.rand_problem(N, N=N, P=300, gpu=True, gates=True, presets=True, static_mask=True, init_state=True)
    gp = EU.replaced(gp, gpu_mem=np.zeros(300, np.int64), pod_gpu_cnt=np.zeros(300, np.int32))
    with capi.Context(0) as ctx:
        ctx.load_problem(gp)
        ctx.load_scenarios(scen, order)
        ctx.run_loaded(True, True)
        res = ctx.fetch(True, True)
        g = ctx.fetch_gpu_usage(pods=True)
    ref = GU.dev_usage(gp, res.placement, res.gpu_slices, held)
    assert not res.gpu_slices.any() and g.dev_used.tolist() == ref.dev_used.tolist() and g.dev_pods.tolist() == ref.dev_pods.tolist()
    init = np.asarray(gp.init_gpu_used).reshape(N, GU.D)
    live = np.arange(GU.D)[None, :] < np.minimum(gp.gpu_cnt, GU.D)[:, None]
    assert g.dev_used[0].tolist() == np.where(live, init, 0).tolist() and g.dev_used.any()


def test_sweeps_on_the_device_equal_the_oracle_backed_engine():
    cluster, apps, types = MU.example_gpushare()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    refs = [("pai-gpu", "gpu-pod-00"), ("pai-gpu", "gpu-pod-02"), ("pai-gpu", "gpu-rs-03-0")]
    a = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=sim.HipEngine(), headroom=refs, node_table=True, devices=True)
    b = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
    assert a.unscheduled == b.unscheduled
    for f in ("headroom", "headroom_exact", "node_table", "gpu_table"):
        assert getattr(a, f) == getattr(b, f), f
    assert a.headroom_exact[:2] == [True, True] and any(v > 0 for row in a.headroom for v in row)
    assert any(d["pods"] > 0 for rows in a.gpu_table for r in rows for d in r["devices"])
    fa = sim.sweep_failures(cluster, apps, "node", engine=sim.HipEngine(), headroom=refs, node_table=True, devices=True)
    fb = sim.sweep_failures(cluster, apps, "node", engine=GU.GpuUsageOracleEngine(), headroom=refs, node_table=True, devices=True)
    assert fa.unscheduled == fb.unscheduled
    for f in ("headroom", "headroom_exact", "node_table", "gpu_table"):
        assert getattr(fa, f) == getattr(fb, f), f

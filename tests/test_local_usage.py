"""Open-Local usage and the storage bound of headroom on the device (simon_fetch_local_usage, simon_fetch_headroom_local): both calls
bit for bit against the host replay (simulate.host_local_usage / host_headroom(storage=True), which test_local_usage_host.py checks
against the unmodified oracle) of the placements the device itself fetched, and those placements against the oracle -- the random
cases with the tile unset and forced to 7 and 64 nodes, a pile-up longer than one staged chunk, two orders in one batch, listed
scenarios with repeats and in reverse, GPU share next to Open-Local, 1 / 5 / 64 probes on all three headroom calls, a problem without
Open-Local, every refusal.  Run with -m gpu on an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_usage_util as GU
import local_usage_util as LU
import oracle_lib as O
import randprob
import usage_util as UU
from open_simulator_amd import capi, simulate as sim

pytestmark = pytest.mark.gpu

TILES = [None, 7, 64]                      # SIMON_USAGE_TILE unset / 7 / 64 nodes: tile edges inside the pools, last tiles of 1 .. 6 nodes
CHUNK = 512                                # kLocalChunk of csrc/simon_subset.h: storage pods staged per pass


def _tile(monkeypatch, tile):
    """The knob is read once, when the context is made."""
    if tile is None:
        monkeypatch.delenv("SIMON_USAGE_TILE", raising=False)
    else:
        monkeypatch.setenv("SIMON_USAGE_TILE", str(tile))


@functools.lru_cache(maxsize=None)
def _case(N, P):
    prob, scen, orders = LU.random_case(N, P)
    return prob, scen, orders, O.run(prob, scen, orders)


def _run(ctx, prob, scen, orders, slices=False):
    ctx.load_problem(prob)
    ctx.load_scenarios(scen, orders)
    ctx.run_loaded(True, slices)
    return ctx.fetch(True, slices)


def _same_usage(got, want):
    assert got.scenarios.tolist() == want.scenarios.tolist()
    assert got.vg_req.tolist() == want.vg_req.tolist()
    assert got.dev_alloc.tolist() == want.dev_alloc.tolist()


def _check(ctx, prob, scen, orders, res, probes):
    """Both calls on `ctx` (which has just run the batch) against the host replay of the placements `res` holds."""
    held = UU.held_rows(prob, scen)
    S = len(scen)
    _same_usage(ctx.fetch_local_usage(), sim.host_local_usage(prob, res.placement, held, orders, scen))
    for ids in (np.arange(S)[::-1].astype(np.int32), np.array([S - 1, 0, S - 1, 0], np.int32)):           # in reverse; with repeats
        _same_usage(ctx.fetch_local_usage(ids), sim.host_local_usage(prob, res.placement, held, orders, scen, ids))
    fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, storage=True)
    rf, rn, rx = sim.host_headroom(prob, res.placement, held, probes, res.gpu_slices, storage=True, orders=orders, scen=scen)
    assert fit.tolist() == rf.tolist() and nodes.tolist() == rn.tolist() and exact.tolist() == rx.tolist()
    only, none_, _ = ctx.fetch_headroom(probes, storage=True)                                              # fit_nodes NULL
    assert none_ is None and only.tolist() == rf.tolist()
    return fit, exact


@pytest.mark.parametrize("N,P", LU.CASES)
def test_both_calls_on_the_random_cases_with_and_without_tiles(N, P, monkeypatch):
    prob, scen, orders, ref = _case(N, P)
    storage = LU.storage_probes(prob)
    plain = [p for p in range(P) if LU.spec_of_pod(prob, p) is None][:2]
    probes = storage + plain
    first = None
    for tile in TILES:
        _tile(monkeypatch, tile)
        with capi.Context(0) as ctx:
            res = _run(ctx, prob, scen, orders)
            assert res.placement.tolist() == ref.placement.tolist() and res.used_vg.tolist() == ref.used_vg.tolist()
            fit, exact = _check(ctx, prob, scen, orders, res, probes)
            use = ctx.fetch_local_usage()
            assert use.vg_req.sum(axis=(1, 2)).tolist() == ref.used_vg.tolist()
            assert (use.dev_alloc[1] == -1).any(), "the prefix scenario lacks nodes"
            # the neighbouring calls: a storage probe keeps exact = 0 and the resource bound there; a plain probe gives the same answer
            old = ctx.fetch_headroom(probes, nodes=True, devices=True)
            assert not old[2][:len(storage)].any() and exact[:len(storage)].all()
            assert (fit <= old[0]).all() and fit[:, len(storage):].tolist() == old[0][:, len(storage):].tolist()
        assert first is None or fit.tolist() == first.tolist()
        first = fit


@pytest.mark.parametrize("N,P", [LU.CASES[0], LU.CASES[3]])
def test_headroom_is_what_the_oracle_places_after_the_device_s_own_stream(N, P):
    prob, scen, orders, ref = _case(N, P)
    probes = LU.storage_probes(prob)
    with capi.Context(0) as ctx:
        res = _run(ctx, prob, scen, orders)
        fit, _, exact = ctx.fetch_headroom(probes, storage=True)
    assert exact.all()
    for k, p in enumerate(probes):
        UU.check_probe_against_oracle(prob, int(scen[0, 0]), orders[scen[0, 1]], res.placement[0], p, fit[0, k])


@functools.lru_cache(maxsize=None)
def _pile_up():
    """3 annotated nodes and 700 storage pods with any-VG volumes of 1, 2 and 3 GiB in turn (700 > CHUNK = 512, so the list takes two
    staged chunks): Open-Local's Binpack score prefers the node it fills most, so long runs of consecutive stream pods land on one
    node, one of them across the chunk edge.  Two pods without volumes sit among them in the stream."""
    nodes = [LU.node(vgs=[(0, 300, 0), (1, 290, 10)], pods=1000, cpu=10 ** 6, mem=1 << 44) for _ in range(3)]
    pods = [LU.pod(lvm=[(1 + i % 3, -1)], cpu=1, mem=1 << 20) for i in range(700)] + [LU.pod(cpu=1, mem=1 << 20) for _ in range(2)]
    prob = LU.problem(nodes, pods)
    order = np.concatenate([np.arange(300), [700], np.arange(300, 700), [701]]).astype(np.int32)
    return prob, np.array([[3, 0], [2, 0]], np.int32), order[None]


def test_a_pile_up_longer_than_one_staged_chunk(monkeypatch):
    prob, scen, orders = _pile_up()
    ref = O.run(prob, scen, orders)
    row = ref.placement[0][orders[0][orders[0] < 700]]                  # the storage pods' nodes in stream order
    assert len(row) == 700 > CHUNK and (row >= 0).all()
    runs = np.diff(np.concatenate([[0], np.flatnonzero(np.diff(row) != 0) + 1, [700]]))
    assert row[CHUNK - 1] == row[CHUNK], "a same-node run crosses the chunk edge"
    assert runs.max() >= 100 and len(set(row.tolist())) == 3, "long runs of consecutive pods on one node, every node used"
    for tile in (None, 2):
        _tile(monkeypatch, tile)
        with capi.Context(0) as ctx:
            res = _run(ctx, prob, scen, orders)
            assert res.placement.tolist() == ref.placement.tolist()
            fit, exact = _check(ctx, prob, scen, orders, res, [0, 1, 700])
            use = ctx.fetch_local_usage()
        assert use.vg_req.sum(axis=(1, 2)).tolist() == ref.used_vg.tolist()
        assert exact.all() and fit[0, 0] > 0
    UU.check_probe_against_oracle(prob, 3, orders[0], ref.placement[0], 1, fit[0, 1])


def test_two_orders_in_one_batch_end_in_two_states():
    prob = LU.problem([LU.node(vgs=[(0, 10, 0), (1, 20, 0)])], [LU.pod(lvm=[(8, -1)]), LU.pod(lvm=[(12, -1)])])
    scen, orders = np.array([[1, 0], [1, 1]], np.int32), np.array([[0, 1], [1, 0]], np.int32)
    with capi.Context(0) as ctx:
        res = _run(ctx, prob, scen, orders)
        assert res.placement.tolist() == [[0, 0], [0, 0]]
        use = ctx.fetch_local_usage()
        assert (use.vg_req[:, 0, :2] // LU.GiB).tolist() == [[8, 12], [0, 20]]
        _check(ctx, prob, scen, orders, res, [0, 1])


def test_devices_shortfall_and_a_pod_bound_by_node_name():
    nodes = [LU.node(vgs=[(0, 100, 5)], devs=[(LU.SSD, 10, 0), (LU.SSD, 20, 0), (LU.SSD, 100, 0), (LU.HDD, 50, 1), (LU.HDD, 40, 0)]),
             LU.node(annotated=False)]
    pods = [LU.pod(lvm=[(10, -1)], ssd=[10], preset=0), LU.pod(ssd=[50, 60]), LU.pod(lvm=[(7, 0)], hdd=[30]), LU.pod()]
    prob = LU.problem(nodes, pods)
    scen, orders = np.array([[2, 0]], np.int32), np.array([[0, 1, 2, 3]], np.int32)
    ref = O.run(prob, scen, orders)
    with capi.Context(0) as ctx:
        res = _run(ctx, prob, scen, orders)
        assert res.placement.tolist() == ref.placement.tolist() and res.placement[0, :3].tolist() == [0, 0, 0]
        use = ctx.fetch_local_usage()
        assert use.dev_alloc.tolist() == [[0b11100, 0]] and (use.vg_req[0, 0] // LU.GiB).tolist() == [12, 0, 0, 0]
        _check(ctx, prob, scen, orders, res, [1, 2, 3])


def test_gpu_share_next_to_open_local_all_three_bounds(monkeypatch):
    N, P = 23, 80
    prob = randprob.rand_problem(70, N=N, P=P, local=True, gpu=True, static_mask=True, init_state=True, gates=True)
    orders = np.stack([np.arange(P), np.random.default_rng(3).permutation(P)]).astype(np.int32)
    scen = np.array([[N, 1], [N - 6, 0], [N, 0]], np.int32)
    held = UU.held_rows(prob, scen)
    both = [p for p in LU.storage_probes(prob, 64) if prob.gpu_mem[p] > 0][:4]
    probes = both + [p for p in LU.storage_probes(prob) if prob.gpu_mem[p] == 0 and prob.pod_gpu_cnt[p] == 0][:3] + \
        [p for p in range(P) if LU.spec_of_pod(prob, p) is None and GU.probe_exact_gpu(prob, p) and prob.gpu_mem[p] > 0][:2]
    assert len(both) >= 2 and len(probes) >= 6
    ref = O.run(prob, scen, orders, want_gpu_slices=True)
    for tile in (None, 7):
        _tile(monkeypatch, tile)
        with capi.Context(0) as ctx:
            res = _run(ctx, prob, scen, orders, slices=True)
            assert res.placement.tolist() == ref.placement.tolist() and res.gpu_slices.tolist() == ref.gpu_slices.tolist()
            fit, exact = _check(ctx, prob, scen, orders, res, probes)
            dev = ctx.fetch_headroom(probes, devices=True)[0]
            plain = ctx.fetch_headroom(probes)[0]
            # without the recorded devices the call is refused as simon_fetch_headroom_gpu is
            ctx.run_loaded(True, False)
            with pytest.raises(capi.SimonError) as e:
                ctx.fetch_headroom(probes, storage=True)
            assert e.value.code == capi.ESTATE and "SIMON_WANT_GPU_SLICES" in str(e.value)
            _same_usage(ctx.fetch_local_usage(), sim.host_local_usage(prob, res.placement, held, orders, scen))   # (needs no devices)
        k = len(both)
        assert exact.all() and (fit <= dev).all() and (dev <= plain).all()
        assert (fit[:, :k] < dev[:, :k]).any() and (dev[:, :k] < plain[:, :k]).any(), "storage below devices below resources somewhere"
    for j, p in enumerate(both[:2]):
        UU.check_probe_against_oracle(prob, N, orders[1], ref.placement[0], p, fit[0, j])


@functools.lru_cache(maxsize=None)
def _probe_count_case():
    """The problem of the test above with the first 64 pod ids as probes (P = 80: none repeats), and, from the oracle's placements and
    devices, the host restatement of all three calls for the 64 -- a probe's column does not depend on its neighbours, so the first K
    columns are the answer for the first K probes."""
    N, P = 23, 80
    prob = randprob.rand_problem(70, N=N, P=P, local=True, gpu=True, static_mask=True, init_state=True, gates=True)
    orders = np.stack([np.arange(P), np.random.default_rng(3).permutation(P)]).astype(np.int32)
    scen = np.array([[N, 1], [N - 6, 0], [N, 0]], np.int32)
    ref = O.run(prob, scen, orders, want_gpu_slices=True)
    held, probes = UU.held_rows(prob, scen), np.arange(64, dtype=np.int32)
    want = {mode: sim.host_headroom(prob, ref.placement, held, probes, ref.gpu_slices, devices=mode == "devices", storage=mode == "storage",
                                    orders=orders, scen=scen) for mode in ("resources", "devices", "storage")}
    return prob, scen, orders, ref, want


@pytest.mark.parametrize("tile", [None, 7])
@pytest.mark.parametrize("K", [1, 5, 64])
def test_probe_count_edges_on_all_three_headroom_calls(K, tile, monkeypatch):
    """s_fit[K] and s_nodes[K] sit between the per-tile arrays of the headroom workgroup's LDS: one probe, a few, and SIMON_MAX_PROBES."""
    prob, scen, orders, ref, want = _probe_count_case()
    probes = np.arange(K, dtype=np.int32)
    _tile(monkeypatch, tile)
    with capi.Context(0) as ctx:
        res = _run(ctx, prob, scen, orders, slices=True)
        assert res.placement.tolist() == ref.placement.tolist() and res.gpu_slices.tolist() == ref.gpu_slices.tolist()
        for mode, flags in (("resources", {}), ("devices", dict(devices=True)), ("storage", dict(storage=True))):
            fit, nodes, exact = ctx.fetch_headroom(probes, nodes=True, **flags)
            rf, rn, rx = want[mode]
            assert fit.shape == (len(scen), K) and nodes.shape == (len(scen), K), mode
            assert fit.tolist() == rf[:, :K].tolist() and nodes.tolist() == rn[:, :K].tolist() and exact.tolist() == rx[:K].tolist(), mode


@pytest.mark.parametrize("gpu", [False, True])
def test_a_problem_without_open_local_gives_zeros_and_the_gpu_call_s_headroom(gpu):
    N, P = 70, 200
    prob = randprob.rand_problem(5, N=N, P=P, gpu=gpu, gates=True, presets=True, static_mask=True, init_state=True)
    scen, order = np.array([[N, 0], [N // 2, 0]], np.int32), np.arange(P, dtype=np.int32)[None]
    assert prob.local_flags is None
    with capi.Context(0) as ctx:
        res = _run(ctx, prob, scen, order, slices=gpu)
        use = ctx.fetch_local_usage()
        held = UU.held_rows(prob, scen)
        assert not use.vg_req.any() and use.dev_alloc.tolist() == np.where(held, 0, -1).tolist()
        probes = list(range(8))
        a, b = ctx.fetch_headroom(probes, nodes=True, storage=True), ctx.fetch_headroom(probes, nodes=True, devices=True)
        assert all(np.asarray(x).tolist() == np.asarray(y).tolist() for x, y in zip(a, b))
        _check(ctx, prob, scen, order, res, probes)


def _expect(rc, code, ctx, text):
    assert rc == code, (rc, ctx.lib.simon_last_error(ctx.h))
    assert text in ctx.lib.simon_last_error(ctx.h).decode(), ctx.lib.simon_last_error(ctx.h)


def test_refusals_by_code_and_message_and_what_they_leave_behind():
    prob, scen, orders, ref = _case(*LU.CASES[2])
    S, N, P = len(scen), prob.n_nodes, prob.n_pods
    i32 = lambda a: capi._ptr(a, C.c_int32)                                                            # noqa: E731
    i64 = lambda a: capi._ptr(a, C.c_int64)                                                            # noqa: E731
    vg = np.zeros((S + 1, N, capi.MAX_VG), np.int64)
    fit = np.zeros((S, 70), np.int64)

    def usage_struct(size=None, have=True):
        o = capi.LocalUsageC()
        o.struct_size = C.sizeof(capi.LocalUsageC) if size is None else size
        o.vg_req = i64(vg if have else None)
        return o

    with capi.Context(0) as ctx:
        lib, h = ctx.lib, ctx.h
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        good = usage_struct()
        probes = np.array(LU.storage_probes(prob), np.int32)
        K = len(probes)
        # nothing has run; a run that stored no placements
        _expect(lib.simon_fetch_local_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_local(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(False, False)
        assert LU.local_usage_errors(S, None, S, have_placement=False) == ["no placements"]
        _expect(lib.simon_fetch_local_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_local(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        ctx.run_loaded(True, False)
        res = ctx.fetch(True)
        before_u = ctx.fetch_local_usage()
        before_h = ctx.fetch_headroom(probes, nodes=True, storage=True)
        bad_ids, neg_ids = np.array([0, S], np.int32), np.array([-1], np.int32)
        for what, n, ids, o, text in (("n", 0, None, good, "scenarios listed"), ("n", -3, None, good, "scenarios listed"),
                                      ("scenario id", 2, bad_ids, good, "outside [0,"), ("scenario id", 1, neg_ids, good, "outside [0,"),
                                      ("scenario id", S + 1, None, good, "outside [0,"),
                                      ("missing array", S, None, usage_struct(have=False), "missing required arrays"),
                                      ("struct_size", S, None, usage_struct(size=16), "size mismatch")):
            assert what in LU.local_usage_errors(S, ids, n, have_vg_req=bool(o.vg_req), struct_ok=o.struct_size == C.sizeof(capi.LocalUsageC))
            _expect(lib.simon_fetch_local_usage(h, None if ids is None else i32(ids), n, C.byref(o)), capi.EINVAL, ctx, text)
            assert "fetch_local_usage" in lib.simon_last_error(h).decode()
        for what, k, pp, f, text in (("K", 0, probes, fit, "probes outside [1, 64]"), ("K", 65, np.zeros(65, np.int32), fit, "probes outside [1, 64]"),
                                     ("pod id", 2, np.array([0, P], np.int32), fit, "outside [0,"), ("pod id", 1, np.array([-1], np.int32), fit, "outside [0,"),
                                     ("missing array", 1, probes, None, "missing required arrays")):
            assert what in LU.headroom_local_errors(P, pp, k, have_fit=f is not None)
            _expect(lib.simon_fetch_headroom_local(h, i32(pp), k, i64(f), None, None), capi.EINVAL, ctx, text)
            assert "fetch_headroom_local" in lib.simon_last_error(h).decode()
        # a refused call leaves results and batch alone
        _same_usage(ctx.fetch_local_usage(), before_u)
        after_h = ctx.fetch_headroom(probes, nodes=True, storage=True)
        assert all(np.asarray(a).tolist() == np.asarray(b).tolist() for a, b in zip(after_h, before_h))
        assert ctx.fetch(True).placement.tolist() == res.placement.tolist()
        # a reload since the run: the placements no longer belong to what is loaded
        p = prob.c_pods()
        assert lib.simon_load_pods(h, C.byref(p)) == 0
        assert LU.local_usage_errors(S, None, S, reloaded=True) == ["no placements"] == LU.headroom_local_errors(P, probes, K, reloaded=True)
        _expect(lib.simon_fetch_local_usage(h, None, S, C.byref(good)), capi.ESTATE, ctx, "no placements")
        _expect(lib.simon_fetch_headroom_local(h, i32(probes), K, i64(fit), None, None), capi.ESTATE, ctx, "no placements")
        # loaded and run again, with another order set: the storage-pod lists follow the orders
        ctx.load_problem(prob)
        res2 = _run(ctx, prob, scen[:, ::1], orders[::-1].copy())
        _same_usage(ctx.fetch_local_usage(), sim.host_local_usage(prob, res2.placement, UU.held_rows(prob, scen), orders[::-1], scen))


def test_sweeps_on_the_device_equal_the_oracle_backed_engine():
    import mix_util as MU
    cluster, apps, types = MU.example_open_local()
    apps = [sim.AppResource(a.name, {k: v for k, v in a.resource.items() if k != "DaemonSet"}) for a in apps]
    refs = [("default", "nginx-lvm-0"), ("kube-system", "metrics-server-0")]
    a = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=sim.HipEngine(), headroom=refs, node_table=True, storage=True)
    b = sim.sweep(cluster, apps, types[0], [0, 1, 3], engine=LU.LocalUsageOracleEngine(), headroom=refs, node_table=True, storage=True)
    assert a.unscheduled == b.unscheduled
    for f in ("headroom", "headroom_exact", "node_table", "storage_table"):
        assert getattr(a, f) == getattr(b, f), f
    assert a.headroom_exact[0] and any(r["kind"] == "VG" and r["pct"] > 0 for rows in a.storage_table for r in rows)
    assert any(r["kind"].startswith("Device(") and r["used"] for rows in a.storage_table for r in rows)
    fa = sim.sweep_apps(cluster, apps, new_node=types[0], counts=[0, 2], engine=sim.HipEngine(), headroom=refs, storage=True)
    fb = sim.sweep_apps(cluster, apps, new_node=types[0], counts=[0, 2], engine=LU.LocalUsageOracleEngine(), headroom=refs, storage=True)
    assert fa.unscheduled == fb.unscheduled
    for f in ("headroom", "headroom_exact", "storage_table"):
        assert getattr(fa, f) == getattr(fb, f), f

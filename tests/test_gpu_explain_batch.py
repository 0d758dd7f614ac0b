"""simon_explain_batch on the device: many scenarios of the loaded batch replayed in one launch, each failed pod's per-node codes reduced
to a (code, node count) histogram on the device.  The yardstick is the C oracle per scenario -- O.run(prob, scen[s:s+1], orders,
explain_scenario=0, ...) -- with its code rows binned by np.unique (explain_util.binned).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import explain_util as XU
import image_util as IU
import mix_util as MU
import oracle_lib as O
import randprob
from open_simulator_amd import capi, simulate as sim

pytestmark = pytest.mark.gpu

FEATURES = {
    "topology+gpu": (dict(seed=3777, N=30, P=300, anti=True, aff=True, spread_hard=True, spread_soft=True, ipa=True, static_mask=True,
                          tight_pods=True, gpu=True), {0x1000, 0x2000, 0x4000, 0x8000}),
    "scalars+eph": (dict(seed=11, N=70, P=600, tight_pods=True, scalars=4, eph=True), {0x4000}),
    "local": (dict(seed=5, N=30, P=300, local=True, tight_pods=True), {0x0400, 0x4000}),
    "ports+anti_host": (dict(seed=7421, N=40, P=500, ports=True, anti_host=True, tight_pods=True, static_mask=True), {0x0800, 0x2000, 0x4000, 0x8000}),
}
LISTED = [3, 0, 5, 1, 4, 2, 3]            # all six scenarios, permuted, one repeat


def family(code):
    """The plugin family of a failure code: its leading bit (static 0x8000, fit 0x4000, topology 0x2000, gpu 0x1000, ports 0x0800, local 0x0400)."""
    return 1 << (int(code).bit_length() - 1) if code else 0


def oracle_explain(prob, scen, orders, s, max_failed, ranks=None, fold_images=False):
    """(n_failed, failed pods, [k][n] codes) of scenario s on the CPU oracle."""
    n = int(scen[s, 0])
    p = IU.fold_images(prob, n) if fold_images else prob
    _, ref = O.run(p, scen[s:s + 1], orders, explain_scenario=0, max_failed=max_failed, node_ranks=None if ranks is None else ranks[s:s + 1])
    return ref


def check(eb, k, ref, n, max_failed, max_bins, rows):
    """Listed scenario k of an ExplainBatch against the oracle's (n_failed, failed, codes)."""
    nf, failed, codes = ref
    assert int(eb.n_failed[k]) == nf
    rec = min(nf, max_failed)
    assert eb.recorded(k) == rec and eb.failed_pods[k, :rec].tolist() == failed.tolist()
    assert int(eb.n_nodes[k]) == n
    for i in range(rec):
        want_codes, want_counts = XU.binned(codes[i])
        nb = int(eb.n_bins[k, i])
        if rows:                                      # (the full row is what a host falls back to when the histogram overflows)
            assert eb.rows[k, i, :n].tolist() == codes[i].tolist() and not eb.rows[k, i, n:].any()
        if len(want_codes) > capi.EXPLAIN_BINS:
            assert nb == -1 and not eb.bins[k, i].view(np.uint8).any()
            continue
        assert nb == len(want_codes), (k, i)
        m = min(nb, max_bins)
        b = eb.bins[k, i]
        assert b["code"][:m].tolist() == want_codes[:m] and b["count"][:m].tolist() == want_counts[:m], (k, i)
        assert not b["pad"].any() and not b[m:].view(np.uint8).any()
        assert (eb.pod_bins(k, i) is None) == (nb > max_bins)
    assert not eb.bins[k, rec:].view(np.uint8).any() and not eb.n_bins[k, rec:].any()       # beyond what the scenario recorded: zero
    if rows:
        assert not eb.rows[k, rec:].any()


_REFS = {}


def feature_case(name, max_failed=64):
    """The problem, its six scenarios and the oracle's answers, computed once per case."""
    if name not in _REFS:
        kw, families = FEATURES[name]
        kw = dict(kw)
        prob = randprob.rand_problem(kw.pop("seed"), **kw)
        scen, orders = randprob.rand_scenarios(7, prob, S=6)
        refs = [oracle_explain(prob, scen, orders, s, max_failed) for s in range(6)]
        seen = {family(c) for r in refs for c in np.unique(r[2]).tolist()} - {0}
        assert seen == families, (name, sorted(hex(f) for f in seen))            # the inputs still reach the plugins they were chosen for
        assert all(139 <= r[0] <= 402 for r in refs), [r[0] for r in refs]     # every scenario fails more pods than the cap
        assert max(len(np.unique(row)) for r in refs for row in r[2]) <= 25
        _REFS[name] = (prob, scen, orders, refs)
    return _REFS[name]


@pytest.mark.parametrize("name", sorted(FEATURES))
def test_every_plugin_family_against_the_oracle(name):
    prob, scen, orders, refs = feature_case(name)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch(LISTED, max_failed=64, max_bins=32, rows=True)
        assert eb.scenarios.tolist() == LISTED and eb.rows.shape == (len(LISTED), 64, int(scen[:, 0].max()))
        for k, s in enumerate(LISTED):
            check(eb, k, refs[s], int(scen[s, 0]), 64, 32, True)
        # without rows, and as explain_loaded tells it scenario by scenario
        eb2 = ctx.explain_batch(LISTED, max_failed=64, max_bins=32)
        assert eb2.rows is None
        for f in ("n_failed", "failed_pods", "n_bins", "bins"):
            assert getattr(eb2, f).tobytes() == getattr(eb, f).tobytes(), f
        for s in range(6):
            nf, failed, codes = ctx.explain_loaded(s, 64)
            k = LISTED.index(s)
            assert nf == eb.n_failed[k] and failed.tolist() == eb.failed_pods[k, :len(failed)].tolist()
            for i, row in enumerate(codes):
                assert eb.pod_bins(k, i) == list(zip(*XU.binned(row)))


def test_single_explains_afterwards_are_those_of_a_fresh_context():
    prob, scen, orders, refs = feature_case("local")
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        nf, failed, codes = ctx.explain_loaded(2, 16)
        fresh = (nf, failed.tolist(), codes.tolist(), ctx.explain_local_detail(len(failed), int(scen[2, 0])).tolist())
    assert fresh[0] == refs[2][0] and fresh[2] == refs[2][2][:16].tolist()
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.explain_loaded(4, 16)
        before = ctx.explain_local_detail(16, int(scen[4, 0])).tolist()
        ctx.explain_batch(LISTED, 64, 32, rows=True)
        assert ctx.explain_local_detail(16, int(scen[4, 0])).tolist() == before       # the last SINGLE explain's sizes stay
        nf, failed, codes = ctx.explain_loaded(2, 16)
        assert (nf, failed.tolist(), codes.tolist(), ctx.explain_local_detail(len(failed), int(scen[2, 0])).tolist()) == fresh
        res = ctx.run_batch(scen, orders)
        assert res.unscheduled.tolist() == [r[0] for r in refs]


def test_max_bins_below_the_distinct_count():
    prob, scen, orders, refs = feature_case("topology+gpu")
    assert max(len(np.unique(row)) for r in refs for row in r[2]) > 2
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch(LISTED, max_failed=64, max_bins=2)
    assert int(eb.n_bins.max()) > 2                                   # the true count, beyond what the row holds
    for k, s in enumerate(LISTED):
        check(eb, k, refs[s], int(scen[s, 0]), 64, 2, False)


@pytest.mark.parametrize("N,P", [(257, 2400), (513, 4600)])
def test_pools_that_are_no_multiple_of_the_workgroup(N, P, monkeypatch):
    """257 / 513 nodes on 256 threads: lanes own 2 - 3 nodes, the last pass is ragged; scenarios of different sizes in one launch."""
    monkeypatch.setenv("SIMON_WG", "256")
    prob = randprob.rand_problem(N, N=N, P=P, tight_pods=True, static_mask=True, scalars=2)
    scen = np.array([[N, 0], [N - 1, 1], [N - 64, 0], [N - 29, 2]], np.int32)
    orders = randprob.rand_scenarios(3, prob, S=4)[1]
    listed = [2, 0, 3, 1]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch(listed, max_failed=12, max_bins=32, rows=True)
    for k, s in enumerate(listed):
        ref = oracle_explain(prob, scen, orders, s, 12)
        assert ref[0] > 12
        check(eb, k, ref, int(scen[s, 0]), 12, 32, True)


def test_a_scenario_without_failures_next_to_failing_ones():
    prob = randprob.rand_problem(32, N=60, P=160, tight_pods=True)
    orders = randprob.rand_scenarios(5, prob, S=4)[1]
    scen = np.array([[60, 0], [20, 0], [25, 1], [60, 2], [33, 1]], np.int32)
    refs = [oracle_explain(prob, scen, orders, s, 300) for s in range(5)]
    assert refs[0][0] == 0 and refs[3][0] == 0 and min(refs[s][0] for s in (1, 2, 4)) > 0
    listed = [1, 0, 2, 3, 4, 0]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch(listed, max_failed=300, max_bins=8, rows=True)      # a cap nobody reaches: every failed pod is recorded
    for k, s in enumerate(listed):
        check(eb, k, refs[s], int(scen[s, 0]), 300, 8, True)


def distinct_codes_problem():
    """128 nodes; node j < 127 lacks the resources named by the bits of j + 1 (cpu, memory, ephemeral storage, four extended resources:
    too small or zero) and has plenty of the rest, node 127 has plenty of everything; ONE pod that requests all seven.  The first n nodes
    give the pod n distinct NodeResourcesFit codes."""
    N = 128
    lacks = np.array([[((j + 1) >> b) & 1 if j < 127 else 0 for j in range(N)] for b in range(7)], bool)
    GiB = 1 << 30
    prob = capi.Problem(alloc_cpu=np.where(lacks[0], 100, 64000).astype(np.int64), alloc_mem=np.where(lacks[1], 64 << 20, 256 * GiB).astype(np.int64),
                        alloc_pods=np.full(N, 110, np.int32), node_class=np.zeros(N, np.int32),
                        req_cpu=np.array([1000], np.int64), req_mem=np.array([GiB], np.int64), pod_class=np.zeros(1, np.int32),
                        n_pod_classes=1, n_node_classes=1, simon_raw=np.zeros((1, 1), np.int64), const_score=np.full(1, 1000300, np.int64))
    prob.alloc_eph = np.where(lacks[2], 0, 100 * GiB).astype(np.int64)
    prob.req_eph = np.array([GiB], np.int64)
    prob.scalar_alloc = np.where(lacks[3:7], 0, 8).astype(np.int64)
    prob.scalar_req = np.ones((4, 1), np.int64)
    return prob.normalise()


def test_exactly_64_and_65_distinct_codes():
    prob = distinct_codes_problem()
    scen = np.array([[64, 0], [65, 0], [127, 0], [128, 0], [63, 0]], np.int32)
    orders = np.zeros((1, 1), np.int32)
    refs = [oracle_explain(prob, scen, orders, s, 4) for s in range(5)]
    assert [r[0] for r in refs] == [1, 1, 1, 0, 1]
    assert [len(np.unique(r[2][0])) for r in refs if r[0]] == [64, 65, 127, 63]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch([0, 1, 2, 3, 4], max_failed=4, max_bins=64, rows=True)
        assert eb.n_bins[:, 0].tolist() == [64, -1, -1, 0, 63]
        for s in range(5):
            check(eb, s, refs[s], int(scen[s, 0]), 4, 64, True)
        eb = ctx.explain_batch([1, 0], max_failed=1, max_bins=64)
        assert eb.n_bins[:, 0].tolist() == [-1, 64]


@pytest.mark.parametrize("budget_mb", ["0", "1"])
def test_state_chunks_give_identical_results(budget_mb, monkeypatch):
    """Per-scenario state is allocated for the POOL: 1 500 nodes with GPUs, four extended resources and ephemeral storage take more than
    1500 x (44 + 32 + 72) B = 222 KB per scenario, so a budget of 1 MB holds at most four of the five scenarios (two launches) and a
    budget of 0 one (five launches).  The scenarios themselves are small."""
    prob = randprob.rand_problem(77, N=1500, P=500, tight_pods=True, scalars=4, eph=True, gpu=True)
    orders = randprob.rand_scenarios(8, prob, S=5)[1]
    scen = np.array([[40, 0], [57, 1], [33, 2], [64, 0], [48, 1]], np.int32)
    listed = [4, 2, 0, 3, 1]
    out = []
    for env in (None, budget_mb):
        if env is not None:
            monkeypatch.setenv("SIMON_STATE_BUDGET_MB", env)               # read when the context is created
        with capi.Context(0) as ctx:
            ctx.load_problem(prob)
            ctx.load_scenarios(scen, orders)
            out.append(ctx.explain_batch(listed, max_failed=20, max_bins=16, rows=True))
    for f in ("n_failed", "failed_pods", "n_bins", "bins", "rows"):
        assert getattr(out[0], f).tobytes() == getattr(out[1], f).tobytes(), f
    for k, s in enumerate(listed):
        ref = oracle_explain(prob, scen, orders, s, 20)
        assert ref[0] > 0
        check(out[1], k, ref, int(scen[s, 0]), 20, 16, True)


def test_every_scenario_follows_its_own_rank_row():
    """Scenarios of ONE size with different node ranks (as test_gpu_round2's explain_loaded test builds them): the replay of a listed
    scenario breaks ties with ITS ranks, wherever it stands in the list."""
    prob = randprob.rand_problem(6100, N=40, P=400, tight_pods=True, static_mask=True)
    prob.alloc_cpu[:] = prob.alloc_cpu[0]; prob.alloc_mem[:] = prob.alloc_mem[0]; prob.node_class[:] = 0
    n = 30
    scen = np.array([[n, 0], [n, 0], [n, 0], [n - 3, 0]], np.int32)
    orders = np.arange(prob.n_pods, dtype=np.int32)[None]
    rng = np.random.default_rng(11)
    ranks = np.zeros((len(scen), prob.n_nodes), np.int32)
    for s in range(len(scen)):
        m = int(scen[s, 0])
        ranks[s, :m] = rng.permutation(m)
    listed = [2, 3, 1, 0, 2]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_node_ranks(ranks)
        eb = ctx.explain_batch(listed, max_failed=32, max_bins=32, rows=True)
    refs = [oracle_explain(prob, scen, orders, s, 32, ranks) for s in range(len(scen))]
    differ = 0
    for k, s in enumerate(listed):
        assert refs[s][0] > 0
        check(eb, k, refs[s], int(scen[s, 0]), 32, 32, True)
        if s in (1, 2):                                       # the same size under rank row 0
            other = O.run(prob, scen[s:s + 1], orders, explain_scenario=0, max_failed=32, node_ranks=ranks[0:1])[1]
            differ += int(other[0] != refs[s][0] or other[1].tolist() != refs[s][1].tolist() or other[2].tolist() != refs[s][2].tolist())
    assert differ, "rank row 0 would have given the same answers: the test does not discriminate"


def test_every_size_is_scored_with_its_own_image_slot():
    cluster, apps, template = IU.image_sweep_case(4, n_nodes=10, n_workloads=10, template_images=True, max_replicas=14)
    batch = sim.sweep_batch(cluster, apps, template, [0, 1, 2, 4, 6], image_batch=True)
    prob, scen, orders = batch.flat.problem, batch.scen, batch.orders
    assert prob.image_locality is not None and batch.node_ranks is None
    refs = [oracle_explain(prob, scen, orders, s, 24, fold_images=True) for s in range(len(scen))]
    failing = [s for s in range(len(scen)) if refs[s][0] > 0]
    assert len({int(scen[s, 0]) for s in failing}) >= 2, "the case needs failing scenarios of two sizes at least"
    listed = failing[::-1] + [failing[0]]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        eb = ctx.explain_batch(listed, max_failed=24, max_bins=32, rows=True)
    for k, s in enumerate(listed):
        check(eb, k, refs[s], int(scen[s, 0]), 24, 32, True)


def test_refusals_leave_the_context_usable():
    prob, scen, orders, refs = feature_case("scalars+eph")
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        with pytest.raises(capi.SimonError) as e:                             # nothing loaded
            ctx.explain_batch([0], 4, 4)
        assert e.value.code == -1
        ctx.load_scenarios(scen, orders)
        for bad in ([0, 6], [-1], [2, 1, 99]):
            with pytest.raises(capi.SimonError) as e:
                ctx.explain_batch(bad, 64, 32)
            assert e.value.code == -22, bad
        for kw in (dict(max_bins=0), dict(max_bins=65), dict(max_failed=0)):
            with pytest.raises(capi.SimonError) as e:
                ctx.explain_batch([0, 1], **kw)
            assert e.value.code == -22, kw
        with pytest.raises(capi.SimonError) as e:                             # rows one entry narrower than the largest listed scenario
            ctx.explain_batch([1, 0], 64, 32, rows=True, code_stride=int(scen[0, 0]) - 1)
        assert e.value.code == -22
        eb = ctx.explain_batch([5, 0], 64, 32, rows=True, code_stride=int(scen[:, 0].max()) + 3)       # a wider stride is fine
        check(eb, 0, refs[5], int(scen[5, 0]), 64, 32, True)
        check(eb, 1, refs[0], int(scen[0, 0]), 64, 32, True)
        res = ctx.run_batch(scen, orders)
        assert res.unscheduled.tolist() == [r[0] for r in refs]


def test_a_segmented_batch_is_refused():
    prob = randprob.rand_problem(21, N=30, P=260, tight_pods=True)
    scen, orders = randprob.rand_scenarios(2, prob, S=4)
    prob, F = MU.segmentable(prob, scen)
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        ctx.set_scenario_segments([F], scen[:, :1] - F)
        with pytest.raises(capi.SimonError, match="segmented") as e:
            ctx.explain_batch([0, 1], 16, 8)
        assert e.value.code == -1
        ctx.run_loaded(True)
        seg = ctx.fetch(True)
        ctx.set_scenario_segments(None, None)                                  # prefix scenarios again: the call goes through
        eb = ctx.explain_batch([1, 0], 16, 8)
        assert eb.n_failed.tolist() == [int(seg.unscheduled[1]), int(seg.unscheduled[0])]
        for k, s in enumerate([1, 0]):
            check(eb, k, oracle_explain(prob, scen, orders, s, 16), int(scen[s, 0]), 16, 8, False)


@pytest.mark.parametrize("name", sorted(XU.CASES))
def test_sweep_reasons_on_the_engine_equal_the_oracle_engine(name, monkeypatch):
    make, counts, text = XU.CASES[name]
    cluster, apps, types = make()
    calls = []
    real = capi.Context.explain_batch
    monkeypatch.setattr(capi.Context, "explain_batch", lambda self, *a, **kw: (calls.append(bool(kw.get("rows") or (len(a) > 3 and a[3]))), real(self, *a, **kw))[1])
    details = []
    real_detail = capi.Context.explain_local_detail
    monkeypatch.setattr(capi.Context, "explain_local_detail", lambda self, *a: (details.append(1), real_detail(self, *a))[1])
    got = sim.sweep(cluster, apps, types[0], counts, engine=sim.HipEngine(), reasons=True)
    want = sim.sweep(cluster, apps, types[0], counts, engine=MU.OracleEngine(), reasons=True)
    assert got.unscheduled == want.unscheduled and any(got.unscheduled)
    assert got.unscheduled_pods == want.unscheduled_pods
    assert text in " ".join(u["reason"] for lst in got.unscheduled_pods for u in lst)
    if name == "gpushare":
        assert calls == [False, True]                 # Node:<name> reasons: bins first, then the rows of those scenarios
    if name == "open_local":
        assert calls == [False, True] and details     # sizes in the text: rows, then the single replay with its details
    n_calls = len(calls)
    plain = sim.sweep(cluster, apps, types[0], counts, engine=sim.HipEngine())
    assert plain.unscheduled_pods == [] and len(calls) == n_calls          # reasons=False: no explain at all


def test_sweep_reasons_from_the_histograms_alone(monkeypatch):
    """The simple example without its app's DaemonSet: every size feeds the pool's pod stream, so no size is replayed by simulate(), and
    no reason names a node: ONE explain_batch without rows tells every failing size."""
    make, counts, text = XU.CASES["simple"]
    cluster, apps, types = make()
    for app in apps:
        app.resource.pop("DaemonSet", None)
    calls, singles = [], []
    real = capi.Context.explain_batch
    monkeypatch.setattr(capi.Context, "explain_batch", lambda self, *a, **kw: (calls.append((len(a[0]), bool(kw.get("rows")))), real(self, *a, **kw))[1])
    real_explain = capi.Context.explain
    monkeypatch.setattr(capi.Context, "explain", lambda self, *a, **kw: (singles.append(1), real_explain(self, *a, **kw))[1])
    got = sim.sweep(cluster, apps, types[0], counts, engine=sim.HipEngine(), reasons=True)
    want = sim.sweep(cluster, apps, types[0], counts, engine=MU.OracleEngine(), reasons=True)
    failing = sum(1 for u in want.unscheduled if u > 0)
    assert failing >= 2 and got.unscheduled == want.unscheduled
    assert got.unscheduled_pods == want.unscheduled_pods
    assert [len(lst) for lst in got.unscheduled_pods] == got.unscheduled
    assert calls == [(failing, False)] and not singles
    # groups of one scenario (a buffer budget below one scenario's): as many calls, the same answer
    calls.clear()
    engine = sim.HipEngine()
    engine.buffer_bytes = 1
    assert sim.sweep(cluster, apps, types[0], counts, engine=engine, reasons=True).unscheduled_pods == want.unscheduled_pods
    assert calls == [(1, False)] * failing


def test_single_replays_write_the_recorded_rows_and_nothing_else():
    """simon_explain / simon_explain_loaded through the library itself (capi.Context slices buffers of its own): failed_pods and
    fail_codes are written for the first min(return value, max_failed) pods, rows of the scenario's n_nodes; what lies behind them
    stays as the caller had it.  5 identical nodes of 1 000 mCPU, 6 identical pods of 600 mCPU: one pod per node, so 3 / 2 / 1 pods
    fail on 3 / 4 / 5 nodes."""
    GiB = 1 << 30
    prob = capi.Problem(alloc_cpu=np.full(5, 1000, np.int64), alloc_mem=np.full(5, 64 * GiB, np.int64), alloc_pods=np.full(5, 110, np.int32),
                        node_class=np.zeros(5, np.int32), req_cpu=np.full(6, 600, np.int64), req_mem=np.full(6, GiB, np.int64),
                        pod_class=np.zeros(6, np.int32), n_pod_classes=1, n_node_classes=1, simon_raw=np.zeros((1, 1), np.int64),
                        const_score=np.full(1, 1000300, np.int64)).normalise()
    scen = np.array([[3, 0], [5, 0]], np.int32)
    orders = np.arange(6, dtype=np.int32)[None, :]
    refs = {n: oracle_explain(prob, np.array([[n, 0]], np.int32), orders, 0, 8) for n in (3, 4, 5)}
    assert [refs[n][0] for n in (3, 4, 5)] == [3, 2, 1]
    PODS, CODES, GUARD = -7, 0xABCD, 2

    def replay(ctx, n, max_failed, scenario=None):
        """One call on sentinel-filled buffers two rows longer than max_failed; checks them against the oracle's run of n nodes."""
        failed = np.full(max_failed + GUARD, PODS, np.int32)
        codes = np.full((max_failed + GUARD) * n, CODES, np.uint16)
        if scenario is None:
            rc = ctx.lib.simon_explain(ctx.h, capi.Scenario(n, 0), capi._ptr(orders[0], capi.C.c_int32), capi._ptr(failed, capi.C.c_int32),
                                       capi._ptr(codes, capi.C.c_uint16), max_failed)
        else:
            rc = ctx.lib.simon_explain_loaded(ctx.h, scenario, capi._ptr(failed, capi.C.c_int32), capi._ptr(codes, capi.C.c_uint16), max_failed)
        nf, want_failed, want_codes = refs[n]
        k = min(nf, max_failed)
        assert rc == nf
        assert failed[:k].tolist() == want_failed[:k].tolist() and (failed[k:] == PODS).all()
        assert codes[:k * n].reshape(k, n).tolist() == want_codes[:k].tolist() and (codes[k * n:] == CODES).all()
        return rc, failed.tobytes(), codes.tobytes()

    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        first = replay(ctx, 3, 2, scenario=0)             # more failed pods than rows: rows 0 - 1, the guard rows untouched
        replay(ctx, 3, 8, scenario=0)                     # fewer: rows 0 - 2, rows 3 - 9 untouched
        replay(ctx, 4, 8)                                 # ad hoc, a size the batch does not hold: stride 4
        eb = ctx.explain_batch([1, 0], 8, 4)
        assert eb.n_failed.tolist() == [1, 3]
        assert replay(ctx, 3, 2, scenario=0) == first

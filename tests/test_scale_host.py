"""Replica-scaling sweeps, the host side (no GPU): sweep_scale against simulate() of every scenario's own scaled cluster on the CPU oracle
-- which pins "one order row and one presence row per replica level give every level its own stream inside one problem" --, that the
levels' orders really are not restrictions of the top level's, OrderSegments.compose() on hand cases, the refusals of the segment table
restated and matched against the library's validator (simon_orders.h, run stand-alone under sanitizers: the library's own argument
checks sit behind simon_ctx_create, which needs a device), the fallbacks, and the ctypes prototypes against the header."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import mix_util as MU
import podset_util as PU
import scale_util as XU
from open_simulator_amd import capi, simulate as sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [0, 1, 3, 7, 12, 20]
COUNTS = (0, 2)

# example_simple's app holds a DaemonSet, whose pod list follows the node count (the DaemonSet fallback below): its workloads run as one
# app each here, as in test_podsets_host.py
CASES = {"simple": lambda: _apps_split(MU.example_simple()), "gpushare": MU.example_gpushare, "zoned_service": lambda: MU.random_zoned(5, n_nodes=6)}


def _apps_split(case):
    cluster, apps, types = case
    return cluster, XU.split(apps), types


def _sweep(cluster, apps, scale, tmpl, combos=None, engine=None, **kw):
    engine = engine or XU.RecordingEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error", sim.ScaleFallbackWarning)
        res = sim.sweep_scale(cluster, apps, scale, new_node=tmpl, counts=COUNTS, combos=combos, engine=engine, reasons=True, **kw)
    assert res.batched and res.fallback is None and engine.batches > 0
    return res, engine


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_scale_equals_simulate_of_every_scenario(name):
    """The first workload of each case at 0 .. 20 replicas x counts (0, 2), reasons=True, on an oracle-backed engine that honours
    pod_present by running each scenario's OWN problem in the order row of its level: pod -> node by name, the unscheduled (ref, reason)
    lists, unscheduled_by_target, fits, min_count and max_level equal simulate() of that scaled cluster alone."""
    cluster, apps, types = CASES[name]()
    scale = [XU.first_target(apps, LEVELS)]
    res, engine = _sweep(cluster, apps, scale, types[0])
    assert res.combos == [(r,) for r in LEVELS] and res.counts == list(COUNTS) and res.targets == scale
    hand = XU.by_hand(cluster, apps, scale, res.combos, types[0], COUNTS)
    XU.check(res, apps, scale, COUNTS, hand, XU.batch_where(cluster, apps, scale, types[0], COUNTS, engine.launches))
    assert any(f for row in hand for _, f in row) and len({len(f) for row in hand for _, f in row}) > 1, "the levels must differ in what they leave unscheduled"
    # whole combos per launch: two scenarios each
    part, eng2 = _sweep(cluster, apps, scale, types[0], batch_scenarios=2)
    assert eng2.batches == len(LEVELS)
    assert (part.unscheduled, part.unscheduled_by_target, part.max_level, part.cpu_pct) == (res.unscheduled, res.unscheduled_by_target, res.max_level, res.cpu_pct)


def test_two_targets_in_one_app_and_across_apps():
    cluster, apps, types = MU.random_zoned(5, n_nodes=6)
    app = apps[0]
    dep, sts = app.resource["Deployment"][0]["metadata"]["name"], app.resource["StatefulSet"][0]["metadata"]["name"]
    # the same app: its variants are the PAIRS of levels the combos use
    scale = [(app.name, "Deployment", dep, [0, 2, 5]), (app.name, "StatefulSet", sts, [1, 4])]
    res, engine = _sweep(cluster, apps, scale, types[0])
    assert res.combos == [(0, 1), (0, 4), (2, 1), (2, 4), (5, 1), (5, 4)]
    hand = XU.by_hand(cluster, apps, scale, res.combos, types[0], COUNTS)
    XU.check(res, apps, scale, COUNTS, hand, XU.batch_where(cluster, apps, scale, types[0], COUNTS, engine.launches))
    # two apps, one target each, explicit combos (not the whole grid, one twice)
    two = XU.split(apps)
    names = {a.name: a for a in two}
    scale2 = [(f"deployment-{dep}", "Deployment", dep, [0, 2, 5]), (f"statefulset-{sts}", "StatefulSet", sts, [1, 4])]
    assert all(t[0] in names for t in scale2)
    combos = [(5, 4), (0, 1), (2, 4), (5, 4)]
    res2, engine2 = _sweep(cluster, two, scale2, types[0], combos=combos)
    assert res2.combos == combos
    hand2 = XU.by_hand(cluster, two, scale2, combos, types[0], COUNTS)
    XU.check(res2, two, scale2, COUNTS, hand2, XU.batch_where(cluster, two, scale2, types[0], COUNTS, engine2.launches))
    assert res2.unscheduled[0] == res2.unscheduled[3]


def test_the_levels_orders_are_not_the_top_orders_restricted():
    """What makes the per-level orders necessary: for example_simple some level's own order of the app's pods is NOT the top level's
    order restricted to the level's pods -- the test above would pass on identity orders otherwise."""
    cluster, apps, types = CASES["simple"]()
    scale = [XU.first_target(apps, LEVELS)]
    targets = sim._scale_targets(apps, scale)
    tops = sim._scaled_apps(apps, targets, [max(LEVELS)])
    batch = sim.sweep_batch(cluster, tops, types[0], list(COUNTS))
    segs, _ = sim.scale_segments(apps, targets, [(r,) for r in LEVELS], batch.flat, batch.pool)
    a = targets[0][0]
    rows, live = segs.variants[1 + a], segs.live[1 + a]
    assert live.tolist() == LEVELS
    top = rows[len(LEVELS) - 1]
    differ = [r for v, r in enumerate(LEVELS) if rows[v][:r].tolist() != [p for p in top.tolist() if p in set(rows[v][:r].tolist())]]
    assert differ, "every level's order is the top level's restricted: the case proves nothing"
    orders, present = segs.compose()
    assert (np.sort(orders, axis=1) == np.arange(orders.shape[1])).all() and present.sum(1).tolist() == [int(segs.seg_start[1]) + sum(
        int(segs.live[1 + b][segs.choice[c, 1 + b]]) for b in range(len(apps))) for c in range(len(LEVELS))]


def test_compose_on_hand_cases():
    # G = 1, one variant, all live
    one = capi.OrderSegments([0, 3], [[[2, 0, 1]]], None, [[0]])
    o, p = one.compose()
    assert o.tolist() == [[2, 0, 1]] and p.tolist() == [[True, True, True]]
    # an empty segment in the middle, live = 0 and live = len
    seg = capi.OrderSegments([0, 2, 2, 5], [[[0, 1], [1, 0]], np.zeros((1, 0), np.int32), [[2, 3, 4], [4, 3, 2], [3, 4, 2]]], [[2, 0], [0], [3, 1, 0]],
                             [[0, 0, 0], [1, 0, 1], [1, 0, 2], [0, 0, 1]])
    o, p = seg.compose()
    assert o.tolist() == [[0, 1, 2, 3, 4], [1, 0, 4, 3, 2], [1, 0, 3, 4, 2], [0, 1, 4, 3, 2]]
    assert p.tolist() == [[True] * 5, [False, False, False, False, True], [False] * 5, [True, True, False, False, True]]
    assert seg.n_orders == 4 and seg.n_pods == 5
    c, keep = seg.c_struct()
    assert c.n_seg == 3 and c.struct_size == capi.C.sizeof(capi.OrderSegmentsC) and keep[0].tolist() == [2, 1, 3] and keep[1].tolist() == [0, 1, 1, 0, 2, 3, 4, 4, 3, 2, 3, 4, 2]
    with pytest.raises(ValueError):
        capi.OrderSegments([0, 3], [[[2, 0, 1]], [[0]]], None, [[0]])
    with pytest.raises(ValueError):
        capi.OrderSegments([0, 3], [[[2, 0, 1]]], [[3, 3]], [[0]])
    # the restated rules accept what compose() takes
    assert XU.segment_error(5, 4, 3, seg.seg_start, keep[0], keep[1], keep[2], seg.choice.reshape(-1)) == "ok"


def _broken_tables():
    """(name of the rule, P, n_orders, G, seg_start, n_variants, pods, live or None, choice): hand tables that break one rule each, and
    valid ones."""
    good = (5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], [2, 0, 3], [0, 0, 1, 0])
    yield ("ok",) + good
    yield ("ok", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], None, [0, 0, 1, 0])
    yield ("ok", 3, 1, 3, [0, 0, 3, 3], [1, 2, 1], [2, 1, 0, 0, 1, 2], [0, 3, 0, 0], [0, 1, 0])                   # empty segments at both ends
    yield ("G", 0, 1, 0, [0], [], [], None, [])
    yield ("G", 65, 1, 65, list(range(66)), [1] * 65, list(range(65)), None, [0] * 65)
    yield ("ok", 64, 1, 64, list(range(65)), [1] * 64, list(range(64)), None, [0] * 64)
    yield ("starts", 5, 2, 2, [1, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], None, [0, 0, 1, 0])
    yield ("starts", 5, 2, 2, [0, 6, 5], [2, 1], [0], None, [0, 0, 1, 0])
    yield ("starts", 5, 2, 2, [0, 2, 4], [2, 1], [0, 1, 1, 0, 4, 2], None, [0, 0, 1, 0])
    yield ("variants", 5, 2, 2, [0, 2, 5], [2, 0], [0, 1, 1, 0], None, [0, 0, 1, 0])
    yield ("variants", 5, 2, 2, [0, 2, 5], [2, capi.MAX_ORDER_VARIANTS - 1], [0, 1, 1, 0], None, [0, 0, 1, 0])     # too many in all: refused before anything is sized
    yield ("variants", 5, 2, 2, [0, 2, 5], [2 ** 31 - 1, 2 ** 31 - 1], [0, 1, 1, 0], None, [0, 0, 1, 0])
    yield ("pod id", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 5, 3], None, [0, 0, 1, 0])
    yield ("pod id", 5, 2, 2, [0, 2, 5], [2, 1], [0, -1, 1, 0, 4, 2, 3], None, [0, 0, 1, 0])
    yield ("overlap", 5, 2, 2, [0, 2, 5], [2, 1], [0, 0, 1, 0, 4, 2, 3], None, [0, 0, 1, 0])                      # twice in a first row
    yield ("overlap", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 1, 2, 3], None, [0, 0, 1, 0])                      # in two segments: 4 is covered by none
    yield ("not a permutation", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 1, 4, 2, 3], None, [0, 0, 1, 0])            # a repeat in a later row
    yield ("not a permutation", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 4, 4, 2, 3], None, [0, 0, 1, 0])            # another segment's pod
    yield ("live", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], [3, 0, 3], [0, 0, 1, 0])
    yield ("live", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], [2, 0, -1], [0, 0, 1, 0])
    yield ("choice", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], None, [0, 0, 2, 0])
    yield ("choice", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], None, [0, 0, 1, 1])
    yield ("choice", 5, 2, 2, [0, 2, 5], [2, 1], [0, 1, 1, 0, 4, 2, 3], None, [-1, 0, 1, 0])


def test_segment_rules_restated_on_hand_cases():
    for want, *table in _broken_tables():
        assert XU.segment_error(*table) == want, (want, table)


def test_library_validator_agrees_with_the_restated_rules(tmp_path):
    """simon_orders.h -- the validation and the host twin behind simon_load_scenarios_composed -- is plain C++: a stand-alone program built
    with the address and undefined-behaviour sanitizers validates every hand table and random valid ones (the error kinds must be the
    restated ones) and composes the valid ones in its host loops (the rows must be OrderSegments.compose()'s)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"      # (the build's own compiler at the least)
    cases = list(_broken_tables())
    for seed, (P, cuts) in enumerate([(1, []), (33, [0, 1, 32]), (65, [33, 33, 64]), (200, [7, 100])]):
        t = XU.table_case(P, cuts, 3, 5, seed, live_values=lambda n: [0, min(1, n), n])
        _, (nv, pods, live) = t.c_struct()
        cases.append(("ok", P, 5, len(nv), t.seg_start.tolist(), nv.tolist(), pods.tolist(), live.tolist(), t.choice.reshape(-1).tolist()))
    lines = []
    for want, P, n_orders, G, st, nv, pods, live, choice in cases:
        lines.append(" ".join(map(str, [P, n_orders, G, len(st), *st, len(nv), *nv, len(pods), *pods, -1 if live is None else len(live), *(live or []),
                                        len(choice), *choice])))
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    src = tmp_path / "t.cpp"
    src.write_text('''
        #include "simon_orders.h"
        #include <cstdio>
        #include <vector>
        static std::vector<int32_t> arr(FILE* f, bool* absent = nullptr) {
            int n = 0;
            if (fscanf(f, "%d", &n) != 1) n = 0;
            if (absent) *absent = n < 0;
            std::vector<int32_t> v(n < 0 ? 0 : n);
            for (auto& x : v) if (fscanf(f, "%d", &x) != 1) x = 0;
            return v;
        }
        int main(int argc, char** argv) {
            FILE* f = fopen(argv[1], "r");
            int P, n_orders, G;
            while (fscanf(f, "%d %d %d", &P, &n_orders, &G) == 3) {
                bool no_live = false;
                // exact-size heap arrays: a read past what the rules allow is the sanitizer's to report
                std::vector<int32_t> st = arr(f), nv = arr(f), pods = arr(f), live = arr(f, &no_live), choice = arr(f);
                simon::OrderSegView v{G, st.data(), nv.data(), pods.data(), no_live ? nullptr : live.data(), choice.data()};
                simon::OrderSegTable t;
                long long at = -1;
                const int e = simon::order_segments_check(v, P, n_orders, t, &at);
                printf("%d", e);
                if (e == 0) {
                    const int W = (P + 31) / 32;
                    std::vector<int32_t> orders((size_t)n_orders * P), inv((size_t)n_orders * P);
                    std::vector<uint32_t> words((size_t)n_orders * W);
                    simon::order_segments_compose_host(t, pods.data(), no_live ? nullptr : live.data(), choice.data(), n_orders, orders.data(), inv.data(),
                                                       no_live ? nullptr : words.data());
                    for (int o = 0; o < n_orders; ++o)
                        for (int i = 0; i < P; ++i)
                            if (inv[(size_t)o * P + orders[(size_t)o * P + i]] != i) return 3;
                    for (int32_t x : orders) printf(" %d", x);
                    if (!no_live) for (uint32_t w : words) printf(" %u", w);
                }
                printf("\\n");
            }
            return 0;
        }''')
    exe = tmp_path / "t"
    subprocess.check_call([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "open-simulator_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe), str(tmp_path / "cases.txt")]).decode().strip().split("\n")
    assert len(out) == len(cases)
    for line, (want, P, n_orders, G, st, nv, pods, live, choice) in zip(out, cases):
        got = [int(x) for x in line.split()]
        assert XU.SEG_ERRORS[got[0]] == want == XU.segment_error(P, n_orders, G, st, nv, pods, live, choice), (want, line[:40])
        if want != "ok":
            assert len(got) == 1
            continue
        lens = np.diff(st)
        at, variants, lives, lat = 0, [], [], 0
        for g in range(G):
            variants.append(np.array(pods[at:at + nv[g] * lens[g]], np.int32).reshape(nv[g], lens[g]))
            at += nv[g] * lens[g]
            if live is not None:
                lives.append(live[lat:lat + nv[g]])
                lat += nv[g]
        orders, present = capi.OrderSegments(st, variants, lives if live is not None else None, np.array(choice).reshape(n_orders, G)).compose()
        assert got[1:1 + n_orders * P] == orders.reshape(-1).tolist()
        if live is not None:
            assert got[1 + n_orders * P:] == capi.presence_words(present).reshape(-1).tolist() if P else True


def test_fallbacks_warn_and_still_answer():
    cluster, apps, types = CASES["zoned_service"]()
    scale = [XU.first_target(apps, [0, 3, 7])]
    combos = [(0,), (3,), (7,)]
    hand = XU.by_hand(cluster, apps, scale, combos, types[0], COUNTS)

    def each(engine, match, cl=cluster, ap=apps, sc=scale, tmpl=types[0], want=hand):
        with pytest.warns(sim.ScaleFallbackWarning, match=match):
            res = sim.sweep_scale(cl, ap, sc, new_node=tmpl, counts=COUNTS, engine=engine, reasons=True)
        assert not res.batched and re.search(match, res.fallback)
        XU.check(res, ap, sc, COUNTS, want if want is not None else XU.by_hand(cl, ap, sc, res.combos, tmpl, COUNTS))
        return res
    # 1. an engine without pod subsets
    each(MU.OracleEngine(), "the engine has no pod subsets")
    # 2. two pods of one name: the cluster already runs a pod called like a replica
    ns = next(o for o in apps[0].resource[scale[0][1]] if o["metadata"]["name"] == scale[0][2])["metadata"].get("namespace") or "default"
    twin = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": f"{scale[0][2]}-1", "namespace": ns},
            "spec": {"containers": [{"name": "c", "image": "twin", "resources": {"requests": {"cpu": "10m", "memory": "8Mi"}}}]}}
    each(PU.PodsetOracleEngine(), "two pods are named", cl=dict(cluster, Pod=list(cluster.get("Pod", [])) + [twin]), want=None)
    # 3. an app with a DaemonSet: example_simple's whole app, whose own pod order at a size is not the pool's
    whole, wapps, wtypes = MU.example_simple()
    assert wapps[0].resource.get("DaemonSet")
    each(PU.PodsetOracleEngine(), r"app simple holds a DaemonSet, and its pod order at .* with \d+ new nodes is not the pool's", cl=whole, ap=wapps,
         sc=[XU.first_target(wapps, [1, 5])], tmpl=wtypes[0], want=None)
    # 4. node ranks the engine lacks (several zones)
    class NoRanks(PU.PodsetOracleEngine):
        supports_node_ranks = False
    each(NoRanks(), "node ranks")
    # 4b. ImageLocality the engine lacks: a node lists the image the target's pods run
    obj = next(o for o in apps[0].resource[scale[0][1]] if o["metadata"]["name"] == scale[0][2])
    image = obj["spec"]["template"]["spec"]["containers"][0]["image"]
    nodes = [dict(n) for n in cluster["Node"]]
    nodes[0] = dict(nodes[0], status=dict(nodes[0]["status"], images=[{"names": [image if ":" in image else image + ":latest"], "sizeBytes": 500 * 1024 * 1024}]))
    assert not getattr(PU.PodsetOracleEngine, "supports_image_locality", False)
    each(PU.PodsetOracleEngine(), "ImageLocality", cl=dict(cluster, Node=nodes), want=None)
    # 5. the engine refuses the batch
    class Refusing(PU.PodsetOracleEngine):
        def run(self, prob, scen, orders, **kw):
            if kw.get("pod_present") is not None:
                e = capi.SimonError("simon_run_loaded failed (-1): refused")
                e.code = capi.ESTATE
                raise e
            return super().run(prob, scen, orders, **kw)
    each(Refusing(), "the engine refused the batch")
    # an engine with pod subsets but without explain_batch: batched, the failing scenarios replayed one by one, the same texts
    class NoExplainBatch(PU.PodsetOracleEngine):
        supports_explain_batch = False
        explain_batch = None
    res = sim.sweep_scale(cluster, apps, scale, new_node=types[0], counts=COUNTS, engine=NoExplainBatch(), reasons=True)
    assert res.batched
    XU.check(res, apps, scale, COUNTS, hand)


def test_bad_targets_are_value_errors():
    cluster, apps, types = CASES["zoned_service"]()
    app = apps[0]
    dep = app.resource["Deployment"][0]["metadata"]["name"]
    eng = PU.PodsetOracleEngine()
    for scale, match in [([(app.name, "DaemonSet", "agent", [1])], "no replica count"), ([(app.name, "CronJob", "x", [1])], "no replica count"),
                         ([("nobody", "Deployment", dep, [1])], "names app"), ([(app.name, "Deployment", "nothing", [1])], "has no Deployment"),
                         ([(app.name, "Deployment", dep, [1, -1])], "none negative"), ([(app.name, "Deployment", dep, [1]), (app.name, "Deployment", dep, [2])], "a target twice"),
                         ([], "one target at least")]:
        with pytest.raises(ValueError, match=match):
            sim.sweep_scale(cluster, apps, scale, engine=eng)
    with pytest.raises(ValueError, match="one level of each"):
        sim.sweep_scale(cluster, apps, [(app.name, "Deployment", dep, [1, 2])], combos=[(3,)], engine=eng)
    with pytest.raises(ValueError, match="new node is nil"):
        sim.sweep_scale(cluster, apps, [(app.name, "Deployment", dep, [1, 2])], counts=(0, 1), engine=eng)
    assert eng.batches == 0


def test_engine_takes_segments_or_rows_not_both():
    seg = capi.OrderSegments([0, 1], [[[0]]], None, [[0]])
    for kw in ({"orders": np.zeros((1, 1), np.int32)}, {"pod_present": np.ones((1, 1), bool)}):
        with pytest.raises(ValueError, match="neither orders nor pod_present"):
            sim._segments_only(seg, kw.get("orders"), kw.get("pod_present"))
    sim._segments_only(None, np.zeros((1, 1), np.int32), None)
    assert sim.HipEngine.supports_order_segments and sim.HipEngine.supports_pod_subsets


def test_prototypes_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "simon_hip.h")).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert "int simon_load_scenarios_composed(simon_ctx* ctx, const simon_scenario* scen, int32_t S, const simon_order_segments* seg, int32_t n_orders);" in hdr
    assert "int simon_fetch_orders(simon_ctx* ctx, int32_t first, int32_t n, int32_t* orders , uint32_t* present );" in hdr
    assert "#define SIMON_MAX_ORDER_SEGMENTS 64" in hdr and capi.MAX_ORDER_SEGMENTS == 64
    body = re.search(r"typedef struct simon_order_segments \{(.*?)\} simon_order_segments;", hdr).group(1)
    fields = [f.strip().split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [n for n, _ in capi.OrderSegmentsC._fields_]
    assert "int simon_hip_version(void);" in hdr and capi.ABI_VERSION == 7
    assert {"simon_load_scenarios_composed", "simon_fetch_orders"} <= set(capi.EXPORTS)
    lib = capi.load_library()
    C = capi.C
    assert lib.simon_load_scenarios_composed.argtypes == [C.c_void_p, C.POINTER(capi.Scenario), C.c_int32, C.POINTER(capi.OrderSegmentsC), C.c_int32]
    assert lib.simon_fetch_orders.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    assert lib.simon_load_scenarios_composed.restype is C.c_int and lib.simon_fetch_orders.restype is C.c_int
    assert C.sizeof(capi.OrderSegmentsC) == 48

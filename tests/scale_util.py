"""Shared pieces of the replica-scaling tests (test_scale_host.py, test_gpu_scale.py): the yardstick -- simulate() of every scenario's own
scaled cluster on the CPU oracle --, an oracle-backed engine that records what a batch placed, the comparison by object names, the
refusals of simon_load_scenarios_composed's segment table restated, and small segment tables for the composition tests."""
import numpy as np

import mix_util as MU
import podset_util as PU
import subset_util as SU
from open_simulator_amd import capi, simulate as sim, workloads as wl


def split(apps, daemonsets=False):
    """One app per workload object of the given apps (DaemonSets left out unless asked for): test_podsets_host.py's helper."""
    out = []
    for app in apps:
        for kind, objs in app.resource.items():
            if kind == "DaemonSet" and not daemonsets:
                continue
            if kind in ("StorageClass", "Service", "ConfigMap", "PersistentVolumeClaim"):
                continue
            for o in objs:
                out.append(sim.AppResource(f"{kind.lower()}-{o['metadata']['name']}", {kind: [o]}))
    return out


def first_target(apps, levels):
    """(app name, kind, workload name, levels) of the first scalable workload of the first app that has one."""
    for app in apps:
        for kind in ("Deployment", "ReplicaSet", "StatefulSet", "Job"):
            for o in app.resource.get(kind, []):
                return (app.name, kind, o["metadata"]["name"], list(levels))
    raise AssertionError("no scalable workload")


class RecordingEngine(PU.PodsetOracleEngine):
    """PodsetOracleEngine that keeps (scen, placement) of every pod-subset batch, in launch order."""

    def __init__(self):
        super().__init__()
        self.launches = []

    def run(self, prob, scen, orders, **kw):
        res = super().run(prob, scen, orders, **kw)
        if kw.get("pod_present") is not None:
            self.launches.append((capi.scenarios_array(scen).copy(), res.placement.copy()))
        return res


def _ref(pod):
    return (pod["metadata"].get("namespace", ""), pod["metadata"]["name"])


def by_hand(cluster, apps, scale, combos, tmpl, counts):
    """simulate() of every (combo, count) on the oracle: [c][k] -> (where by pod ref, [(pod ref, reason)] of the unscheduled pods)."""
    targets = sim._scale_targets(apps, scale)
    out = []
    for combo in combos:
        mine = sim._scaled_apps(apps, targets, combo)
        out.append([])
        for k in counts:
            new = wl.new_fake_nodes(tmpl, k) if k else []
            if not sim.build_stream(cluster, mine, list(cluster["Node"]) + new, len(cluster["Node"]) + k)[0]:
                out[-1].append(({}, []))                               # (no pod at all: nothing to simulate)
                continue
            res = sim.simulate(cluster, mine, engine=MU.OracleEngine(), new_nodes=new)
            out[-1].append((SU.names_of(res), [(_ref(u["pod"]), u["reason"]) for u in res.unscheduled_pods]))
    return out


def batch_where(cluster, apps, scale, tmpl, counts, launches):
    """pod ref -> node name (None: unscheduled) of every scenario of the recorded launches, in scenario order over all launches: the
    batch's pool problem is rebuilt (sweep_batch with every target at its largest level) to name the pods and nodes."""
    targets = sim._scale_targets(apps, scale)
    tops = sim._scaled_apps(apps, targets, [max(t[3]) for t in targets])
    flat = sim.sweep_batch(cluster, tops, tmpl, list(counts)).flat
    refs = [_ref(p) for p in flat.pods]
    out = []
    for scen, placement in launches:
        for row in placement:
            out.append({refs[pid]: (flat.node_names[j] if j >= 0 else None) for pid, j in enumerate(row.tolist()) if j != capi.GATED})
    return out


def check(res, apps, scale, counts, hand, where=None):
    """A ScaleSweepResult (reasons=True) against by_hand's answers; where: batch_where's list, scenario (c, k) at c * K + k."""
    targets = sim._scale_targets(apps, scale)
    C, K, T = len(res.combos), len(counts), len(targets)
    for c in range(C):
        refs = [set(sim._target_refs(apps, targets[t], int(res.combos[c][t]))) for t in range(T)]
        for k in range(K):
            placed, failed = hand[c][k]
            assert res.unscheduled[c][k] == len(failed), (c, k)
            assert [(_ref(e["pod"]), e["reason"]) for e in res.unscheduled_pods[c][k]] == failed, (c, k)
            assert res.unscheduled_by_target[c][k] == [sum(ref in refs[t] for ref, _ in failed) for t in range(T)], (c, k)
            assert res.fits[c][k] == (len(failed) == 0), (c, k)                       # (caps 100: occupancy never refuses)
            if where is not None:
                assert where[c * K + k] == placed, (c, k)
        fit = [counts[k] for k in range(K) if not hand[c][k][1]]
        assert res.min_count[c] == (min(fit) if fit else None), c
    index = {tuple(combo): c for c, combo in enumerate(res.combos)}
    low = [min(t[3]) for t in targets]
    for t in range(T):
        for k in range(K):
            best = None
            for level in sorted(set(targets[t][3])):
                c = index.get(tuple(level if u == t else low[u] for u in range(T)))
                if c is None or hand[c][k][1]:
                    break
                best = level
            assert res.max_level[t][k] == best, (t, k)


# (case, environment, generation, threads per scenario): the score-table routes the switches of tests/test_gpu_routes.py force, on
# evict_util.route_problem's problems -- generations without rest (gates_*), GPU share folded and per node, the REST path (anti),
# generation 7 behind a Service as one wave and as a team
ROUTES = [("gates_fine", {"SIMON_TABLE_COARSE": "0"}, 4, 64),
          ("gates_coarse", {"SIMON_TABLE_COARSE": "1"}, 5, 64),
          ("gpu_fold", {}, 5, 64),
          ("gpu_hbm", {"SIMON_NO_GPU_FOLD": "1", "SIMON_LDS_WS": "0"}, 6, 64),
          ("anti", {}, 6, 64),
          ("service_wave", {"SIMON_TEAM": "0"}, 7, 64),
          ("service_team", {"SIMON_TEAM": "1"}, 7, 256)]


# ---- simon_load_scenarios_composed: the refusals of the segment table, restated (include/simon_hip.h) ----
SEG_ERRORS = ["ok", "G", "null", "starts", "variants", "pod id", "overlap", "not a permutation", "live", "choice"]     # OrderSegError's order


def segment_error(P, n_orders, G, seg_start, n_variants, pods, live, choice):
    """The first rule a table breaks, by the name SEG_ERRORS gives it ("ok": accepted).  pods: the flat variant rows; live: flat or None."""
    if G < 1 or G > capi.MAX_ORDER_SEGMENTS:
        return "G"
    st = list(seg_start)
    if st[0] != 0 or any(st[g + 1] < st[g] for g in range(G)) or st[G] != P:
        return "starts"
    if any(v < 1 for v in n_variants[:G]) or sum(n_variants[:G]) > capi.MAX_ORDER_VARIANTS:
        return "variants"
    owner, at, first_sets = {}, 0, []
    rows = []
    for g in range(G):
        n = st[g + 1] - st[g]
        rows.append([list(pods[at + w * n: at + (w + 1) * n]) for w in range(n_variants[g])])
        at += n_variants[g] * n
    # in the library's order: segment by segment, row by row, entry by entry
    for g in range(G):
        for w, row in enumerate(rows[g]):
            seen = set()
            for p in row:
                if p < 0 or p >= P:
                    return "pod id"
                if w == 0:
                    if p in owner:
                        return "overlap"
                    owner[p] = g
                elif owner.get(p) != g or p in seen:
                    return "not a permutation"
                seen.add(p)
    if live is not None:
        at = 0
        for g in range(G):
            for w in range(n_variants[g]):
                if not 0 <= live[at] <= st[g + 1] - st[g]:
                    return "live"
                at += 1
    for i, v in enumerate(choice):
        if not 0 <= v < n_variants[i % G]:
            return "choice"
    return "ok"


def table_case(P, cuts, n_var, n_orders, seed, live_values=None, last_everywhere=False):
    """A random valid capi.OrderSegments over P pods: segment boundaries at `cuts` (inside [0, P], repeats = empty segments), n_var
    variants per segment, random disjoint id sets; live_values: the values live draws from per segment (callable len -> list) or None;
    last_everywhere: order 0 picks the last variant of every segment."""
    rng = np.random.default_rng(seed)
    seg_start = np.array([0] + sorted(cuts) + [P], np.int32)
    G = len(seg_start) - 1
    ids = rng.permutation(P).astype(np.int32)
    variants, live = [], []
    for g in range(G):
        mine = ids[seg_start[g]:seg_start[g + 1]]
        variants.append(np.array([rng.permutation(mine) for _ in range(n_var)], np.int32).reshape(n_var, len(mine)))
        if live_values is not None:
            live.append(rng.choice(live_values(len(mine)), n_var).astype(np.int32))
    choice = rng.integers(0, n_var, (n_orders, G)).astype(np.int32)
    if last_everywhere:
        choice[0] = n_var - 1
    return capi.OrderSegments(seg_start, variants, live if live_values is not None else None, choice)

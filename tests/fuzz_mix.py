#!/usr/bin/env python3
"""Randomised parity sweep of SEGMENTED batches (simon_set_scenario_segments: a scenario holds the fixed nodes and a prefix of every pool
segment) on every route of the score-table kernel: generations 4 - 7, both workspace homes, one wave and the team of four, up to 256 node
classes, beyond 128 signatures, GPU share folded or as mask rows, REST && SPREAD, caller rank rows, 1 ... 8 segments with starts anywhere,
empty segments, no fixed nodes, all-zero and all-full scenarios, gated and pinned pods on segment nodes, pod priorities, plan caps.
Every placement, unscheduled count, used cpu / memory, GPU slice and preempt-risk flag of every scenario is compared with the CPU oracle
on that scenario's own node set (mix_util.oracle_of_scenario).  Cases from 500 000 on: random k8s clusters through simulate.sweep_mix,
every mix by object names against Simulate() of that mix alone (mix_util.mix_answer).

draw(case) and reference(inputs) need no GPU (tests/test_mix_host.py runs them); one_case = draw + reference + the device.
Not collected by pytest (a slice runs in tests/test_gpu_mix.py); by hand on a GPU box:   python tests/fuzz_mix.py [n_cases] [first_seed]"""
import os
import re
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401
import mix_util as MU  # noqa: E402
import randprob  # noqa: E402
from open_simulator_amd import capi, flatten as fl, simulate as sim  # noqa: E402

K8S_FIRST = 500000
# The deterministic slice (tests/test_gpu_mix.py): case -> ((kernel_variant, kernel_generation, workgroup_size) of each of its runs, the
# route families it is there for -- families() of its runs, "multi_segment" apart, which every case of the slice must be), as a
# campaign on an MI355X recorded them.
SLICE = {
         11: ([(4, 5, 64)], ['caller_ranks', 'gen5']),   # generation 5, caller ranks, 6 segments behind 92 fixed nodes, 40 node classes
         17: ([(4, 5, 64)], ['caller_ranks', 'gen5', 'sigs_over_128']),   # generation 5 with more than 128 signatures, caller ranks, 12 scenarios
         83: ([(4, 6, 64), (4, 6, 64)], ['caller_ranks', 'gen6_hbm', 'gen6_lds']),   # GPU share as mask rows, rows in HBM and in LDS, caller ranks
         124: ([(4, 5, 64)], ['gen5', 'gpu_fold']),   # GPU share + node-level anti-affinity folded into the table (generation 5)
         133: ([(4, 6, 64), (4, 6, 64)], ['gen6_hbm', 'gen6_lds']),   # generation 6 in HBM and in LDS, 7 segments behind 3 fixed nodes, 11 scenarios
         166: ([(4, 7, 64), (4, 7, 256)], ['gen7_team', 'gen7_wave', 'rest_and_spread']),   # REST && SPREAD, one wave and the team, 7 segments
         329: ([(4, 4, 64), (4, 4, 64)], ['caller_ranks', 'gen4_hbm', 'gen4_lds']),   # generation 4 fine, workspace in HBM and in LDS, caller ranks, pins (one node class)
         366: ([(4, 7, 64), (4, 7, 256)], ['gen7_team', 'gen7_wave', 'rest_and_spread']),   # REST && SPREAD, one wave and the team, no fixed nodes
         403: ([(4, 6, 64), (4, 6, 64)], ['gen6_hbm', 'gen6_lds']),   # generation 6 in HBM and in LDS, ports, priorities
         454: ([(4, 5, 64)], ['gen5', 'gpu_fold']),   # GPU share, anti-affinity and ports folded (generation 5), 379 nodes
         480: ([(4, 4, 64), (4, 4, 64)], ['gen4_hbm', 'gen4_lds']),   # generation 4 fine in HBM and in LDS
         482: ([(4, 4, 64)], ['caller_ranks', 'classes_129_256']),   # 192 caller node classes (four per lane), caller ranks, 8 segments
         521: ([(4, 5, 64)], ['caller_ranks', 'gen5']),   # generation 5, caller ranks, pinned pods without gates
         692: ([(4, 4, 64)], ['caller_ranks', 'classes_129_256']),   # 156 internal node classes (four per lane), caller ranks
         728: ([(4, 7, 64), (4, 7, 256)], ['caller_ranks', 'classes_65_128_gen6or7', 'gen7_team', 'gen7_wave']),   # 65 ... 128 internal node classes on generation 7, caller ranks, 423 nodes
         770: ([(4, 4, 64), (4, 4, 64)], ['caller_ranks', 'gen4_hbm', 'gen4_lds']),   # generation 4 fine in HBM and in LDS, caller ranks, 11 scenarios, 235 nodes
         968: ([(4, 7, 64), (4, 7, 256)], ['caller_ranks', 'classes_65_128_gen6or7', 'gen7_team', 'gen7_wave']),   # 88 internal node classes on generation 7, caller ranks
         500046: ([(4, 7, 256)], ['k8s_zones_1']),                     # k8s objects, one zone, three node types
         500059: ([(4, 7, 256)], ['caller_ranks', 'k8s_zones_2']),     # two zones (rank rows of sweep_mix), grids of two and three counts
         500033: ([(4, 7, 256)], ['caller_ranks', 'k8s_zones_3'])}     # three zones, three node types
# (randprob's odd_units is not drawn: gcd-1 memory quantities leave the narrow number range, such problems run on the all-feature kernel,
# which takes no segments -- 74 of 74 such cases were refused in the first campaign)
BASE = ["nz_differs", "init_state", "static_mask", "presets", "zero_pods", "tight_pods", "pins"]
KINDS = ["plain_fine", "plain_coarse", "classes256", "rest", "fold", "spread", "rest_spread", "many_sigs", "classes128", "free"]
FAMILIES = ["gen4_hbm", "gen4_lds", "gen5", "classes_129_256", "classes_65_128_gen6or7", "gen6_lds", "gen6_hbm", "gpu_fold", "gen7_wave",
            "gen7_team", "rest_and_spread", "sigs_over_128", "caller_ranks", "multi_segment"]
G_ = 1 << 30


def _rest_features(rng, feat, zone_terms=True):
    picked = False
    for f, pr in (("gpu", 0.5), ("anti_host", 0.3), ("anti", 0.25 if zone_terms else 0), ("ports", 0.25), ("eph", 0.2)):
        if rng.random() < pr:
            feat[f] = picked = True
    if rng.random() < (0.2 if zone_terms else 0.08):
        feat["scalars"] = int(rng.integers(1, 4))
        picked = True
    if not picked:
        feat["gpu"] = True
    if "anti" in feat:
        feat.pop("anti_host", None)
        if rng.random() < 0.4:
            feat["aff"] = True


def _spread_features(rng, feat):
    feat["spread_soft"] = True
    for f, pr in (("ipa_self", 0.12), ("hard_simple", 0.12)):
        if rng.random() < pr:
            feat[f] = True


def _few_gpu_kinds(prob):
    """GPU share the table can fold in: few request kinds (fuzz_spread.py does the same)."""
    prob.gpu_mem = np.where(prob.gpu_mem > 4 * G_, 8 * G_, np.where(prob.gpu_mem > 0, 2 * G_, 0)).astype(np.int64)
    prob.pod_gpu_cnt = np.where(prob.gpu_mem > 0, np.where(prob.pod_gpu_cnt >= 2, 2, 1), 0).astype(np.int32)
    prob.normalise()


def draw(case):
    """Everything one array-level case hands to the device and to the reference; pure numpy, seeded by `case`."""
    rng = np.random.default_rng(73000 + case)
    kind = KINDS[case % len(KINDS)]
    size = (case // len(KINDS)) % 4                                    # the band with thousands of nodes: a quarter of the cases
    N = int([rng.integers(6, 90), rng.integers(100, 600), rng.integers(600, 1400), rng.integers(1400, 3000)][size])
    P = int(rng.integers(20, 300 if size == 0 else 1200))
    feat = {f: True for f in BASE if rng.random() < 0.25}
    if rng.random() < 0.5:
        feat["gates"] = True
    env, runs = {}, [{}]
    n_node_classes = int(rng.choice([1, 2, 4, 9, 20, 40]))
    n_pod_classes = int(rng.choice([1, 3, 8, 30, 64, 120]))
    sub = kind
    if kind == "many_sigs":                                            # 129 + signatures under plain / REST / SPREAD rows
        n_pod_classes = int(rng.choice([130, 200, 300]))
        sub = str(rng.choice(["plain_fine", "plain_coarse", "rest", "spread", "rest_spread"]))
    if kind == "classes128":                                           # 65 .. 128 internal node classes on generation 6 / 7
        sub = str(rng.choice(["rest", "spread"]))
        n_node_classes = int(rng.choice([70, 90, 110])) if sub == "rest" else int(rng.choice([14, 18, 22, 25]))   # (spread: shapes x zones)
        N = max(N, int(rng.integers(300, 900)))
    if kind == "free":
        sub = str(rng.choice(["plain_fine", "plain_coarse", "rest", "fold", "spread", "rest_spread"]))
    if kind == "classes256":                                           # 129 .. 256 node classes: plain problems only, few signatures
        n_node_classes = int(rng.choice([129, 140, 160, 192, 200, 256]))
        n_pod_classes = int(rng.choice([1, 3, 8, 20, 40]))
        N = max(N, int(rng.integers(300, 1500)))
    elif sub == "plain_fine":
        env["SIMON_TABLE_COARSE"] = "0"
        runs = [{"SIMON_LDS_WS": "0"}, {"SIMON_LDS_WS": "1"}]
    elif sub == "plain_coarse":
        env["SIMON_TABLE_COARSE"] = "1"
    elif sub == "rest":                                                # mask rows of generation 6: nothing folded into the table
        _rest_features(rng, feat)
        env.update(SIMON_NO_GPU_FOLD="1", SIMON_NO_FOLD="1")
        runs = [{"SIMON_LDS_WS": "0"}, {"SIMON_LDS_WS": "1"}]
    elif sub == "fold":                                                # the same filters as monotone infeasibility of the table
        feat["gpu"] = True
        for f, pr in (("anti_host", 0.3), ("ports", 0.25)):
            if rng.random() < pr:
                feat[f] = True
    elif sub == "spread":
        _spread_features(rng, feat)
        n_node_classes = min(n_node_classes, int(rng.choice([1, 2, 4, 9]))) if kind != "classes128" else n_node_classes   # (x 5 zones inside)
        for f, pr in (("anti_host", 0.25), ("gpu", 0.25)):
            if rng.random() < pr:
                feat[f] = True
        runs = [{"SIMON_TEAM": "0"}, {"SIMON_TEAM": "1"}]
    elif sub == "rest_spread":                                         # walks over the mask rows
        _spread_features(rng, feat)
        feat.pop("hard_simple", None)
        n_node_classes = min(n_node_classes, int(rng.choice([1, 2, 4, 9])))
        _rest_features(rng, feat, zone_terms=False)                   # (required anti-affinity on zone keys beside the walks: the all-feature kernel)
        env.update(SIMON_NO_GPU_FOLD="1", SIMON_NO_FOLD="1")
        runs = [{"SIMON_TEAM": "0"}, {"SIMON_TEAM": "1"}]
    if size >= 2:                                                      # static masks are O(Cp N) Python work in the generator
        feat.pop("static_mask", None)
    prob = randprob.rand_problem(74000 + case, N=N, P=P, n_node_classes=n_node_classes, n_pod_classes=n_pod_classes, **feat)
    if "gpu" in feat and sub in ("fold", "spread"):
        _few_gpu_kinds(prob)
    if rng.random() < 0.25:                                            # pods of unequal priority: simon_fetch_preempt_risk
        prob.priority = rng.choice([0, 0, 0, 10, 1000, -5], P).astype(np.int32)
        prob.init_min_priority = int(rng.choice([0x7fffffff, 0, 100, 2000]))
        feat["priority"] = True
    # ---- segments: fixed nodes [0, F), 1 ... 8 segments behind them, starts anywhere
    F = 0 if rng.random() < 0.12 else int(rng.integers(1, max(2, (3 * N) // 4)))
    n_seg = int(min(rng.integers(1, capi.MAX_SEGMENTS + 1), max(1, N - F)))
    inner = np.sort(rng.choice(np.arange(F + 1, N), n_seg - 1, replace=False)) if n_seg > 1 else np.zeros(0, np.int64)
    if n_seg > 1 and rng.random() < 0.2:                               # an empty segment: two equal starts (or one that starts at N)
        g = int(rng.integers(0, n_seg - 1))
        inner[g] = inner[g + 1] if g + 1 < len(inner) else N
        inner = np.sort(inner)
    seg_start = np.concatenate([[F], inner]).astype(np.int32)
    seg_len = np.append(seg_start[1:], N) - seg_start
    prob, _ = MU.segmentable(prob, fixed=F)
    S = int(rng.integers(1, 13))
    n_orders = 3
    orders = np.stack([np.arange(P, dtype=np.int32)] + [rng.permutation(P).astype(np.int32) for _ in range(n_orders - 1)])
    counts = np.stack([rng.integers(0, seg_len[g] + 1, S) for g in range(n_seg)], 1).astype(np.int32)
    for s in range(S):
        u = rng.random()
        if u < 0.1:
            counts[s] = 0                                              # nothing but the fixed nodes
        elif u < 0.2:
            counts[s] = seg_len                                        # the whole pool
    if F == 0:                                                         # no fixed nodes: a scenario keeps one node at least
        first = int(np.flatnonzero(seg_len > 0)[0])
        for s in range(S):
            if counts[s].sum() == 0:
                counts[s, first] = 1
    scen = np.stack([F + counts.sum(1), rng.integers(0, n_orders, S)], 1).astype(np.int32)
    ranks = None
    if case % 3 == 2:                                                  # caller rank rows: a permutation over the scenario's own nodes, anything elsewhere
        ranks = rng.integers(-7, N + 7, (S, N)).astype(np.int32)
        for s in range(S):
            own = np.flatnonzero(MU.present_mask(N, seg_start, counts[s]))
            ranks[s, own] = rng.permutation(len(own))
    caps = sorted(int(c) for c in rng.integers(5, 101, int(rng.integers(2, 4)))) if rng.random() < 0.4 else []
    return SimpleNamespace(case=case, kind=kind, sub=sub, N=N, P=P, S=S, feat=feat, prob=prob, scen=scen, orders=orders, F=F, seg_start=seg_start,
                           counts=counts, ranks=ranks, env=env, runs=runs, caps=caps, want_gpu=prob.gpu_mem is not None,
                           n_node_classes=n_node_classes, n_pod_classes=n_pod_classes)


def present_of(inp, s):
    return MU.present_mask(inp.prob.n_nodes, inp.seg_start, inp.counts[s])


def reference(inp):
    """Per scenario the oracle on its own node set: placement row (pool indices), unscheduled, used cpu / memory, GPU slices where the
    problem has GPUs, preempt_risk where it has priorities."""
    S, P = inp.S, inp.P
    ref = SimpleNamespace(placement=np.zeros((S, P), np.int32), unscheduled=np.zeros(S, np.int64), used_cpu=np.zeros(S, np.int64),
                          used_mem=np.zeros(S, np.int64), gpu_slices=np.zeros((S, P), np.uint64) if inp.want_gpu else None,
                          preempt_risk=np.zeros(S, np.uint8) if inp.prob.priority is not None else None)
    for s in range(S):
        row, r = MU.oracle_of_scenario(inp.prob, present_of(inp, s), inp.orders[inp.scen[s, 1]], None if inp.ranks is None else inp.ranks[s])
        ref.placement[s], ref.unscheduled[s], ref.used_cpu[s], ref.used_mem[s] = row, r.unscheduled[0], r.used_cpu[0], r.used_mem[0]
        if ref.gpu_slices is not None:
            ref.gpu_slices[s] = r.gpu_slices[0]
        if ref.preempt_risk is not None:
            ref.preempt_risk[s] = r.preempt_risk[0]
    return ref


def plan_of(inp, ref, cap):
    """simon_min_plan_vg(cap, cap, 100) from the reference's results: the scenario with no unscheduled pod and cpu / memory occupancy of ITS
    OWN nodes within the cap that has the fewest nodes; ties: the first."""
    a, m = inp.prob.alloc_cpu.astype(np.int64), inp.prob.alloc_mem.astype(np.int64)
    best = None
    for s in range(inp.S):
        own = present_of(inp, s)
        if ref.unscheduled[s] or sim.occupancy_pct(int(ref.used_cpu[s]), int(a[own].sum())) > cap or \
                sim.occupancy_pct(int(ref.used_mem[s]) * 1000, int(m[own].sum()) * 1000) > cap:
            continue
        key = (int(inp.scen[s, 0]), s)
        best = key if best is None or key < best else best
    return (1, best[1]) if best else (0, -1)


def perturb(inp, how):
    """Valid inputs that differ from inp in ONE small way (what a kernel reading the wrong row would see), or None where inp offers no
    such change.  "count": one node of one scenario moved between two segments (same n_nodes); "rank": two entries of one caller rank row
    swapped; "gate": one gate moved to the neighbouring node of the same segment
    (where there is one, a gate at the edge of some scenario's prefix of that segment: elsewhere both nodes are present or absent together)."""
    import copy
    rng = np.random.default_rng(inp.case)
    out = copy.copy(inp)
    seg_len = np.append(inp.seg_start[1:], inp.prob.n_nodes) - inp.seg_start
    if how == "count":
        cand = [(s, a, b) for s in range(inp.S) for a in range(len(seg_len)) for b in range(len(seg_len))
                if a != b and inp.counts[s, a] > 0 and inp.counts[s, b] < seg_len[b]]
        if not cand:
            return None
        s, a, b = cand[int(rng.integers(0, len(cand)))]
        out.counts = inp.counts.copy()
        out.counts[s, a] -= 1
        out.counts[s, b] += 1
        if inp.ranks is not None:                      # keep the row a permutation over the scenario's nodes: the newcomer takes the leaver's rank
            out.ranks = inp.ranks.copy()
            gone, come = inp.seg_start[a] + inp.counts[s, a] - 1, inp.seg_start[b] + inp.counts[s, b]
            out.ranks[s, come] = inp.ranks[s, gone]
    elif how == "rank":
        if inp.ranks is None:
            return None
        cand = [s for s in range(inp.S) if inp.scen[s, 0] >= 2]
        if not cand:
            return None
        s = cand[int(rng.integers(0, len(cand)))]
        i, j = rng.choice(np.flatnonzero(present_of(inp, s)), 2, replace=False)
        out.ranks = inp.ranks.copy()
        out.ranks[s, [i, j]] = inp.ranks[s, [j, i]]
    elif how == "gate":
        g = inp.prob.gate_node
        if g is None:
            return None
        seg_of = np.searchsorted(inp.seg_start, np.arange(inp.prob.n_nodes), side="right") - 1
        pre = inp.prob.preset_node if inp.prob.preset_node is not None else np.full(inp.P, -1)
        cand = [p for p in np.flatnonzero((g >= inp.F) & (pre < 0)).tolist() if seg_len[seg_of[g[p]]] >= 2]
        if not cand:
            return None
        nb = lambda j: j + 1 if j + 1 < inp.prob.n_nodes and seg_of[j + 1] == seg_of[j] else j - 1   # noqa: E731
        present = np.stack([present_of(inp, s) for s in range(inp.S)])
        edge = [p for p in cand if (present[:, g[p]] != present[:, nb(int(g[p]))]).any()]   # (some scenario holds one of the two nodes only)
        cand = edge or cand
        p = cand[int(rng.integers(0, len(cand)))]
        j = int(g[p])
        k = nb(j)
        out.prob = copy.copy(inp.prob)
        out.prob.gate_node = g.copy()
        out.prob.gate_node[p] = k
        if out.prob.pin_node is not None and out.prob.pin_node[p] == j:
            out.prob.pin_node = out.prob.pin_node.copy()
            out.prob.pin_node[p] = k
    else:
        raise ValueError(how)
    return out


class _Stderr:
    """File descriptor 2 into a temporary file for the duration (the library's SIMON_DEBUG_ROUTE line names what decided the kernel)."""

    def __enter__(self):
        sys.stderr.flush()
        self.saved, self.tmp = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


_ROUTE = re.compile(r"\[route\] variant (\d+) rest (\d) spread (\d) fold (\d) gfold (\d) table_ok \d+ perm_ok \d+ coarse (\d) n_sigs (\d+) Cn_t (\d+)")


def run_device(inp, env):
    """One context: the segmented batch (+ caller ranks), results, risk flags, plans at inp.caps, what ran.  None: refused at run time
    (SIMON_ESTATE: the all-feature kernel takes prefix scenarios only).  Any other refusal raises."""
    env = dict(inp.env, **env, SIMON_DEBUG_ROUTE="1")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with _Stderr() as err, capi.Context(0) as ctx:        # (the route lines of the load calls and of the run)
            ctx.load_problem(inp.prob)
            ctx.load_scenarios(inp.scen, inp.orders)
            ctx.set_scenario_segments(inp.seg_start, inp.counts)
            if inp.ranks is not None:
                ctx.set_node_ranks(inp.ranks)
            try:
                ctx.run_loaded(True, inp.want_gpu)
                refused = False
            except capi.SimonError as e:
                if getattr(e, "code", None) != capi.ESTATE:
                    raise
                refused = True
            if refused:
                return None
            res = ctx.fetch(True, inp.want_gpu)
            out = SimpleNamespace(placement=res.placement, unscheduled=res.unscheduled, used_cpu=res.used_cpu, used_mem=res.used_mem,
                                  gpu_slices=res.gpu_slices if inp.want_gpu else None,
                                  preempt_risk=ctx.fetch_preempt_risk() if inp.prob.priority is not None else None)
            out.plans = []
            for cap in inp.caps:
                plan, _ = ctx.min_plan_vg(cap, cap, 100)
                out.plans.append((int(plan.found), int(plan.scenario) if plan.found else -1))
            st = ctx.stats()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m = _ROUTE.search(err.text)
    out.route = dict(variant=st.kernel_variant, generation=st.kernel_generation, wg=st.workgroup_size, lds=int(st.lds_bytes), env=env)
    if m:
        out.route.update(rest=int(m[2]), spread=int(m[3]), fold=int(m[4]), gfold=int(m[5]), coarse=int(m[6]), n_sigs=int(m[7]), Cn_t=int(m[8]))
    return out


def compare(inp, ref, out):
    """Names of the fields in which a device run differs from the reference (with the first scenario that differs)."""
    bad = []
    for name in ("placement", "unscheduled", "used_cpu", "used_mem", "gpu_slices", "preempt_risk"):
        a, b = getattr(ref, name), getattr(out, name)
        if a is None:
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or not (a.astype(np.int64) == b.astype(np.int64)).all():
            diff = np.flatnonzero((a.astype(np.int64) != b.astype(np.int64)).reshape(len(a), -1).any(1)) if a.shape == b.shape else [-1]
            bad.append(f"{name}@{int(diff[0])}")
    for cap, got in zip(inp.caps, out.plans):
        if got != plan_of(inp, ref, cap):
            bad.append(f"plan@{cap}:{got}!={plan_of(inp, ref, cap)}")
    return bad


def host_device(inp):
    """The reference in the device's place (no GPU): what one_case compares when BOTH sides are the oracle -- with `inp` perturbed, the
    harness's own sensitivity (tests/test_mix_host.py)."""
    out = reference(inp)
    out.plans = [plan_of(inp, out, cap) for cap in inp.caps]
    out.route = dict(variant=0, generation=0, wg=0, lds=0, env={})
    return out


def seg_lengths(inp):
    return np.append(inp.seg_start[1:], inp.prob.n_nodes) - inp.seg_start


def n_segments(inp):
    """Segments that hold a node (an empty one changes nothing: a batch with ONE non-empty segment is still a prefix batch in disguise)."""
    return int((seg_lengths(inp) > 0).sum())


def slice_conditions(inp, ref):
    """What a case of the deterministic slice must offer: two or more non-empty segments of which some scenario holds a strict, non-zero
    prefix (so that a node is absent BETWEEN present ones); on the reference's results, some scenario places a pod on a segment node and,
    with gates, some pod is gated out of one scenario and placed in another.  Returns the list of conditions it misses."""
    missing = []
    if ((inp.counts > 0) & (inp.counts < seg_lengths(inp)[None])).any(0).sum() < 2:
        missing.append("fewer than two segments with a strict, non-zero prefix in some scenario")
    if not (ref.placement >= inp.F).any():
        missing.append("no pod on a segment node")
    if "gates" in inp.feat and not ((ref.placement == capi.GATED).any(0) & (ref.placement >= 0).any(0)).any():
        missing.append("no pod gated out of one scenario and placed in another")
    return missing


def families(inp, outs):
    """Route families the runs of one case took, from simon_get_stats and the library's route line."""
    fam = set()
    for i, out in enumerate(outs):
        r = out.route
        if r["variant"] != capi.KERNEL_NARROW_CACHE:
            continue
        gen, cn = r["generation"], r.get("Cn_t", 0)
        other = [o for o in outs if o is not out and o.route["env"].get("SIMON_LDS_WS") not in (None, r["env"].get("SIMON_LDS_WS"))]
        in_lds = r["env"].get("SIMON_LDS_WS") == "1" and bool(other) and r["lds"] > other[0].route["lds"]
        if gen == 4 and cn <= 128:
            fam.add("gen4_lds" if in_lds else "gen4_hbm")
        if gen == 6:
            fam.add("gen6_lds" if in_lds else "gen6_hbm")
        if gen == 5:
            fam.add("gen5")
        if cn > 128:
            fam.add("classes_129_256")
        if 64 < cn <= 128 and gen in (6, 7):
            fam.add("classes_65_128_gen6or7")
        if r.get("gfold"):
            fam.add("gpu_fold")
        if gen == 7:
            fam.add("gen7_team" if r["wg"] == 256 else "gen7_wave")
        if r.get("rest") and r.get("spread"):
            fam.add("rest_and_spread")
        if r.get("n_sigs", 0) > 128:
            fam.add("sigs_over_128")
        if inp.ranks is not None:
            fam.add("caller_ranks")
        if n_segments(inp) > 1:
            fam.add("multi_segment")
    return fam


def one_case(case, device=run_device):
    if case >= K8S_FIRST:
        return one_case_k8s(case)
    inp = draw(case)
    ref = reference(inp)
    outs, bad = [], []
    for env in inp.runs:
        out = device(inp, env)
        if out is None:
            continue
        outs.append(out)
        bad += [f"{b} {sorted(env.items())}" for b in compare(inp, ref, out)]
    info = dict(case=case, kind=inp.kind, sub=inp.sub, N=inp.N, P=inp.P, S=inp.S, segs=n_segments(inp), F=inp.F, feat=sorted(inp.feat),
                classes=inp.n_node_classes, pod_classes=inp.n_pod_classes, ranks=inp.ranks is not None, caps=inp.caps,
                unscheduled=int(ref.unscheduled.sum()), refused=not outs, families=sorted(families(inp, outs)), slice_missing=slice_conditions(inp, ref),
                routes=[(o.route["variant"], o.route["generation"], o.route["wg"]) for o in outs],
                detail=[(o.route["lds"], o.route.get("Cn_t"), o.route.get("n_sigs"), o.route.get("rest"), o.route.get("spread"), o.route.get("gfold")) for o in outs], bad=bad)
    return not bad, info


# ---- k8s objects through sweep_mix -----------------------------------------------------------------------------------------------
class _Recording(sim.HipEngine):
    def run(self, prob, scen, orders, **kw):
        self.seen = (prob, scen, kw)
        self.out = super().run(prob, scen, orders, **kw)
        return self.out


def draw_k8s(case):
    rng = np.random.default_rng(91000 + case)
    zones = ("za", "zb", "zc")[:1 + case % 3]
    n_types = int(rng.integers(1, 5))
    cluster, apps, types = MU.random_zoned(case, n_nodes=int(rng.integers(4, 15)), n_types=n_types, zones=zones)
    # Kept to what the score-table kernel takes (the all-feature kernel takes no segments; measured on campaigns of this band): no
    # preferred pod (anti-)affinity (two clusters in three that carried it fell back), and no required node affinity in a cluster with a
    # DoNotSchedule spread constraint (all 45 of 400 clusters that still fell back had such a constraint, 32 of them that affinity too:
    # the constraint's eligible nodes are then no longer "every labelled node")
    specs = [w["spec"]["template"]["spec"] for app in apps for ws in app.resource.values() for w in ws]
    hard = any(c["whenUnsatisfiable"] == "DoNotSchedule" for sp in specs for c in sp.get("topologySpreadConstraints", []))
    for sp in specs:
        aff = sp.get("affinity", {})
        for k in ("podAffinity", "podAntiAffinity"):
            aff.get(k, {}).pop("preferredDuringSchedulingIgnoredDuringExecution", None)
        if hard:
            aff.get("nodeAffinity", {}).pop("requiredDuringSchedulingIgnoredDuringExecution", None)
    grid = [sorted(set(rng.integers(0, 4, int(rng.integers(1, 4))).tolist())) for _ in range(n_types)]
    return SimpleNamespace(case=case, cluster=cluster, apps=apps, types=types, grid=grid, zones=zones)


def reference_k8s(inp):
    """Per mix of the grid: Simulate() of that mix ALONE on the oracle engine, by object names; and sweep_mix on the oracle engine."""
    import itertools
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", sim.MixFallbackWarning)
        sw = sim.sweep_mix(inp.cluster, inp.apps, inp.types, inp.grid, engine=MU.OracleEngine())
    where = []
    for mix in itertools.product(*inp.grid):
        res, w, _ = MU.mix_answer(inp.cluster, inp.apps, inp.types, mix)
        where.append((w, len(res.unscheduled_pods)))
    return SimpleNamespace(sweep=sw, where=where)


def names_of_row(flat, row):
    """{(namespace, pod name): node name or None} of one placement row over the pool problem (gated pods: not part of the mix)."""
    return {tuple(flat.pod_refs[pid]): (None if j == capi.UNSCHEDULED else flat.node_names[j]) for pid, j in enumerate(np.asarray(row).tolist())
            if j != capi.GATED}


def pool_flat(inp):
    base = list(inp.cluster.get("Node", []))
    pool = base + [n for nn in sim.mix_fake_nodes(inp.types, [max(g) for g in inp.grid]) for n in nn]
    pods, gates = sim.build_stream(inp.cluster, inp.apps, pool, len(base))
    return fl.flatten(pool, pods, inp.cluster.get("Service", []), inp.cluster.get("ReplicaSet", []), inp.cluster.get("StatefulSet", []), gates,
                      storage_classes=sim._storage_classes(inp.cluster, inp.apps))


def compare_k8s(inp, ref, hip, placement):
    bad = []
    if list(hip.counts) != list(ref.sweep.counts):
        return ["counts"]
    for name in ("unscheduled", "cpu_pct", "mem_pct", "vg_pct", "best", "cost"):
        if getattr(hip, name) != getattr(ref.sweep, name):
            bad.append(name)
    flat = pool_flat(inp)
    for s, mix in enumerate(hip.counts):
        w, n_uns = ref.where[s]
        if names_of_row(flat, placement[s]) != w or hip.unscheduled[s] != n_uns:
            bad.append(f"pods@{mix}")
    return bad


def one_case_k8s(case, engine=None):
    import warnings
    inp = draw_k8s(case)
    ref = reference_k8s(inp)
    eng = engine or _Recording()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", sim.MixFallbackWarning)
        hip = sim.sweep_mix(inp.cluster, inp.apps, inp.types, inp.grid, engine=eng)
    info = dict(case=case, kind="k8s", zones=len(inp.zones), types=len(inp.types), grid=inp.grid, nodes=len(inp.cluster["Node"]),
                unscheduled=int(sum(ref.sweep.unscheduled)), refused=not hip.batched, families=[], bad=[])
    if not hip.batched:                # visible fallback (every mix as its own problem): counted as refused, its answers compared all the same --
        info["feat"] = [hip.fallback]  # aggregates of every mix, and the pods of the best mix by object names
        bad = [name for name in ("counts", "unscheduled", "cpu_pct", "mem_pct", "vg_pct", "best", "cost") if getattr(hip, name) != getattr(ref.sweep, name)]
        if hip.best is not None and not bad:
            got = {(p["metadata"].get("namespace", ""), p["metadata"]["name"]): st["node"]["metadata"]["name"] for st in hip.result.node_status for p in st["pods"]}
            if got != {k: v for k, v in ref.where[list(hip.counts).index(hip.best)][0].items() if v is not None}:
                bad.append(f"pods@{hip.best}")
        info["bad"] = bad
        return not bad, info
    st = eng.last_stats
    info["routes"] = [(st.kernel_variant, st.kernel_generation, st.workgroup_size)] if st is not None else []
    info["families"] = ["k8s_zones_%d" % len(inp.zones)] + (["caller_ranks"] if eng.seen[2].get("node_ranks") is not None else []) + \
        (["multi_segment"] if sum(max(g) > 0 for g in inp.grid) > 1 else [])
    info["bad"] = compare_k8s(inp, ref, hip, eng.out.placement)
    return not info["bad"], info


REFUSED_CAP = 0.10      # share of a band's cases the library may refuse at run time (or sweep_mix may run one by one) before the
#                         campaign fails: the regime must not hide behind refusals


def perturb_main():
    """python tests/fuzz_mix.py --perturb: the device is handed VALID inputs that differ from the reference's in one small way (perturb),
    over the array-level cases of the slice; prints which cases notice.  Nothing here can fault a device: every input passes the validator."""
    kinds = ("count", "rank", "gate")
    caught, tried = {h: [] for h in kinds}, {h: 0 for h in kinds}
    for case in sorted(c for c in SLICE if c < K8S_FIRST):
        inp = draw(case)
        ref = reference(inp)
        for how in kinds:
            other = perturb(inp, how)
            if other is None:
                continue
            tried[how] += 1
            outs = [out for out in (run_device(other, env) for env in inp.runs) if out is not None]
            if any(compare(inp, ref, out) for out in outs):
                caught[how].append(case)
    print(f"fuzz_mix --perturb: cases that noticed / cases that offered the change: {({h: (len(caught[h]), tried[h]) for h in kinds})}; noticed by {caught}")
    return 0 if all(caught[h] for h in kinds) else 1


def main():
    if "--perturb" in sys.argv:
        return perturb_main()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_cases = int(args[0]) if len(args) > 0 else 40
    first = int(args[1]) if len(args) > 1 else 0
    bad = refused = 0
    fam, multi, refused_feat = {}, {}, {}
    for case in range(first, first + n_cases):
        ok, info = one_case(case)
        if "--verbose" in sys.argv:
            print("CASE", info, flush=True)
        for f in info["families"]:
            fam[f] = fam.get(f, 0) + 1
            if "multi_segment" in info["families"]:
                multi[f] = multi.get(f, 0) + 1
        if info["refused"]:
            refused += 1
            for f in info.get("feat", []):
                refused_feat[f] = refused_feat.get(f, 0) + 1
        if not ok:
            bad += 1
            print("MISMATCH", info, flush=True)
    shown = {f: fam.get(f, 0) for f in (FAMILIES if first < K8S_FIRST else sorted(fam))}     # (a family no case reached shows as 0)
    print(f"fuzz_mix: {n_cases} cases from {first}, families {shown} (with two or more segments: {[multi.get(f, 0) for f in shown]}), refused {refused} "
          f"(features of the refused: {dict(sorted(refused_feat.items()))}), mismatches {bad}")
    if refused > REFUSED_CAP * n_cases:
        print(f"fuzz_mix: refused {refused} of {n_cases}: over the cap of {REFUSED_CAP:.0%}")
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

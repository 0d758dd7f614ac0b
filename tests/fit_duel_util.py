"""Fit duels on 31-bit quantities for the score table's mask rows (tests only): seeded problems in which ONE probe pod is admitted to exactly
three nodes by the static mask -- `near` (best cpu + memory score) misses the probed quantity by ONE unit, `exact` (second best) fits with
nothing left, `fallback` (worst) fits with room.  The exact answer is `exact`; an over-admitting fit sends the pod to `near`, an
over-rejecting one to `fallback`.  The cpu and memory sizes are plain and the three totals about 30 points apart: the score arithmetic is
tests/duel_util.py's subject, not this module's.  (With Features.anti the mask admits a fourth node, `blocked`: best score of all and room
for everything, but a guard pod that matches the hostname-key term of the probe's required anti-affinity landed there first -- the term's
rows share the workspace and the `bit` of the GPU and extra-resource rows.)

Three parts, in the shape of tests/duel_util.py:
  * the exact reference: a scheduler over a capi.Problem in Python integers (schedule) that takes the three fit functions of the mask rows
    as a parameter (Fit): xres (simon_table.hip: xres_fits_t), gpu_fits (gpu_fits_t), gpu_commit (gpu_commit_t);
  * near-miss models: Fit objects that replace ONE of the three the way a subtly wrong kernel or staging would;
  * the generator: duels are small stand-alone specifications (Duel), each accepted only if every model loses it exactly when the duel's
    kind is among the model's kinds (checked on the duel's own three-node problem); assemble() joins them into one problem, build() adds
    orders and scenarios and asserts the domain that rest_supported / gfold_supported (simon_hip.hip) ask for, restated in check_domain().

Flavours: "initial" -- the fragile state comes from init_req_eph / init_scalar_req / init_gpu_used (the prologue's rows); "refresh" -- it
is reached when a setter pod of the same stream, admitted to that one node only and with a request signature of its own, lands first
(rest_assume_store, or the fold's refresh).  `near` and `exact` both get a setter.  An order permutes whole duels; a duel's pods stay
together and in their order (guard, setters, probe, follow-up).

Kinds (magnitudes 2^27 .. 2^31 - 1: one unit lies below fp32's resolution; quantities are random, so every gcd is 1 unless said otherwise):
  eph_edge          alloc == used + req on `exact`, alloc + 1 == used + req on `near`; the first duel's `exact` has alloc == 2^31 - 1
  eph_wrap          `near` has used + req in [2^31, 2^32) with both operands below 2^31
  eph_gcd:edge/wrap the same two in a problem whose every ephemeral quantity is a multiple of g = 3 * 2^10: raw values beyond 2^32 (on
                    `near` of the edge form alloc == -1 (mod 2^22): where a sum of raw values cut to 32 bits wraps)
  scalar_edge:k / scalar_wrap:k   the same two on extended resource k = 0 .. 3; the pod names only that one, the other three are full
                    (used == alloc) on all three nodes
  gpu_one_edge      count 1: the only device with room has idle == req on `exact`, req - 1 on `near`; the first duel's total is 2^31 - 1
  gpu_total_floor   the same with gpu_mem_total not divisible by gpu_cnt: the edge sits on the floored per-device total
  gpu_tightest      count 1: on `exact` device 0 has room for the follow-up's larger request exactly, devices 1 and 2 have idle == req:
                    device 1 must be booked (tightest, lowest id on equal idle); the follow-up pod, admitted to `exact` alone, fits device
                    0 only if it was left alone; gpu_slices tell devices 1 and 2 apart
  gpu_multi:n       count n = 2 .. 4: on `exact` the sum of floor(idle / req) is n with nothing left; on `near` the summed idle memory is
                    (n + 1) req - 2 but the slices are n - 1
  gpu_overbooked    on `near` init_gpu_used of the one device that is not full is one unit ABOVE the per-device total (rest_supported
                    compares neither with the other); an over-booked device holds nothing.  The state cannot be reached by a booking: in
                    the refresh flavour only `exact` gets a setter.

Models (name -> the kinds it loses; it wins every other duel -- tests/test_fit_duels_host.py):
  sum_i32 (signed 32-bit req + used), via_fp32, fit_strict (`>` for `>=`), fit_lenient (admits at one unit short), trunc32_no_gcd (raw
  values cut to 32 bits, no gcd), named_always (un-named components compared with the neighbouring component's request) replace xres;
  gpu_via_fp32, gpu_fit_strict, gpu_fit_lenient, idle_unsigned (unsigned tot - used), gpu_pooled (summed idle memory), gpu_total_ceil
  replace gpu_fits; gpu_first_fit and gpu_tie_last replace gpu_commit.
Dropped: gpu_floor_late ("divides the node total after subtracting") is dead.  With total = cnt T + rem, 0 <= rem < cnt, the late form asks
(total - cnt used) / cnt >= req, i.e. T - used - req >= -rem / cnt > -1, which for integers is T - used - req >= 0: the floored form, on every
input; the same holds slice by slice.  gpu_total_ceil (per-device total rounded UP) takes its place as the model gpu_total_floor is for,
and gpu_tie_last (the LAST device among equally tight ones) is added for the tie rule of gpu_tightest.  No kind is dropped.
gpu_via_fp32 and gpu_fit_strict are listed for every GPU kind: each kind has an exact fit on `exact` (gpu_tightest: the follow-up's).

Fixtures (fixture(name), cached, never modified by a test; at most 73 nodes and 73 pods, a pod class and so a signature per pod):
xres_initial / xres_refresh (ephemeral storage + four extended resources), ephgcd_initial / ephgcd_refresh (the gcd is a property of the
whole problem, so eph_gcd has problems of its own), gpu_initial / gpu_refresh (at most 32 distinct GPU requests: the fold is eligible),
mixed_refresh (GPU, extra resources and the anti-affinity term together), xres_70classes / gpu_70classes (every node a capacity shape of
its own: 72 internal node classes), xres_spread / gpu_spread (one soft PodTopologySpread constraint on the hostname key, matched by probes
and follow-ups only, so every count is 0 when a probe is scored), and edge_{eph,scalar,gpu}_{inside,outside}: six duels plus one node
nobody is admitted to whose quotient is 2^31 - 1 / 2^31."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import duel_util
from open_simulator_amd import capi
from open_simulator_amd.gomath import spread_log_table

LIM31 = 1 << 31
M32 = (1 << 32) - 1
EPH_G = 3 << 10
MAX_XRES_SIGS = 32            # simon_table.h: kTableMaxXres
MAX_GPU_SIGS = 32             # simon_table.h: kTableMaxGpuSigs
K_SCALAR = capi.MAX_SCALAR
DEV = capi.MAX_GPU_DEV


# ---- the three fit functions: exact reference ---------------------------------------------------------------------------------------
def xres_exact(req, used, alloc, g):
    """fitsRequest's ephemeral-storage and extended-resource checks (fit.go:264-299): component 0 whatever the request, an extended
    resource only when the pod names it.  req / used / alloc: [5] raw values; g: [5] the gcd each was staged on (unused here)."""
    if alloc[0] < req[0] + used[0]:
        return False
    return not any(req[r] != 0 and alloc[r] < req[r] + used[r] for r in range(1, 5))


def _idle_exact(used, cnt, total):
    tot = total // cnt
    return [tot - used[d] for d in range(min(cnt, DEV))]


def _slices(idle, req, num, ge):
    """two-pointer greedy (gpunodeinfo.go:268-287): device ids, one per slice, or [] when fewer than num"""
    ids = []
    for d, room in enumerate(idle):
        while ge(room, req) and len(ids) < num:
            ids.append(d)
            room -= req
    return ids if len(ids) == num else []


_GE = lambda idle, req: idle >= req


def gpu_fits_exact(used, cnt, total, req, num, idle_of=_idle_exact, ge=_GE):
    if req <= 0 or num <= 0 or cnt <= 0:
        return False
    idle = idle_of(used, cnt, total)
    if num == 1:
        return any(ge(x, req) for x in idle)
    return bool(_slices(idle, req, num, ge))


def gpu_commit_exact(used, cnt, total, req, num):
    """GpuNodeInfo.AllocateGpuId (gpunodeinfo.go:232-290): the device ids Reserve books, [] when none"""
    if req <= 0 or num <= 0 or cnt <= 0:
        return []
    idle = _idle_exact(used, cnt, total)
    if num == 1:
        cand = -1
        for d, x in enumerate(idle):
            if x >= req and (cand < 0 or x < idle[cand]):
                cand = d
        return [cand] if cand >= 0 else []
    return _slices(idle, req, num, _GE)


@dataclass(frozen=True)
class Fit:
    name: str
    xres: callable = xres_exact
    gpu_fits: callable = gpu_fits_exact
    gpu_commit: callable = gpu_commit_exact


EXACT = Fit("exact")


# ---- near-miss models ------------------------------------------------------------------------------------------------------------------
def _staged(v, g):
    assert all(x % gi == 0 for x, gi in zip(v, g)), (v, g)
    return [x // gi for x, gi in zip(v, g)]


def _xres_model(short):
    """short(alloc, req, used, r) -> the component does not fit; on staged (gcd-normalised) quantities"""
    def fits(req, used, alloc, g):
        q, u, a = _staged(req, g), _staged(used, g), _staged(alloc, g)
        return not short(a[0], q[0], u[0]) and not any(q[r] != 0 and short(a[r], q[r], u[r]) for r in range(1, 5))
    return fits


def _i32(x):
    return (x + LIM31) % (1 << 32) - LIM31


_F = np.float32
xres_sum_i32 = _xres_model(lambda a, q, u: a < _i32(q + u))
xres_via_fp32 = _xres_model(lambda a, q, u: bool(_F(a) < _F(q) + _F(u)))
xres_strict = _xres_model(lambda a, q, u: q != 0 and a <= q + u)          # (a zero request of component 0 is left alone: the model is `>` for `>=`
xres_lenient = _xres_model(lambda a, q, u: a + 1 < q + u)                 # on what a pod asks for)


def xres_trunc32_no_gcd(req, used, alloc, g):
    """raw values cut to 32 bits, the sum in 32 bits too (with gcd 1 and quantities below 2^31 this is the exact compare)"""
    q, u, a = ([x & M32 for x in v] for v in (req, used, alloc))
    return not a[0] < ((q[0] + u[0]) & M32) and not any(q[r] != 0 and a[r] < ((q[r] + u[r]) & M32) for r in range(1, 5))


def xres_named_always(req, used, alloc, g):
    q, u, a = _staged(req, g), _staged(used, g), _staged(alloc, g)
    if a[0] < q[0] + u[0]:
        return False
    for r in range(1, 5):
        eff = q[r] if q[r] != 0 else q[1 + r % 4]
        if eff != 0 and a[r] < eff + u[r]:
            return False
    return True


def _idle_fp32(used, cnt, total):
    tot = _F(total // cnt)
    return [tot - _F(used[d]) for d in range(min(cnt, DEV))]


def _idle_unsigned(used, cnt, total):
    return [x & M32 for x in _idle_exact(used, cnt, total)]


def _idle_ceil(used, cnt, total):
    tot = -(-total // cnt)
    return [tot - used[d] for d in range(min(cnt, DEV))]


def _gpu_model(idle_of=_idle_exact, ge=_GE):
    return lambda used, cnt, total, req, num: gpu_fits_exact(used, cnt, total, req, num, idle_of, ge)


def gpu_fits_pooled(used, cnt, total, req, num):
    if req <= 0 or num <= 0 or cnt <= 0:
        return False
    return sum(max(x, 0) for x in _idle_exact(used, cnt, total)) >= num * req


def _commit_pick(last):
    def commit(used, cnt, total, req, num):
        if num != 1 or req <= 0 or cnt <= 0:
            return gpu_commit_exact(used, cnt, total, req, num)
        idle = _idle_exact(used, cnt, total)
        room = [d for d, x in enumerate(idle) if x >= req]
        if not room:
            return []
        if not last:
            return [room[0]]                                              # first fit
        tight = min(idle[d] for d in room)
        return [max(d for d in room if idle[d] == tight)]                 # tightest fit, HIGHEST id on ties
    return commit


XRES_KINDS = ("eph_edge", "eph_wrap", "scalar_edge", "scalar_wrap")
GCD_KINDS = ("eph_gcd:edge", "eph_gcd:wrap")
GPU_KINDS = ("gpu_one_edge", "gpu_total_floor", "gpu_tightest", "gpu_multi", "gpu_overbooked")
# model -> (Fit, the kinds whose every duel it loses)
MODELS = {
    "sum_i32": (Fit("sum_i32", xres=xres_sum_i32), ("eph_wrap", "scalar_wrap", "eph_gcd:wrap")),
    "via_fp32": (Fit("via_fp32", xres=xres_via_fp32), ("eph_edge", "scalar_edge", "eph_gcd:edge")),
    "fit_strict": (Fit("fit_strict", xres=xres_strict), XRES_KINDS + ("eph_gcd",)),
    "fit_lenient": (Fit("fit_lenient", xres=xres_lenient), ("eph_edge", "scalar_edge", "eph_gcd:edge")),
    "trunc32_no_gcd": (Fit("trunc32_no_gcd", xres=xres_trunc32_no_gcd), ("eph_gcd",)),
    "named_always": (Fit("named_always", xres=xres_named_always), ("scalar_edge", "scalar_wrap")),
    "gpu_via_fp32": (Fit("gpu_via_fp32", gpu_fits=_gpu_model(_idle_fp32, lambda i, r: bool(i >= _F(r)))), GPU_KINDS),
    "gpu_fit_strict": (Fit("gpu_fit_strict", gpu_fits=_gpu_model(ge=lambda i, r: i > r)), GPU_KINDS),
    "gpu_fit_lenient": (Fit("gpu_fit_lenient", gpu_fits=_gpu_model(ge=lambda i, r: i + 1 >= r)), ("gpu_one_edge", "gpu_total_floor", "gpu_tightest", "gpu_multi")),
    "idle_unsigned": (Fit("idle_unsigned", gpu_fits=_gpu_model(_idle_unsigned)), ("gpu_overbooked",)),
    "gpu_pooled": (Fit("gpu_pooled", gpu_fits=gpu_fits_pooled), ("gpu_multi",)),
    "gpu_total_ceil": (Fit("gpu_total_ceil", gpu_fits=_gpu_model(_idle_ceil)), ("gpu_total_floor",)),
    "gpu_first_fit": (Fit("gpu_first_fit", gpu_commit=_commit_pick(False)), ("gpu_tightest",)),
    "gpu_tie_last": (Fit("gpu_tie_last", gpu_commit=_commit_pick(True)), ("gpu_tightest",)),
}


def targets(kind):
    """the models that must lose a duel of this kind"""
    return [m for m, (_, kinds) in MODELS.items() if kind in kinds or kind.split(":")[0] in kinds]


# ---- the reference scheduler --------------------------------------------------------------------------------------------------------------
def staging_gcds(prob):
    """the gcd of the ephemeral quantities as rest_supported takes it (allocatable, initial, requests), 1 for every extended resource"""
    g = 0
    for arr in (prob.alloc_eph, prob.init_req_eph, prob.req_eph):
        if arr is not None:
            g = math.gcd(g, int(np.gcd.reduce(np.asarray(arr, np.int64))))
    return [g or 1, 1, 1, 1, 1]


def schedule(prob, order, n_nodes, fit=EXACT):
    """One scenario, one pod at a time (oracle/simon_oracle.c: run_scenario, schedule_one, filter_node, add_pod) for the features these
    problems hold: static masks, gates, cpu / memory / pods, ephemeral storage and extended resources, Open-Gpu-Share, required
    anti-affinity and soft PodTopologySpread on a key that gives every node its own domain; a flat Simon table.  The three fit functions
    come from `fit`.  Returns (placement [P], unscheduled, used_cpu, used_mem, gpu_slices [P]) in Python integers."""
    N, P = prob.n_nodes, prob.n_pods
    I = lambda a, n: [int(v) for v in a] if a is not None else [0] * n
    a_c, a_m, a_p = I(prob.alloc_cpu, N), I(prob.alloc_mem, N), I(prob.alloc_pods, N)
    rq_c, rq_m, npods = I(prob.init_req_cpu, N), I(prob.init_req_mem, N), I(prob.init_npods, N)
    assert prob.preset_node is None and all((getattr(prob, "init_nz_" + r) == getattr(prob, "init_req_" + r)).all() and
                                            (getattr(prob, "nz_" + r) == getattr(prob, "req_" + r)).all() for r in ("cpu", "mem"))
    K = 0 if prob.scalar_alloc is None else prob.scalar_alloc.shape[0]
    assert K in (0, K_SCALAR)
    alloc_x = [[int(prob.alloc_eph[j]) if prob.alloc_eph is not None else 0] + [int(prob.scalar_alloc[k, j]) for k in range(K)] + [0] * (4 - K) for j in range(N)]
    used_x = [[int(prob.init_req_eph[j]) if prob.init_req_eph is not None else 0] + [int(prob.init_scalar_req[k, j]) if prob.init_scalar_req is not None else 0 for k in range(K)] + [0] * (4 - K)
              for j in range(N)]
    req_x = [[int(prob.req_eph[p]) if prob.req_eph is not None else 0] + [int(prob.scalar_req[k, p]) if prob.scalar_req is not None else 0 for k in range(K)] + [0] * (4 - K) for p in range(P)]
    g = staging_gcds(prob)
    g_cnt, g_tot = I(prob.gpu_cnt, N), I(prob.gpu_mem_total, N)
    g_used = [[int(v) for v in prob.init_gpu_used[j]] if prob.init_gpu_used is not None else [0] * DEV for j in range(N)]
    p_gm, p_gn = I(prob.gpu_mem, P), [min(v, 64) for v in I(prob.pod_gpu_cnt, P)]
    p_rc, p_rm, pcls, gate = I(prob.req_cpu, P), I(prob.req_mem, P), I(prob.pod_class, P), (I(prob.gate_node, P) if prob.gate_node is not None else [-1] * P)
    adm = duel_util.admitted_nodes(prob)
    T = 0 if prob.term_topo_key is None else len(prob.term_topo_key)
    assert T == 0 or (np.asarray(prob.topo_dom)[np.asarray(prob.term_topo_key)] == np.arange(N)).all()    # every term on a node-level key
    lst = lambda off, idx, c: [int(t) for t in idx[off[c]:off[c + 1]]] if off is not None and T else []
    cnt_match, cnt_owner = [[0] * N for _ in range(T)], [[0] * N for _ in range(T)]
    place, slices, unsched = [capi.UNSCHEDULED] * P, [0] * P, 0
    for p in (int(x) for x in order):
        if gate[p] >= n_nodes:
            place[p] = capi.GATED
            continue
        c = pcls[p]
        anti, match = lst(prob.anti_off, prob.anti_idx, c), lst(prob.match_off, prob.match_idx, c)
        soft = lst(prob.spread_soft_off, prob.spread_soft_idx, c)
        skew = lst(prob.spread_soft_off, prob.spread_soft_skew, c)
        any_x = any(req_x[p])
        feas = []
        for j in adm[c]:
            if j >= n_nodes or npods[j] + 1 > a_p[j]:
                continue
            if not (p_rc[p] == 0 and p_rm[p] == 0 and not any_x):
                if a_c[j] < rq_c[j] + p_rc[p] or a_m[j] < rq_m[j] + p_rm[p] or not fit.xres(req_x[p], used_x[j], alloc_x[j], g):
                    continue
            if any(cnt_match[t][j] > 0 for t in anti) or any(cnt_owner[t][j] > 0 for t in match):
                continue
            if p_gm[p] > 0 and (g_tot[j] < p_gm[p] or not fit.gpu_fits(g_used[j], g_cnt[j], g_tot[j], p_gm[p], p_gn[p])):
                continue
            feas.append(j)
        if not feas:
            unsched += 1
            continue
        best = feas[0]
        if len(feas) > 1:
            pts = {}
            if soft:                                                      # podtopologyspread/scoring.go:60-256, every node labelled
                w = float(prob.spread_log[len(feas)])
                for j in feas:
                    pts[j] = int(sum(float(cnt_match[t][j]) * w + float(sk - 1) for t, sk in zip(soft, skew)))
                lo, hi = min(pts.values()), max(pts.values())
            best_total = -1
            for j in feas:
                total = duel_util.laba(duel_util.EXACT, rq_c[j] + p_rc[p], a_c[j], rq_m[j] + p_rm[p], a_m[j])
                if soft:
                    total += 2 * (100 if hi == 0 else 100 * (hi + lo - pts[j]) // hi)
                if total > best_total:
                    best, best_total = j, total
        j = best
        rq_c[j] += p_rc[p]; rq_m[j] += p_rm[p]; npods[j] += 1
        used_x[j] = [u + q for u, q in zip(used_x[j], req_x[p])]
        for t in match:
            cnt_match[t][j] += 1
        for t in anti:
            cnt_owner[t][j] += 1
        if p_gm[p] > 0:
            for d in fit.gpu_commit(g_used[j], g_cnt[j], g_tot[j], p_gm[p], p_gn[p]):
                g_used[j][d] += p_gm[p]
                slices[p] += 1 << (8 * d)
        place[p] = j
    return place, unsched, sum(rq_c[:n_nodes]), sum(rq_m[:n_nodes]), slices


# ---- duels ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class DNode:
    role: str                      # near / exact / fallback / blocked
    frac: float                    # share of cpu and memory in use at the start
    x_alloc: list                  # [5] ephemeral storage (in units of the problem's g) + 4 extended resources
    x_used: list
    cnt: int = 0
    total: int = 0
    g_used: list = field(default_factory=lambda: [0] * DEV)


@dataclass
class DPod:
    role: str                      # guard / setter / probe / follow
    admit: list                    # local node indices
    x_req: list = field(default_factory=lambda: [0] * 5)
    gpu_mem: int = 0
    gpu_cnt: int = 0


@dataclass
class Duel:
    kind: str
    nodes: list
    pods: list

    @property
    def base_kind(self):
        return self.kind.split(":")[0]

    def local(self, role):
        return [i for i, n in enumerate(self.nodes) if n.role == role][0]


@dataclass
class Pools:
    """the few request values a problem draws from: at most 32 distinct extra-resource requests and 32 distinct GPU requests"""
    x_edge: dict
    x_wrap: dict
    x_set: dict
    g_req: dict
    g_follow: int
    g_set: list


def make_pools(rng):
    R = lambda lo, hi: int(rng.integers(lo, hi)) | 1
    return Pools(x_edge={c: [R(1 << 27, 1 << 29) for _ in range(2 if c == 0 else 1)] for c in range(5)},
                 x_wrap={c: [R(1 << 30, (1 << 30) + (1 << 29)) for _ in range(2 if c == 0 else 1)] for c in range(5)},
                 x_set={c: [R(1 << 24, 1 << 28) for _ in range(2 if c == 0 else 1)] for c in range(5)},
                 g_req={k: [R(1 << 27, 1 << 28 if k in ("gpu_tightest", "gpu_multi") else 1 << 29) for _ in range(2)] for k in GPU_KINDS},
                 # (the last setter request is larger than gpu_tightest's: only such a one can leave two equally tight devices behind)
                 g_follow=R(1 << 28, 1 << 29), g_set=[R(1 << 24, 1 << 27), R(1 << 24, 1 << 27), R(1 << 28, 1 << 29)])


FRAC = {"near": 0.10, "exact": 0.40, "fallback": 0.70, "blocked": 0.02}


def _room_x(rng):
    """a node's extra resources away from the duel: ephemeral storage half used, every extended resource full"""
    a = [int(rng.integers(1 << 29, LIM31)) for _ in range(5)]
    return a, [a[0] // 2] + a[1:]


def _xres_states(rng, form, req, top, g=1):
    """(alloc, used) of near / exact / fallback for one component and one request.  Cutting raw values to 32 bits keeps differences, so it
    moves a one-unit edge only where the cut sum wraps: with g = 3 * 2^10 that is alloc == -1 (mod 2^22), which eph_gcd:edge gives `near`."""
    if form == "edge":
        a = [int(rng.integers(1 << 30, LIM31 - 1)) if g == 1 else (int(rng.integers(1 << 8, 1 << 9)) << 22) - 1, LIM31 - 1 if top else int(rng.integers(1 << 30, LIM31)), int(rng.integers(1 << 30, LIM31))]
        return [(a[0], a[0] + 1 - req), (a[1], a[1] - req), (a[2], a[2] - req - int(rng.integers(1 << 20, 1 << 27)))]
    a0 = int(rng.integers((1 << 30) + (1 << 29), LIM31 - 2))
    a1 = int(rng.integers(req + (1 << 28) + (1 << 20), LIM31))
    a2 = int(rng.integers(req + (1 << 29), LIM31))
    return [(a0, int(rng.integers(max(LIM31 - req, 1 << 29), a0 + 1))), (a1, a1 - req), (a2, a2 - req - int(rng.integers(1 << 20, 1 << 27)))]


def _gpu_states(rng, kind, n, req, follow, top):
    """(cnt, total, used [8]) of near / exact / fallback"""
    out = []
    for role in ("near", "exact", "fallback"):
        cnt = int(rng.integers(3 if kind == "gpu_tightest" else 2 if kind in ("gpu_multi", "gpu_total_floor") else 1, DEV + 1))
        T = LIM31 - 1 if (top and role == "exact") else int(rng.integers((1 << 30) + (1 << 29), LIM31 - 1))
        total = cnt * T + (int(rng.integers(1, cnt)) if kind == "gpu_total_floor" else 0)
        idle = [0] * cnt
        d = int(rng.integers(0, cnt))
        if kind == "gpu_tightest" and role == "exact":
            idle[0], idle[1], idle[2] = follow, req, req
        elif kind == "gpu_multi":
            a = int(rng.integers(1, n))
            d2 = (d + 1 + int(rng.integers(0, cnt - 1))) % cnt
            idle[d], idle[d2] = {"near": (a * req + req - 1, (n - a) * req - 1), "exact": (a * req, (n - a) * req),
                                 "fallback": (n * req + int(rng.integers(1 << 20, 1 << 26)), 0)}[role]
        elif kind == "gpu_overbooked" and role == "near":
            idle[d] = -1
        else:
            idle[d] = {"near": req - 1, "exact": req, "fallback": req + int(rng.integers(1 << 20, 1 << 27))}[role]
        out.append((cnt, total, [T - x for x in idle] + [0] * (DEV - cnt)))
    return out


def _draw(rng, kind, flavour, pools, anti, top):
    base, _, sub = kind.partition(":")
    roles = [("near", "exact", "fallback")[i] for i in rng.permutation(3)]
    if anti:
        roles.insert(int(rng.integers(0, 4)), "blocked")
    nodes, by_role = [], {}
    is_gpu = base.startswith("gpu")
    if is_gpu:
        n = int(sub) if base == "gpu_multi" else 1
        req = int(rng.choice(pools.g_req[base]))
        states = dict(zip(("near", "exact", "fallback"), _gpu_states(rng, base, n, req, pools.g_follow, top)))
    else:
        comp = int(sub) + 1 if base.startswith("scalar") else 0
        form = sub if base == "eph_gcd" else base.split("_")[1]
        req = int(rng.choice((pools.x_edge if form == "edge" else pools.x_wrap)[comp]))
        states = dict(zip(("near", "exact", "fallback"), _xres_states(rng, form, req, top, EPH_G if base == "eph_gcd" else 1)))
    for role in roles:
        xa, xu = _room_x(rng)
        nd = DNode(role, FRAC[role], xa, xu)
        if role == "blocked":                                             # room for everything: the guard's anti-affinity term alone keeps the probe off
            nd.x_alloc = [LIM31 - 1 - int(rng.integers(0, 1 << 20)) for _ in range(5)]
            nd.x_used = [int(rng.integers(0, 1 << 20)) for _ in range(5)]
            if is_gpu:
                nd.cnt, nd.total = 4, 4 * (LIM31 - 5)
        elif is_gpu:
            nd.cnt, nd.total, nd.g_used = states[role]
        else:
            nd.x_alloc[comp], nd.x_used[comp] = states[role]
        by_role[role] = len(nodes)
        nodes.append(nd)
    three = sorted(by_role[r] for r in ("near", "exact", "fallback"))
    pods = []
    if anti:
        pods.append(DPod("guard", [by_role["blocked"]]))
        three = sorted(three + [by_role["blocked"]])
    if flavour == "refresh":
        for role in ("near", "exact"):
            nd = nodes[by_role[role]]
            if is_gpu:
                if base == "gpu_overbooked" and role == "near":
                    continue
                done = False
                for s in (int(x) for x in rng.permutation(pools.g_set)):
                    for d in (int(x) for x in rng.permutation(nd.cnt)):
                        pre = list(nd.g_used)
                        pre[d] -= s
                        if pre[d] >= 0 and gpu_commit_exact(pre, nd.cnt, nd.total, s, 1) == [d]:
                            nd.g_used, done = pre, True
                            pods.append(DPod("setter", [by_role[role]], gpu_mem=s, gpu_cnt=1))
                            break
                    if done:
                        break
                if not done:
                    return None
            else:
                s = int(rng.choice(pools.x_set[comp]))
                if nd.x_used[comp] < s:
                    return None
                nd.x_used[comp] -= s
                xr = [0] * 5
                xr[comp] = s
                pods.append(DPod("setter", [by_role[role]], x_req=xr))
    if is_gpu:
        pods.append(DPod("probe", three, gpu_mem=req, gpu_cnt=n))
        if base == "gpu_tightest":
            pods.append(DPod("follow", [by_role["exact"]], gpu_mem=pools.g_follow, gpu_cnt=1))
    else:
        xr = [0] * 5
        xr[comp] = req
        pods.append(DPod("probe", three, x_req=xr))
    return Duel(kind, nodes, pods)


@dataclass
class Features:
    xres: bool = False
    gpu: bool = False
    anti: bool = False
    spread: bool = False
    eph_g: int = 1
    distinct_caps: bool = False


def assemble(duels, ft, seed=0, ballast=None):
    """-> (capi.Problem, first pod of every duel, first node of every duel).  Every pod has a class of its own (its static-mask row) and is gated
    on its duel's last node.  ballast (tests' range edge): (field, value) of one more node nobody is admitted to."""
    rng = np.random.default_rng(seed)
    N = sum(len(d.nodes) for d in duels) + (ballast is not None)
    P = sum(len(d.pods) for d in duels)
    a_c, a_m, i_c, i_m, gate, rq_c, rq_m = [], [], [], [], [], [], []
    mask = np.zeros((P, (N + 63) // 64), np.uint64)
    reason = np.full((P, N), capi.REASON_NODE_AFFINITY, np.uint8)
    x_alloc, x_used, x_req = np.zeros((5, N), np.int64), np.zeros((5, N), np.int64), np.zeros((5, P), np.int64)
    g_cnt, g_tot, g_used, g_mem, g_num = np.zeros(N, np.int32), np.zeros(N, np.int64), np.zeros((N, DEV), np.int64), np.zeros(P, np.int64), np.zeros(P, np.int32)
    match, anti, soft = [], [], []
    pod0, node0 = [], []
    j0 = p0 = 0
    for k, d in enumerate(duels):
        pod0.append(p0); node0.append(j0)
        for i, nd in enumerate(d.nodes):
            j = j0 + i
            shape = j if ft.distinct_caps else k % 8
            a_c.append(64001 + 2 * shape); a_m.append(128001 + 2 * shape)
            i_c.append(int(nd.frac * a_c[-1])); i_m.append(int(nd.frac * a_m[-1]))
            x_alloc[:, j], x_used[:, j] = nd.x_alloc, nd.x_used
            g_cnt[j], g_tot[j], g_used[j] = nd.cnt, nd.total, nd.g_used
        for i, pd in enumerate(d.pods):
            p = p0 + i
            rq_c.append(int(rng.integers(100, 400))); rq_m.append(int(rng.integers(100, 400)))
            gate.append(j0 + len(d.nodes) - 1)
            for loc in pd.admit:
                mask[p, (j0 + loc) // 64] |= np.uint64(1) << np.uint64((j0 + loc) % 64)
                reason[p, j0 + loc] = 0
            x_req[:, p] = pd.x_req
            g_mem[p], g_num[p] = pd.gpu_mem, pd.gpu_cnt
            match.append(([0] if ft.spread and pd.role in ("probe", "follow") else []) + ([int(ft.spread)] if ft.anti and pd.role == "guard" else []))
            anti.append([int(ft.spread)] if ft.anti and pd.role == "probe" else [])
            soft.append([0] if ft.spread and pd.role in ("probe", "follow") else [])
        j0 += len(d.nodes); p0 += len(d.pods)
    if ballast is not None:
        a_c.append(64001); a_m.append(128001); i_c.append(0); i_m.append(0)
        name, value = ballast
        if name == "eph":
            x_alloc[0, N - 1] = value
        elif name == "scalar":
            x_alloc[2, N - 1] = value
        else:
            g_cnt[N - 1], g_tot[N - 1] = 1, value
    prob = capi.Problem(alloc_cpu=np.array(a_c, np.int64), alloc_mem=np.array(a_m, np.int64), alloc_pods=np.full(N, 110, np.int32),
                        node_class=np.zeros(N, np.int32), init_req_cpu=np.array(i_c, np.int64), init_req_mem=np.array(i_m, np.int64),
                        init_nz_cpu=np.array(i_c, np.int64), init_nz_mem=np.array(i_m, np.int64), nz_cpu=np.array(rq_c, np.int64), nz_mem=np.array(rq_m, np.int64),
                        req_cpu=np.array(rq_c, np.int64), req_mem=np.array(rq_m, np.int64), pod_class=np.arange(P, dtype=np.int32),
                        gate_node=np.array(gate, np.int32), n_pod_classes=P, n_node_classes=1, static_mask=mask, static_reason=reason,
                        simon_raw=np.full((P, 1), 57, np.int64))
    if ft.xres:
        prob.alloc_eph, prob.init_req_eph, prob.req_eph = x_alloc[0] * ft.eph_g, x_used[0] * ft.eph_g, x_req[0] * ft.eph_g
        prob.scalar_alloc, prob.init_scalar_req, prob.scalar_req = x_alloc[1:].copy(), x_used[1:].copy(), x_req[1:].copy()
    if ft.gpu:
        prob.gpu_cnt, prob.gpu_mem_total, prob.init_gpu_used, prob.gpu_mem, prob.pod_gpu_cnt = g_cnt, g_tot, g_used, g_mem, g_num
    if ft.anti or ft.spread:
        csr = lambda lists: (np.cumsum([0] + [len(x) for x in lists]).astype(np.int32), np.array([v for x in lists for v in x] or [0], np.int32))
        prob.topo_dom, prob.topo_n_dom, prob.topo_is_hostname = np.arange(N, dtype=np.int32)[None, :], np.array([N], np.int32), np.array([1], np.uint8)
        prob.term_topo_key = np.zeros(int(ft.anti) + int(ft.spread), np.int32)
        prob.match_off, prob.match_idx = csr(match)
        prob.anti_off, prob.anti_idx = csr(anti)
        if ft.spread:
            prob.spread_soft_off, prob.spread_soft_idx = csr(soft)
            prob.spread_soft_skew = np.ones(max(1, int(prob.spread_soft_off[-1])), np.int32)
            prob.spread_log = spread_log_table(N)
    return prob.normalise(), pod0, node0


def duel_result(duel, ft, fit):
    """(placements, gpu_slices) of the duel's pods on the duel's own problem under `fit`"""
    prob, _, _ = assemble([duel], ft)
    place, _, _, _, slices = schedule(prob, range(prob.n_pods), prob.n_nodes, fit)
    return place, slices


def gen_duel(rng, kind, flavour, pools, ft, top=False):
    """One duel that the exact reference decides for `exact` (every pod placed) and that every model loses exactly when it should"""
    for _ in range(4000):
        duel = _draw(rng, kind, flavour, pools, ft.anti, top)
        if duel is None:
            continue
        want = duel_result(duel, ft, EXACT)
        probe = [i for i, pd in enumerate(duel.pods) if pd.role == "probe"][0]
        if capi.UNSCHEDULED in want[0] or want[0][probe] != duel.local("exact"):
            raise AssertionError(f"the exact reference does not decide a {kind} duel for `exact`: {want}")
        must = targets(kind)
        if all((duel_result(duel, ft, fit) != want) == (m in must) for m, (fit, _) in MODELS.items()):
            return duel
    raise RuntimeError(f"no {kind} duel found")


# ---- the domain of the mask rows, restated (simon_hip.hip: rest_supported, gfold_supported, choose_variant) ------------------------------------
def check_domain(prob, eph_g=1):
    """-> the list of what keeps the problem off the mask rows (empty: inside)"""
    bad = []
    N, P = prob.n_nodes, prob.n_pods
    if prob.alloc_eph is not None:
        g = staging_gcds(prob)[0]
        if g != eph_g:
            bad.append(f"ephemeral gcd {g}, meant {eph_g}")
        for arr, what in ((prob.alloc_eph, "alloc_eph"), (prob.req_eph, "req_eph")):
            if int(arr.max()) // g >= LIM31:
                bad.append(f"{what} quotient {int(arr.max()) // g}")
        if (prob.init_req_eph < 0).any() or (prob.init_req_eph > prob.alloc_eph).any():
            bad.append("init_req_eph beyond alloc_eph")
        if (prob.init_scalar_req > prob.scalar_alloc).any() or (prob.init_scalar_req < 0).any():
            bad.append("init_scalar_req beyond scalar_alloc")
        if int(prob.scalar_alloc.max()) >= LIM31 or int(prob.scalar_req.max()) >= LIM31:
            bad.append(f"extended resource {max(int(prob.scalar_alloc.max()), int(prob.scalar_req.max()))}")
        sigs = {(int(prob.req_eph[p]),) + tuple(int(v) for v in prob.scalar_req[:, p]) for p in range(P)} - {(0,) * 5}
        if len(sigs) > MAX_XRES_SIGS:
            bad.append(f"{len(sigs)} extra-resource requests")
        if prob.preset_node is not None and any(prob.preset_node[p] >= 0 and (prob.req_eph[p] or prob.scalar_req[:, p].any()) for p in range(P)):
            bad.append("a preset pod requests an extra resource")
    if prob.gpu_cnt is not None:
        per_dev = [int(prob.gpu_mem_total[j]) // int(prob.gpu_cnt[j]) for j in range(N) if prob.gpu_cnt[j] > 0]
        vals = per_dev + [int(v) for v in prob.init_gpu_used.reshape(-1)] + [int(v) for v in prob.gpu_mem if v > 0]
        g = functools.reduce(math.gcd, vals, 0) or 1
        if g != 1:
            bad.append(f"GPU gcd {g}")
        if min(vals) < 0 or max(vals) // g >= LIM31:
            bad.append(f"GPU quotient {max(vals) // g}")
        sigs = {(int(m) // g, min(int(n), 64)) for m, n in zip(prob.gpu_mem, prob.pod_gpu_cnt) if m > 0}
        if len(sigs) > MAX_GPU_SIGS:
            bad.append(f"{len(sigs)} GPU requests")
    if duel_util.route_bound(prob) >= LIM31 or max(int(prob.alloc_mem.max()), int(prob.init_req_mem.max())) + int(prob.req_mem.sum()) >= LIM31:
        bad.append("cpu / memory beyond the narrow route (choose_variant)")
    for arrs in ((prob.alloc_cpu, prob.init_req_cpu, prob.req_cpu), (prob.alloc_mem, prob.init_req_mem, prob.req_mem)):
        if functools.reduce(math.gcd, (int(np.gcd.reduce(a)) for a in arrs), 0) != 1:
            bad.append("cpu / memory gcd")
    return bad


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------------
XRES_LIST = ("eph_edge", "eph_wrap") + tuple(f"scalar_edge:{k}" for k in range(4)) + tuple(f"scalar_wrap:{k}" for k in range(4))
GPU_LIST = ("gpu_one_edge", "gpu_total_floor", "gpu_tightest", "gpu_multi:2", "gpu_multi:3", "gpu_multi:4", "gpu_overbooked")
MIXED_LIST = ("eph_edge", "gpu_one_edge", "scalar_wrap:1", "gpu_tightest", "eph_wrap", "gpu_multi:3", "scalar_edge:2", "gpu_overbooked", "gpu_total_floor",
              "scalar_edge:0", "gpu_multi:2", "scalar_wrap:3")
EDGE_LIST = {"eph": ("eph_edge", "eph_wrap"), "scalar": ("scalar_edge:1", "scalar_wrap:1"), "gpu": ("gpu_one_edge", "gpu_multi:2")}
# name -> (seed, kinds in turn, duels, flavour, features, ballast)
FIXTURES = {
    "xres_initial": (21, XRES_LIST, 20, "initial", Features(xres=True), None),
    "xres_refresh": (22, XRES_LIST, 20, "refresh", Features(xres=True), None),
    "ephgcd_initial": (23, GCD_KINDS, 12, "initial", Features(xres=True, eph_g=EPH_G), None),
    "ephgcd_refresh": (24, GCD_KINDS, 12, "refresh", Features(xres=True, eph_g=EPH_G), None),
    "gpu_initial": (25, GPU_LIST, 21, "initial", Features(gpu=True), None),
    "gpu_refresh": (26, GPU_LIST, 21, "refresh", Features(gpu=True), None),
    "mixed_refresh": (27, MIXED_LIST, 12, "refresh", Features(xres=True, gpu=True, anti=True), None),
    "xres_70classes": (28, XRES_LIST, 24, "refresh", Features(xres=True, distinct_caps=True), None),
    "gpu_70classes": (29, GPU_LIST, 24, "refresh", Features(gpu=True, distinct_caps=True), None),
    "xres_spread": (30, XRES_LIST, 20, "refresh", Features(xres=True, spread=True), None),
    "gpu_spread": (31, GPU_LIST, 21, "refresh", Features(gpu=True, spread=True), None),
}
for _res, _ft in (("eph", Features(xres=True)), ("scalar", Features(xres=True)), ("gpu", Features(gpu=True))):
    FIXTURES[f"edge_{_res}_inside"] = (32, EDGE_LIST[_res], 6, "refresh", _ft, (_res, LIM31 - 1))
    FIXTURES[f"edge_{_res}_outside"] = (32, EDGE_LIST[_res], 6, "refresh", _ft, (_res, LIM31))
TOP_KINDS = ("eph_edge", "eph_gcd:edge", "scalar_edge:0", "gpu_one_edge")      # their first duel's `exact` holds 2^31 - 1
DUEL_FIXTURES = [n for n in FIXTURES if not n.startswith("edge_")]


@dataclass
class Fixture:
    name: str
    prob: capi.Problem
    orders: np.ndarray          # four orders that permute whole duels
    scen: np.ndarray            # the full pool under each order, then two prefix scenarios that end behind a whole duel
    expected: np.ndarray        # [P] the exact reference's placements of the full pool (the same under every order: duels are disjoint)
    slices: np.ndarray          # [P] uint64 its gpu_slices
    duels: list
    pod0: list                  # first pod of every duel
    node0: list                 # first node of every duel
    ft: Features

    def duel_pods(self, d):
        return range(self.pod0[d], self.pod0[d] + len(self.duels[d].pods))


def build(name):
    seed, kinds, D, flavour, ft, ballast = FIXTURES[name]
    rng = np.random.default_rng(seed)
    pools = make_pools(rng)
    seen = set()
    duels = []
    for i in range(D):
        kind = kinds[i % len(kinds)]
        duels.append(gen_duel(rng, kind, flavour, pools, ft, top=kind in TOP_KINDS and kind not in seen))
        seen.add(kind)
    prob, pod0, node0 = assemble(duels, ft, seed, ballast)
    N, P = prob.n_nodes, prob.n_pods
    assert N <= 200 and P <= 200 and P <= 128                   # (a pod class and a signature per pod: generation 6 holds 128)
    bad = check_domain(prob, ft.eph_g)
    assert len(bad) == (1 if ballast is not None and ballast[1] >= LIM31 else 0), bad
    shapes = {(int(a), int(b)) for a, b in zip(prob.alloc_cpu, prob.alloc_mem)}
    assert len(shapes) == (N if ft.distinct_caps else min(8, D)), len(shapes)        # (the ballast node has shape 0)
    blocks = lambda perm: [p for d in perm for p in range(pod0[d], pod0[d] + len(duels[d].pods))]
    orders = np.array([blocks(range(D)), blocks(reversed(range(D))), blocks(rng.permutation(D)), blocks(rng.permutation(D))], np.int32)
    scen = np.array([[N, o] for o in range(4)] + [[node0[D // 3], 1], [node0[2 * D // 3], 2]], np.int32)
    place, unsched, _, _, slices = schedule(prob, orders[0], N)
    assert unsched == 0
    for d, duel in enumerate(duels):
        probe = pod0[d] + [i for i, pd in enumerate(duel.pods) if pd.role == "probe"][0]
        assert place[probe] == node0[d] + duel.local("exact")
    return Fixture(name, prob, orders, scen, np.array(place, np.int32), np.array(slices, np.uint64), duels, pod0, node0, ft)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """cached; no test modifies what it returns"""
    return build(name)

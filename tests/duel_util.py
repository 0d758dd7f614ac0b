"""Score duels on 31-bit coprime quantities (tests only): seeded problems in which ONE pod is admitted to a handful of nodes by
the static mask, two of them -- the probe and the judge -- hold exactly the same exact total, and the probe sits where the fp64
evaluation of an integer score is fragile.  The first of the two in canonical order wins the exact tie; a kernel whose
LeastAllocated / BalancedAllocation / class term is off by one unit in the last place there sends the pod to the other node.

Three parts:
  * the exact reference (Python integers, correctly rounded floats) and a small scheduler over a capi.Problem that takes the
    three terms as a parameter (Arith);
  * near-miss models: Arith objects that compute ONE term the way a subtly wrong kernel would.  An fma is
    float(Fraction(a) * Fraction(b) + Fraction(c)) (correctly rounded).  They choose the inputs and prove that the fixtures have
    teeth (tests/test_duels_host.py); the kernel's own forms (KERNEL_FORMS) are modelled too and must agree with the exact reference;
  * the generator: build(seed, kinds, n_duels, flavour) -> (capi.Problem, orders, expected_placement), and the named fixtures of
    tests/test_duels_host.py and tests/test_gpu_duels.py (fixture(name), cached, never modified by a test).

Duel kinds (each targets one function and one direction of error; `first` is the node the exact reference picks):
  la_int      (cap - r) 100 / cap is an exact integer: cap = 100 c, c odd in 2^22 .. 2^24         la_naive or la_nobias under-estimates
              (RN(1 / cap) is too small for the one, RN(100 RN(1 / cap)) too large for the other: sub-kinds la_int:naive, la_int:nobias)
  la_below    100 r = 1 (mod cap), cap in 2^29 .. 2^31 coprime to 10: fraction (cap - 1) / cap    la_bigbias over-estimates
  la_edge     r == cap (terms 0, BalancedAllocation 0 by its guard)                               guard_late (`>` for `>=`) over-estimates
              r == cap - 1 (term 0 with fraction 100 / cap, BalancedAllocation NOT guarded)       guard_early (`r + 1 >= cap`) under-estimates
  ba_equal    cap_m = mul cap_c, r_m = mul r_c, mul in {3, 5, 7}, cap_c in 2^27 .. 2^28: cf == mf  ba_uncorrected under-estimates
  ba_int      (1 - |cf - mf|) 100 within one ulp of an integer (found by a directed search)       ba_contracted, either direction
  simon_int / na_int / tt_int        100 x / m an exact integer, m up to 2^30 - 1                  term_naive under-estimates the quotient
  simon_below / na_below / tt_below  100 x = m - 1 (mod m)                                         term_bigbias over-estimates the quotient
  every class-term kind has x >= 2^25                                                             term_i32 wraps 100 x
(guard_late, guard_early and term_bigbias are this module's additions to the issue's list: la_edge and the *_below class-term
kinds need a model of their own direction.)

ba_contracted and ba_int: the directed search (_gen_ba_int: states whose cf - mf is a few units of 2^-60 away from j / 100) finds an
input on which RN(100 - 100 diff) and RN(100 RN(1 - diff)) truncate differently about once per 150 candidates, so both the
model and the kind are kept (tests/test_duels_host.py::test_ba_contracted_search prints the count).

The domain of every problem: cpu gcd 1, memory gcd 1, (largest node quantity + sum of max(req, nz) over all pods) < 2^31 -- what
choose_variant (simon_hip.hip) asks of the narrow route; build() asserts both.  Pod requests are 2^16 .. 2^19 units so that 300 pods
next to a 1.8e9-unit node stay inside; the fragile states come from the nodes' initial state."""
import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from open_simulator_amd import capi

LIM31 = 1 << 31
CAP_MAX = LIM31 - 320 * (1 << 20)        # room for 300 pods of < 2^20 units next to the largest node
Q_LO, Q_HI = 1 << 16, 1 << 19            # a duel pod's request
MIN_STATE = (1 << 20) + (1 << 11)        # every state of a probe / judge (after the duel pod): two requests and the nz offsets fit below it
RAW_MAX = (1 << 30) - 1                  # the host admits raw scores < 2^30


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _rcp(x):
    return 1.0 / x                       # int / float true division: correctly rounded


# ---- the three terms: exact reference --------------------------------------------------------------------------------------------
def la_exact(r, cap):
    return 0 if cap == 0 or r > cap else (cap - r) * 100 // cap


def ba_exact(r_c, cap_c, r_m, cap_m):
    cf = 1.0 if cap_c == 0 else r_c / cap_c
    mf = 1.0 if cap_m == 0 else r_m / cap_m
    return 0 if cf >= 1 or mf >= 1 else int((1 - abs(cf - mf)) * 100)


def term_exact(x, m):
    """floor(100 x / m) of the class terms (oracle/simon_oracle.c: Simon min-max, NodeAffinity, TaintToleration), m > 0"""
    return 100 * x // m


@dataclass(frozen=True)
class Arith:
    name: str
    la: callable = la_exact
    ba: callable = ba_exact
    term: callable = term_exact


EXACT = Arith("exact")


# ---- the kernels' own forms (must equal the exact reference on every fixture) -------------------------------------------------------
def _la_fma(r, cap, c):
    if cap == 0 or r >= cap:
        return 0
    rc100 = 100.0 * _rcp(cap)
    return int(fma(-r, rc100, c))


def la_kernel(r, cap):                   # la_term_f / la_term_t
    return _la_fma(r, cap, 100.0 + 2.0 ** -33)


def la_kernel_v1(r, cap):                # la_term of simon_device.h
    if cap == 0 or r > cap:
        return 0
    rc = _rcp(cap)
    return int(fma(float((cap - r) * 100), rc, 0.5 * rc))


def _ba_from(cf, mf):
    return 0 if cf >= 1 or mf >= 1 else int((1 - abs(cf - mf)) * 100)


def _div1(a, b):                         # div_by_rcp1
    rc = _rcp(b)
    q = float(a) * rc
    return fma(fma(-q, b, a), rc, q)


def _div2(a, b):                         # div_by_rcp
    rc = _rcp(b)
    q = _div1(a, b)
    return fma(fma(-q, b, a), rc, q)


def ba_kernel1(r_c, cap_c, r_m, cap_m):
    return _ba_from(_div1(r_c, cap_c), _div1(r_m, cap_m))


def ba_kernel2(r_c, cap_c, r_m, cap_m):
    return _ba_from(_div2(r_c, cap_c), _div2(r_m, cap_m))


def term_kernel(x, m):
    rr = _rcp(m)
    return int(fma(float(100 * x), rr, 0.5 * rr))


KERNEL_FORMS = [Arith("kernel_table", la=la_kernel, ba=ba_kernel1, term=term_kernel), Arith("kernel_v1", la=la_kernel_v1, ba=ba_kernel2, term=term_kernel)]


# ---- near-miss models -----------------------------------------------------------------------------------------------------------------
def la_naive(r, cap):
    if cap == 0 or r > cap:
        return 0
    return int(float((cap - r) * 100) * _rcp(cap))


def la_nobias(r, cap):
    return _la_fma(r, cap, 100.0)


def la_bigbias(r, cap):
    return _la_fma(r, cap, 100.0 + 2.0 ** -24)


def ba_uncorrected(r_c, cap_c, r_m, cap_m):
    return _ba_from(float(r_c) * _rcp(cap_c), float(r_m) * _rcp(cap_m))


def ba_contracted(r_c, cap_c, r_m, cap_m):
    cf, mf = r_c / cap_c, r_m / cap_m
    return 0 if cf >= 1 or mf >= 1 else int(fma(-100.0, abs(cf - mf), 100.0))


def ba_guard_late(r_c, cap_c, r_m, cap_m):
    cf, mf = r_c / cap_c, r_m / cap_m
    return 0 if cf > 1 or mf > 1 else int((1 - abs(cf - mf)) * 100)


def la_guard_early(r, cap):
    return 0 if r + 1 >= cap else la_exact(r, cap)


def ba_guard_early(r_c, cap_c, r_m, cap_m):
    return 0 if r_c + 1 >= cap_c or r_m + 1 >= cap_m else ba_exact(r_c, cap_c, r_m, cap_m)


def term_naive(x, m):
    return int(float(100 * x) * _rcp(m))


def term_bigbias(x, m):
    rr = _rcp(m)
    return int(fma(float(100 * x), rr, 0.5 * rr + 2.0 ** -24))


def term_i32(x, m):
    y = (100 * x + (1 << 31)) % (1 << 32) - (1 << 31)
    rr = _rcp(m)
    return int(fma(float(y), rr, 0.5 * rr))


LA_KINDS = ("la_int", "la_below", "la_edge", "ba_equal", "ba_int")
CLASS_KINDS = ("simon_int", "simon_below", "na_int", "na_below", "tt_int", "tt_below")
# model -> the kinds whose every duel it sends to the wrong node
MODELS = {
    "la_naive": (Arith("la_naive", la=la_naive), ("la_int:naive",)),
    "la_nobias": (Arith("la_nobias", la=la_nobias), ("la_int:nobias",)),
    "la_bigbias": (Arith("la_bigbias", la=la_bigbias), ("la_below",)),
    "guard_late": (Arith("guard_late", ba=ba_guard_late), ("la_edge:full",)),
    "guard_early": (Arith("guard_early", la=la_guard_early, ba=ba_guard_early), ("la_edge:last",)),
    "ba_uncorrected": (Arith("ba_uncorrected", ba=ba_uncorrected), ("ba_equal",)),
    "ba_contracted": (Arith("ba_contracted", ba=ba_contracted), ("ba_int",)),
    "term_naive": (Arith("term_naive", term=term_naive), ("simon_int", "na_int", "tt_int")),
    "term_bigbias": (Arith("term_bigbias", term=term_bigbias), ("simon_below", "na_below", "tt_below")),
    "term_i32": (Arith("term_i32", term=term_i32), CLASS_KINDS),
}
_LABA_MODELS = [MODELS[k][0] for k in ("la_naive", "la_nobias", "la_bigbias", "guard_late", "guard_early", "ba_uncorrected", "ba_contracted")] + KERNEL_FORMS


def laba(ar, r_c, cap_c, r_m, cap_m):
    return (ar.la(r_c, cap_c) + ar.la(r_m, cap_m)) // 2 + ar.ba(r_c, cap_c, r_m, cap_m)


# ---- the reference scheduler ------------------------------------------------------------------------------------------------------------
def admitted_nodes(prob):
    """per pod class the nodes its static-mask row admits, ascending"""
    N = prob.n_nodes
    out = []
    for c in range(prob.n_pod_classes):
        out.append([j for j in range(N) if prob.static_mask is None or (int(prob.static_mask[c, j // 64]) >> (j % 64)) & 1])
    return out


def schedule(prob, order, n_nodes, ar=EXACT):
    """One scenario of a cpu + memory problem with static masks, presets, gates and the three class tables, one pod at a time
    (oracle/simon_oracle.c: run_scenario, schedule_one), the score terms from `ar`.  Returns (placement [P], unscheduled, used_cpu,
    used_mem) in Python integers."""
    N, P = prob.n_nodes, prob.n_pods
    I = lambda a, n: [int(v) for v in a] if a is not None else [0] * n
    a_c, a_m, a_p = I(prob.alloc_cpu, N), I(prob.alloc_mem, N), I(prob.alloc_pods, N)
    rq_c, rq_m = I(prob.init_req_cpu, N), I(prob.init_req_mem, N)
    nz_c = I(prob.init_nz_cpu, N) if prob.init_nz_cpu is not None else list(rq_c)
    nz_m = I(prob.init_nz_mem, N) if prob.init_nz_mem is not None else list(rq_m)
    npods = I(prob.init_npods, N)
    ncls = I(prob.node_class, N)
    p_rc, p_rm = I(prob.req_cpu, P), I(prob.req_mem, P)
    p_nc = I(prob.nz_cpu, P) if prob.nz_cpu is not None else p_rc
    p_nm = I(prob.nz_mem, P) if prob.nz_mem is not None else p_rm
    pcls = I(prob.pod_class, P)
    preset = I(prob.preset_node, P) if prob.preset_node is not None else [-1] * P
    gate = I(prob.gate_node, P) if prob.gate_node is not None else [-1] * P
    adm = admitted_nodes(prob)
    raw, na, tt = prob.simon_raw, prob.node_affinity_raw, prob.taint_prefer_raw
    place = [capi.UNSCHEDULED] * P
    unsched = 0

    def add(p, j):
        rq_c[j] += p_rc[p]; rq_m[j] += p_rm[p]; nz_c[j] += p_nc[p]; nz_m[j] += p_nm[p]; npods[j] += 1

    for p in (int(x) for x in order):
        if gate[p] >= n_nodes:
            place[p] = capi.GATED
            continue
        if preset[p] >= 0:
            add(p, preset[p]); place[p] = preset[p]
            continue
        c = pcls[p]
        zero = p_rc[p] == 0 and p_rm[p] == 0
        feas = [j for j in adm[c] if j < n_nodes and npods[j] + 1 <= a_p[j] and (zero or (a_c[j] >= rq_c[j] + p_rc[p] and a_m[j] >= rq_m[j] + p_rm[p]))]
        if not feas:
            unsched += 1
            continue
        if len(feas) > 1:
            raws = [int(raw[c, ncls[j]]) for j in feas]
            lo, hi = min(raws), max(raws)
            na_max = max([0] + [int(na[c, ncls[j]]) for j in feas]) if na is not None else 0
            tt_max = max([0] + [int(tt[c, ncls[j]]) for j in feas]) if tt is not None else 0
            best, best_total = -1, 0
            for j, rw in zip(feas, raws):
                total = laba(ar, nz_c[j] + p_nc[p], a_c[j], nz_m[j] + p_nm[p], a_m[j])
                total += 2 * ar.term(rw - lo, hi - lo) if hi > lo else 0
                if na is not None:
                    total += ar.term(int(na[c, ncls[j]]), na_max) if na_max else 0
                if tt is not None:
                    total += 100 - ar.term(int(tt[c, ncls[j]]), tt_max) if tt_max else 100
                if best < 0 or total > best_total:
                    best, best_total = j, total
        else:
            best = feas[0]
        add(p, best); place[p] = best
    return place, unsched, sum(rq_c[:n_nodes]), sum(rq_m[:n_nodes])


# ---- the generator -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Node:
    cap_c: int
    cap_m: int
    r_c: int        # NonZeroRequested + the duel pod's non-zero request: the state the duel pod is scored on
    r_m: int
    raw: int = 0    # the duel's class-table value of this node (class-term kinds)


@dataclass
class Duel:
    kind: str               # with the sub-kind where there is one: "la_edge:full" / "la_edge:last", "la_int:naive" / "la_int:nobias"
    nodes: list             # canonical order; nodes[first] wins the exact tie against nodes[first + 1]
    first: int
    q_c: int = 0
    q_m: int = 0
    lo: int = 0             # simon kinds: the low anchor's raw score

    @property
    def base_kind(self):
        return self.kind.split(":")[0]


def _odd(rng, lo, hi):
    return int(rng.integers(lo, hi)) | 1


def _swap(res, t, o):
    """(target, other) -> (cpu, memory)"""
    return (t, o) if res == 0 else (o, t)


def _find_judge(rng, cap_c, cap_m, total, zone="any", tries=3):
    """A state on (cap_c, cap_m) whose exact LeastAllocated + BalancedAllocation is `total` and on which every near-miss model and
    kernel form agrees with the exact reference.  zone "full_c" / "full_m": that resource exactly full, the other below 1 %."""
    for _ in range(tries):
        n = 40000
        if zone == "any":
            cf = rng.uniform(0.003, 0.997, n)
            mf = np.where(rng.random(n) < 0.5, rng.uniform(0.003, 0.997, n), np.clip(cf + rng.uniform(-0.03, 0.03, n), 0.003, 0.997))
            r_c, r_m = (cf * cap_c).astype(np.int64), (mf * cap_m).astype(np.int64)
        else:
            small = rng.uniform(0.004, 0.0099, n)
            r_c = np.full(n, cap_c, np.int64) if zone == "full_c" else (small * cap_c).astype(np.int64)
            r_m = np.full(n, cap_m, np.int64) if zone == "full_m" else (small * cap_m).astype(np.int64)
        la = ((cap_c - r_c) * 100 // cap_c + (cap_m - r_m) * 100 // cap_m) // 2
        cfv, mfv = r_c / float(cap_c), r_m / float(cap_m)
        ba = np.where((cfv >= 1) | (mfv >= 1), 0, np.trunc((1.0 - np.abs(cfv - mfv)) * 100.0)).astype(np.int64)
        for i in np.nonzero(la + ba == total)[0][:60]:
            rc, rm = int(r_c[i]), int(r_m[i])
            if min(rc, rm) < MIN_STATE or laba(EXACT, rc, cap_c, rm, cap_m) != total:
                continue
            if all(laba(m, rc, cap_c, rm, cap_m) == total for m in _LABA_MODELS):
                return rc, rm
    return None


def _gen_caps(kind, rng, res):
    if kind == "la_int":
        t, o = 100 * _odd(rng, 1 << 22, 1 << 24), _odd(rng, 1 << 28, 1 << 30)
    elif kind == "la_below":
        while True:
            t = _odd(rng, 1 << 29, CAP_MAX)
            if t % 5:
                break
        o = _odd(rng, 1 << 28, 1 << 30)
    elif kind == "la_edge":
        t, o = _odd(rng, 1 << 29, CAP_MAX), _odd(rng, 1 << 28, 1 << 30)
    elif kind == "ba_equal":
        c = _odd(rng, 1 << 27, 1 << 28)
        return c, int(rng.choice([3, 5, 7])) * c
    else:   # ba_int: coprime capacities
        while True:
            t, o = _odd(rng, 1 << 28, 1 << 30), _odd(rng, 1 << 28, 1 << 30)
            if math.gcd(t, o) == 1:
                break
    return _swap(res, t, o)


BA_INT_TRIED = [0, 0]        # candidates of the directed ba_int search, and how many of them ba_contracted truncates differently


def _gen_ba_int(rng, cap_c, cap_m):
    """cf - mf = t / (cap_c cap_m) for an integer t next to j cap_c cap_m / 100: r_c = t cap_m^-1 (mod cap_c), r_m = (r_c cap_m - t) / cap_c"""
    inv = pow(cap_m, -1, cap_c)
    for _ in range(40):
        j = int(rng.integers(8, 60))
        t0 = j * cap_c * cap_m // 100
        for t in range(t0 - 60, t0 + 61):
            r_c = t * inv % cap_c
            r_m, rem = divmod(r_c * cap_m - t, cap_c)
            if rem or not (MIN_STATE <= r_m < cap_m - 1 and MIN_STATE <= r_c < cap_c - 1):
                continue
            BA_INT_TRIED[0] += 1
            if ba_contracted(r_c, cap_c, r_m, cap_m) != ba_exact(r_c, cap_c, r_m, cap_m):
                BA_INT_TRIED[1] += 1
                return r_c, r_m
    return None


def _gen_probe(kind, rng, res, cap_c, cap_m, alt):
    """-> (sub-kind, r_c, r_m, judge zone) or None when this draw does not work out"""
    ct, co = _swap(res, cap_c, cap_m)           # (the inverse of _swap is _swap)
    sub, zone = kind, "any"
    if kind == "la_int":
        c = ct // 100
        sub = "la_int:naive" if alt else "la_int:nobias"     # (the two models err on different capacities)
        rt = ct - int(rng.integers(5, 96)) * c
        ro = int(rng.uniform(0.05, 0.95) * co)
    elif kind == "la_below":
        rt = pow(100, -1, ct)
        ro = int(rng.uniform(0.05, 0.95) * co)
        if not 3 <= la_exact(rt, ct) <= 97:
            return None
    elif kind == "la_edge":
        if alt:
            sub, rt, ro, zone = "la_edge:full", ct, int(rng.uniform(0.0105, 0.0195) * co), "full_m" if res == 0 else "full_c"
        else:
            sub, rt, ro = "la_edge:last", ct - 1, int(rng.uniform(0.2, 0.8) * co)
    elif kind == "ba_equal":
        mul = cap_m // cap_c
        r = int(rng.uniform(0.05, 0.95) * cap_c)
        return sub, r, mul * r, zone
    else:
        got = _gen_ba_int(rng, cap_c, cap_m)
        return None if got is None else (sub, got[0], got[1], zone)
    r_c, r_m = _swap(res, rt, ro)
    return sub, r_c, r_m, zone


def _targets(sub):
    return [m for m, (_, kinds) in MODELS.items() if sub in kinds or sub.split(":")[0] in kinds]


def gen_laba_duel(kind, rng, res, caps=None, alt=0):
    """One duel of a LeastAllocated / BalancedAllocation kind on two nodes of one shape; caps: reuse this shape; alt: which sub-kind"""
    for _ in range(2000):
        cap_c, cap_m = caps or _gen_caps(kind, rng, res)
        got = _gen_probe(kind, rng, res, cap_c, cap_m, alt)
        if got is None:
            continue
        sub, r_c, r_m, zone = got
        if min(r_c, r_m) < MIN_STATE:
            continue
        total = laba(EXACT, r_c, cap_c, r_m, cap_m)
        if any(laba(k, r_c, cap_c, r_m, cap_m) != total for k in KERNEL_FORMS):
            raise AssertionError(f"the kernel's own form differs from the exact reference at {(sub, r_c, cap_c, r_m, cap_m)}")
        deltas = {laba(MODELS[m][0], r_c, cap_c, r_m, cap_m) - total for m in _targets(sub)}
        if 0 in deltas or (min(deltas) < 0 < max(deltas)):
            continue                            # teeth: every targeted model is off, all in one direction
        judge = _find_judge(rng, cap_c, cap_m, total, zone)
        if judge is None or judge == (r_c, r_m):
            continue
        probe, jn = Node(cap_c, cap_m, r_c, r_m), Node(cap_c, cap_m, judge[0], judge[1])
        under = max(deltas) < 0                 # the probe is under-estimated: it comes first, the model hands the pod to the judge
        return Duel(sub, [probe, jn] if under else [jn, probe], 0, int(rng.integers(Q_LO, Q_HI)), int(rng.integers(Q_LO, Q_HI)))
    raise RuntimeError(f"no {kind} duel found")


def _robust_state(rng, cap_c, cap_m, lo_f, hi_f):
    for _ in range(200):
        r_c, r_m = int(rng.uniform(lo_f, hi_f) * cap_c), int(rng.uniform(lo_f, hi_f) * cap_m)
        t = laba(EXACT, r_c, cap_c, r_m, cap_m)
        if all(laba(m, r_c, cap_c, r_m, cap_m) == t for m in _LABA_MODELS):
            return r_c, r_m, t
    raise RuntimeError("no robust state")


def gen_class_duel(kind, rng):
    """One duel of a class-term kind on four nodes in the four node classes 0 .. 3: low anchor, high anchor (both exactly full on cpu:
    LeastAllocated + BalancedAllocation 0, so they lose), then the tied pair.  The judge's quotient differs from the probe's by D
    and its LeastAllocated + BalancedAllocation makes up for it, so that a model that garbles every quotient (term_i32) also errs."""
    table, which = kind.split("_")
    w = 2 if table == "simon" else 1
    sign = -1 if table == "tt" else 1                           # TaintToleration scores 100 - quotient
    for _ in range(400):
        if which == "int":
            m = 100 * int(rng.integers((1 << 29) // 100 + 1, RAW_MAX // 100))
            k = int(rng.integers(40, 96))
            x = k * (m // 100)
        else:
            m = _odd(rng, 1 << 29, RAW_MAX)
            if m % 5 == 0:
                continue
            x = -pow(100, -1, m) % m
            k = term_exact(x, m)
            if not 40 <= k <= 95:
                continue
        model = MODELS["term_naive" if which == "int" else "term_bigbias"][0]
        dq = model.term(x, m) - k
        if dq == 0 or term_kernel(x, m) != k:
            if term_kernel(x, m) != k:
                raise AssertionError(f"the kernel's class term differs from the exact reference at {(x, m)}")
            continue
        under = dq * sign < 0                                    # the probe's SCORE is under-estimated: the probe comes first
        d = int(rng.integers(2, 7))
        kj = k - d * sign if under else k + d * sign             # the judge's class score is D = w d lower (probe first) / higher (judge first)
        if not 30 <= kj <= 98:
            continue
        xj = (2 * kj + 1) * m // 200                             # fraction one half: no model of the quotient but term_i32 moves it
        if any(a.term(xj, m) != kj for a in (MODELS["term_naive"][0], MODELS["term_bigbias"][0], KERNEL_FORMS[0])) or xj < 1 << 25 or x < 1 << 25:
            continue
        caps = [(_odd(rng, 1 << 28, 1 << 30), _odd(rng, 1 << 28, 1 << 30)) for _ in range(4)]
        pc, pm, pt = _robust_state(rng, caps[2][0], caps[2][1], 0.1, 0.4)
        judge = _find_judge(rng, caps[3][0], caps[3][1], pt + (w * d if under else -w * d))
        if judge is None:
            continue
        lo = int(rng.integers(0, RAW_MAX - m)) if table == "simon" else 0
        probe, jn = Node(caps[2][0], caps[2][1], pc, pm, lo + x), Node(caps[3][0], caps[3][1], judge[0], judge[1], lo + xj)
        full = lambda cc, cm, raw: Node(cc, cm, cc, int(rng.uniform(0.985, 0.995) * cm), raw)
        duel = Duel(kind, [full(*caps[0], lo), full(*caps[1], lo + m)] + ([probe, jn] if under else [jn, probe]), 2,
                    int(rng.integers(Q_LO, Q_HI)), int(rng.integers(Q_LO, Q_HI)), lo)
        if duel_pick(duel, EXACT) != 2 or any(duel_pick(duel, MODELS[mm][0]) == 2 for mm in _targets(kind)):
            continue
        return duel
    raise RuntimeError(f"no {kind} duel found")


def duel_pick(duel, ar):
    """index (within the duel) of the node the duel pod goes to under `ar`: first maximum in canonical order"""
    table = duel.base_kind.split("_")[0]
    raws = [n.raw for n in duel.nodes]
    lo, hi = min(raws), max(raws)
    best, best_total = -1, 0
    for i, n in enumerate(duel.nodes):
        total = laba(ar, n.r_c, n.cap_c, n.r_m, n.cap_m)
        if table == "simon":
            total += 2 * ar.term(n.raw - lo, hi - lo)
        elif table == "na":
            total += ar.term(n.raw, hi)
        elif table == "tt":
            total += 100 - ar.term(n.raw, hi)
        if best < 0 or total > best_total:
            best, best_total = i, total
    return best


FLAVOURS = ("initial", "refresh", "nz")


def gen_duels(seed, kinds, n_duels, shapes=None):
    """n_duels duels, the kinds in turn; shapes = n_duels / 2: consecutive duels of a LeastAllocated / BalancedAllocation kind share
    one capacity shape (two signatures on one internal node class)"""
    rng = np.random.default_rng(seed)
    duels = []
    for i in range(n_duels):
        g = i // 2 if shapes else i
        kind = kinds[g % len(kinds)]
        if kind in CLASS_KINDS:
            duels.append(gen_class_duel(kind, rng))
            continue
        caps = None
        if shapes and i % 2:
            caps = (duels[-1].nodes[0].cap_c, duels[-1].nodes[0].cap_m)
        duels.append(gen_laba_duel(kind, rng, g % 2, caps, (g // len(kinds)) % 2))
    return duels


def build(seed, kinds, n_duels, flavour="initial", shapes=None, ballast=None):
    """-> (capi.Problem, orders [4][P], expected_placement [P]: the same under every order, duels being disjoint).
    flavour "initial": the fragile state is the node's init_* state plus the duel pod; "refresh": it is reached only after a preset pod
    of the duel pod's class and request has landed on each node of the pair (the orders keep those ahead of the duel pod); "nz": as
    "initial" with nz_* != req_* and init_nz_* != init_req_*.  Every pod is gated on its duel's last node, so a prefix scenario that
    cuts the pool between two duels holds whole duels only.
    shapes = n_duels / 2: two duels per capacity shape.  ballast = e: one more node nobody is admitted to, sized so that (largest node +
    all pods) on cpu is 2^31 - 1 + e units."""
    return _build(seed, kinds, n_duels, flavour, shapes, ballast)[:3]


def _build(seed, kinds, n_duels, flavour, shapes, ballast):
    """build()'s triple and the duels themselves"""
    assert flavour in FLAVOURS
    duels = gen_duels(seed, kinds, n_duels, shapes)
    rng = np.random.default_rng(seed + 1000003)
    per = 3 if flavour == "refresh" else 1
    nodes = [n for d in duels for n in d.nodes]
    N, P, D = len(nodes) + (ballast is not None), per * len(duels), len(duels)
    class_kind = duels[0].base_kind in CLASS_KINDS
    Cn = 4 if class_kind else 1
    a_c, a_m = [n.cap_c for n in nodes], [n.cap_m for n in nodes]
    i_nc, i_nm, i_rc, i_rm, ncls = [], [], [], [], []
    req_c, req_m, nz_c, nz_m, pcls, preset, gate = [], [], [], [], [], [], []
    mask = np.zeros((D, (N + 63) // 64), np.uint64)
    reason = np.full((D, N), capi.REASON_NODE_AFFINITY, np.uint8)
    tables = {t: np.zeros((D, Cn), np.int64) for t in ("simon", "na", "tt")}
    expected = []
    j0 = 0
    for d, duel in enumerate(duels):
        sub_c, sub_m = (int(rng.integers(1, 1 << 10)), int(rng.integers(1, 1 << 10))) if flavour == "nz" else (0, 0)
        pair = (duel.first, duel.first + 1)
        for i, n in enumerate(duel.nodes):
            k = 2 if (flavour == "refresh" and i in pair) else 1           # requests of the duel's class that make up the state
            i_nc.append(n.r_c - k * duel.q_c); i_nm.append(n.r_m - k * duel.q_m)
            e_c, e_m = (int(rng.integers(1, 1 << 10)), int(rng.integers(1, 1 << 10))) if flavour == "nz" else (0, 0)
            i_rc.append(i_nc[-1] - e_c); i_rm.append(i_nm[-1] - e_m)
            assert i_rc[-1] >= 0 and i_rm[-1] >= 0
            ncls.append(i if class_kind else 0)
            mask[d, (j0 + i) // 64] |= np.uint64(1) << np.uint64((j0 + i) % 64)
            reason[d, j0 + i] = 0
            if class_kind:
                tables[duel.base_kind.split("_")[0]][d, i] = n.raw
        for k in range(per):
            req_c.append(duel.q_c - sub_c); req_m.append(duel.q_m - sub_m); nz_c.append(duel.q_c); nz_m.append(duel.q_m)
            pcls.append(d)
            preset.append(j0 + pair[k] if k < per - 1 else -1)
            gate.append(j0 + len(duel.nodes) - 1)
            expected.append(j0 + pair[k] if k < per - 1 else j0 + duel.first)
        j0 += len(duel.nodes)
    if ballast is not None:
        a_c.append(LIM31 - 1 + ballast - sum(nz_c)); a_m.append(_odd(rng, 1 << 28, 1 << 29))
        for v in (i_nc, i_nm, i_rc, i_rm, ncls):
            v.append(0)
        assert a_c[-1] > max(a_c[:-1])
    prob = capi.Problem(alloc_cpu=np.array(a_c, np.int64), alloc_mem=np.array(a_m, np.int64), alloc_pods=np.full(N, 110, np.int32),
                        node_class=np.array(ncls, np.int32), init_req_cpu=np.array(i_rc, np.int64), init_req_mem=np.array(i_rm, np.int64),
                        init_nz_cpu=np.array(i_nc, np.int64), init_nz_mem=np.array(i_nm, np.int64),
                        req_cpu=np.array(req_c, np.int64), req_mem=np.array(req_m, np.int64), nz_cpu=np.array(nz_c, np.int64), nz_mem=np.array(nz_m, np.int64),
                        pod_class=np.array(pcls, np.int32), gate_node=np.array(gate, np.int32),
                        n_pod_classes=D, n_node_classes=Cn, static_mask=mask, static_reason=reason,
                        simon_raw=tables["simon"] if class_kind and duels[0].base_kind.startswith("simon") else np.full((D, Cn), 57, np.int64))
    if flavour == "refresh":
        prob.preset_node = np.array(preset, np.int32)
    if duels[0].base_kind.startswith("na"):
        prob.node_affinity_raw = tables["na"]
    if duels[0].base_kind.startswith("tt"):
        prob.taint_prefer_raw = tables["tt"]
    prob.normalise()
    # no repeats: signatures and internal node classes do not collapse
    assert len({(d.q_c, d.q_m) for d in duels}) == D
    shapes_seen = {(n.cap_c, n.cap_m) for n in nodes}
    assert len(shapes_seen) == (shapes or (len(nodes) if class_kind else D)), (len(shapes_seen), shapes)
    # the domain of the narrow route (simon_hip.hip: choose_variant)
    for alloc, irq, inz, prq, pnz in ((prob.alloc_cpu, prob.init_req_cpu, prob.init_nz_cpu, prob.req_cpu, prob.nz_cpu),
                                      (prob.alloc_mem, prob.init_req_mem, prob.init_nz_mem, prob.req_mem, prob.nz_mem)):
        g = 0
        for arr in (alloc, irq, inz, prq, pnz):
            g = math.gcd(g, int(np.gcd.reduce(arr)))
        assert g == 1, g
        top = max(int(alloc.max()), int(irq.max()), int(inz.max())) + int(np.maximum(prq, pnz).sum())
        assert top < LIM31 or (ballast and alloc is prob.alloc_cpu and top == LIM31), top
    return prob, _orders(rng, D, per), np.array(expected, np.int32), duels


def route_bound(prob):
    """(largest node quantity + sum of max(req, nz) over all pods) of cpu, in units (gcd 1): what choose_variant compares with 2^31"""
    return max(int(prob.alloc_cpu.max()), int(prob.init_req_cpu.max()), int(prob.init_nz_cpu.max())) + int(np.maximum(prob.req_cpu, prob.nz_cpu).sum())


def _orders(rng, D, per):
    """four permutations of the pods; a duel's preset pods (per == 3: pods 3 d, 3 d + 1) stay ahead of its duel pod (3 d + 2)"""
    pods = lambda d: list(range(per * d, per * d + per))
    o0 = [p for d in range(D) for p in pods(d)]
    o1 = [p for d in reversed(range(D)) for p in pods(d)]
    o2 = [p for d in rng.permutation(D) for p in pods(int(d))[:-1]] + [per * int(d) + per - 1 for d in rng.permutation(D)]
    keys = rng.random((D, per))
    keys.sort(axis=1)
    o3 = [int(p) for p in np.argsort(keys.reshape(-1), kind="stable")]
    return np.array([o0, o1, o2, o3], np.int32)


@dataclass
class Fixture:
    name: str
    prob: capi.Problem
    orders: np.ndarray
    expected: np.ndarray
    scen: np.ndarray            # the full pool under each order, then two prefix scenarios that end behind a whole duel
    duels: list
    kinds: tuple


# name -> (seed, kinds, duels, flavour, extra arguments of build)
FIXTURES = {
    "laba60_initial": (11, LA_KINDS, 60, "initial", {}),
    "laba60_refresh": (12, LA_KINDS, 60, "refresh", {}),
    "laba60_nz": (13, LA_KINDS, 60, "nz", {}),
    "laba100_two_per_shape": (14, LA_KINDS, 100, "initial", {"shapes": 50}),
    "simon16": (15, ("simon_int", "simon_below"), 16, "initial", {}),
    "na16": (16, ("na_int", "na_below"), 16, "initial", {}),
    "tt16": (17, ("tt_int", "tt_below"), 16, "initial", {}),
    "edge_inside": (18, ("la_int", "la_below"), 16, "initial", {"ballast": 0}),
    "edge_outside": (18, ("la_int", "la_below"), 16, "initial", {"ballast": 1}),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    seed, kinds, n, flavour, extra = FIXTURES[name]
    prob, orders, expected, duels = _build(seed, kinds, n, flavour, extra.get("shapes"), extra.get("ballast"))
    per_duel = len(duels[0].nodes)
    N = prob.n_nodes
    scen = [[N, o] for o in range(len(orders))] + [[per_duel * (n // 3), 1], [per_duel * (2 * n // 3), 2]]
    return Fixture(name, prob, orders, expected, np.array(scen, np.int32), duels, tuple(kinds))

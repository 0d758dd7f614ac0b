"""Score duels for the two float normalisations that tests/duel_util.py leaves out (tests only): InterPodAffinity's
    int64(100.0 * (float64(raw - min) / float64(max - min)))        min and max taken from 0, weight 1
and PodTopologySpread's
    100 * (max + min - raw) / max  in int64                          weight 2
(oracle/simon_oracle.c: schedule_one).  A duel is one pod class that its static-mask row admits to its own handful of nodes: anchor
nodes fix the extremes, and two more nodes -- the probe and the judge -- hold exactly the same total.  The probe's normalised term sits
on a pair (x, d) where a plausible slip of the arithmetic is off by one; the judge's LeastAllocated + BalancedAllocation (duel_util:
_find_judge) makes up the difference of the terms.  The node a slip would wrongly prefer comes second in canonical order, so the exact
scheduler takes the first of the pair and the slip the other.

Raw scores come from COUNTERS, never from tables: every duel owns its terms, and counter pods that match (or own) them are put on the
duel's nodes ahead of the duel pod -- as pods bound by preset_node ("preset") or as ordinary pods whose class admits exactly one node
("placed": the kernel then updates its own counter rows before the duel pod is scored).  Topology keys: key 0 is hostname-like (domain =
node), keys 1 and 2 are zone-like with a node's position inside its duel as the domain (a permutation of it for key 2), so at most 8
domains per key and no duel sees another's counts -- the counters are per term.

The fragile pairs come from a vectorised scan of d, m <= 400 in correctly rounded binary64 (pair_tables); the raw spread score
trunc(sum cnt * log(size + 2) + maxSkew - 1) is NOT a duel target: a multiple of a logarithm is never within an ulp of an integer at
these sizes (the generator asserts a distance of 1e-6), so its float sum is only the way to the integers the normalisation sees.

Duel kinds (the model that loses them, the direction in which it errs):
  ipa_over      100 x / d is an integer that 100.0 * (x / d) misses from below: (29, 50), (58, 100)     ipa_int, ipa_mul_first over
  ipa_unc_up    ... and x * RN(1 / d) lands on it: (57, 100), (87, 150)                                  ipa_uncorrected (and the two above) over
  ipa_unc_down  x * RN(1 / d) falls below an integer the division reaches: (49, 98), (49, 49)           ipa_uncorrected under
  ipa_round     the fraction of 100 x / d is at least one half                                          ipa_round over
  ipa_min       every raw score above 0 (the minimum must still be 0)                                    ipa_min_not_zero, either
  ipa_max       every raw score below 0 (the maximum must still be 0)                                    ipa_max_not_zero, either
  pts_naive     (100 y) * RN(1 / m) falls below the integer 100 y / m: (49, 49), (49, 98)                pts_naive under
  pts_float     100.0 * (y / m) falls below it: (29, 50), (57, 100)                                      pts_float under
  pts_round     the fraction of 100 y / m is at least one half                                          pts_round over
The kernels' own forms (KERNEL_FORMS: div_by_rcp's two corrections, the fma with the half bias, divq_r's integer correction) are
modelled too and must equal the exact reference on every node of every duel; the generator asserts it."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import duel_util as U
from duel_util import fma
from open_simulator_amd import capi
from open_simulator_amd.gomath import spread_log_table

PAIR_MAX = 400
MAX_POS = 8                              # nodes of one duel: the domains of the zone-like keys
W_IPA, W_PTS = 1, 2                      # plugin weights
CQ_LO, CQ_HI = 1 << 8, 1 << 12           # a counter pod's request: 60 of them and the duel pod stay below duel_util.MIN_STATE
SPREAD_TAB_MAX, SPREAD_TAB_MAX2 = 512, 2048      # simon_table.h: SIMON_SPREAD_TAB_MAX, SIMON_SPREAD_TAB_MAX2
TABLE_MAX_CLASSES = 64                           # simon_table.h: kTableMaxClasses (beyond it the CN2 instantiations)


# ---- exact references --------------------------------------------------------------------------------------------------------------
def ipa_exact(x, lo, hi):
    return 0 if hi == lo else int(100.0 * ((x - lo) / (hi - lo)))


def pts_exact(raw, lo, hi):
    return 100 if hi == 0 else 100 * (hi + lo - raw) // hi


# ---- the kernels' own forms ----------------------------------------------------------------------------------------------------------
def ipa_rcp2(x, lo, hi):
    """simon_wide.hip stage B: 100.0 * div_by_rcp(x - min, diff, 1.0 / diff)"""
    return 0 if hi == lo else int(100.0 * U._div2(x - lo, hi - lo))


def pts_fma_half(raw, lo, hi):
    """simon_table.hip spread_select: (int)fma(100 (pmax + pmin - raw), 1 / pmax, 0.5 / pmax)"""
    if hi == 0:
        return 100
    r = 1.0 / hi
    return int(fma(float(100 * (hi + lo - raw)), r, 0.5 * r))


def pts_divq_r(raw, lo, hi):
    """simon_wide.hip divq_r: the product with the stored reciprocal plus the integer correction"""
    if hi == 0:
        return 100
    num = 100 * (hi + lo - raw)
    q = int(float(num) * (1.0 / hi))
    r = num - q * hi
    return q + (1 if r >= hi else 0) - (1 if r < 0 else 0)


# ---- near-miss models (scalar forms) ----------------------------------------------------------------------------------------------------
def ipa_int(x, lo, hi):
    return 0 if hi == lo else 100 * (x - lo) // (hi - lo)


def ipa_uncorrected(x, lo, hi):
    return 0 if hi == lo else int(100.0 * (float(x - lo) * (1.0 / (hi - lo))))


def ipa_mul_first(x, lo, hi):
    return 0 if hi == lo else int((100.0 * float(x - lo)) / (hi - lo))


def ipa_round(x, lo, hi):
    return 0 if hi == lo else int(math.floor(100.0 * ((x - lo) / (hi - lo)) + 0.5))


def pts_naive(raw, lo, hi):
    return 100 if hi == 0 else int(float(100 * (hi + lo - raw)) * (1.0 / hi))


def pts_float(raw, lo, hi):
    return 100 if hi == 0 else int(100.0 * ((hi + lo - raw) / hi))


def pts_round(raw, lo, hi):
    return 100 if hi == 0 else (200 * (hi + lo - raw) + hi) // (2 * hi)


def _from0(f):
    """InterPodAffinity: the term of node j among the raw scores of the feasible nodes, extremes from 0 (scoring.go:247-256)"""
    return lambda raws, j: f(raws[j], min(0, min(raws)), max(0, max(raws)))


def _over(f):
    """PodTopologySpread: extremes over the scored nodes"""
    return lambda raws, j: f(raws[j], min(raws), max(raws))


@dataclass(frozen=True)
class TermArith:
    name: str
    ipa: callable = _from0(ipa_exact)
    pts: callable = _over(pts_exact)
    extremes: bool = False               # moves the extremes: the judge's term moves with the probe's


EXACT = TermArith("exact")
KERNEL_FORMS = [TermArith("wide", ipa=_from0(ipa_rcp2), pts=_over(pts_divq_r)), TermArith("generation7", pts=_over(pts_fma_half))]

IPA_KINDS = ("ipa_over", "ipa_unc_up", "ipa_unc_down", "ipa_round", "ipa_min", "ipa_max")
PTS_KINDS = ("pts_naive", "pts_float", "pts_round")
# model -> (arithmetic, the kinds whose every duel it sends to the wrong node)
MODELS = {
    "ipa_int": (TermArith("ipa_int", ipa=_from0(ipa_int)), ("ipa_over", "ipa_unc_up")),
    "ipa_mul_first": (TermArith("ipa_mul_first", ipa=_from0(ipa_mul_first)), ("ipa_over", "ipa_unc_up")),
    "ipa_uncorrected": (TermArith("ipa_uncorrected", ipa=_from0(ipa_uncorrected)), ("ipa_unc_up", "ipa_unc_down")),
    "ipa_round": (TermArith("ipa_round", ipa=_from0(ipa_round)), ("ipa_round",)),
    "ipa_min_not_zero": (TermArith("ipa_min_not_zero", ipa=lambda raws, j: ipa_exact(raws[j], min(raws), max(0, max(raws))), extremes=True), ("ipa_min",)),
    "ipa_max_not_zero": (TermArith("ipa_max_not_zero", ipa=lambda raws, j: ipa_exact(raws[j], min(0, min(raws)), max(raws)), extremes=True), ("ipa_max",)),
    "pts_naive": (TermArith("pts_naive", pts=_over(pts_naive)), ("pts_naive",)),
    "pts_float": (TermArith("pts_float", pts=_over(pts_float)), ("pts_float",)),
    "pts_round": (TermArith("pts_round", pts=_over(pts_round)), ("pts_round",)),
}


def targets(kind):
    return [m for m, (_, kinds) in MODELS.items() if kind in kinds]


# ---- the pair tables ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_tables():
    """kind -> [(x, d)] / [(y, m)], 0 < x <= d <= PAIR_MAX: where the kind's models differ from the exact value in the kind's direction
    and no other scalar model errs the other way.  numpy's binary64 +, *, / are the correctly rounded IEEE operations."""
    d = np.arange(1, PAIR_MAX + 1, dtype=np.float64)[None, :]
    x = np.arange(0, PAIR_MAX + 1, dtype=np.float64)[:, None]
    xi, di = x.astype(np.int64), d.astype(np.int64)
    inside = (xi >= 1) & (xi <= di)
    quo = 100 * xi // di
    frac = 100 * xi % di / d
    t = lambda v: np.trunc(v).astype(np.int64)
    exact = t(100.0 * (x / d))
    i_int, i_unc, i_mul = quo - exact, t(100.0 * (x * (1.0 / d))) - exact, t((100.0 * x) / d) - exact
    p_naive, p_float = t((100.0 * x) * (1.0 / d)) - quo, exact - quo
    calm_i = (i_int == 0) & (i_unc == 0) & (i_mul == 0)
    sel = {
        "ipa_over": (i_int > 0) & (i_mul > 0) & (i_unc == 0),
        "ipa_unc_up": (i_unc > 0) & (i_int > 0) & (i_mul > 0),
        "ipa_unc_down": (i_unc < 0) & (i_int == 0) & (i_mul == 0),
        "ipa_round": calm_i & (frac >= 0.5) & (frac <= 0.9) & (di <= 120),
        "pts_naive": (p_naive < 0) & (p_float == 0),
        "pts_float": (p_float < 0) & (p_naive == 0),
        "pts_round": (p_naive == 0) & (p_float == 0) & (frac >= 0.5) & (frac <= 0.9) & (di <= 60),
    }
    return {k: [(int(a), int(b) + 1) for a, b in np.argwhere(m & inside)] for k, m in sel.items()}


# ---- a duel ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Row:
    """one counted term of a duel"""
    key: int                 # topology key: 0 hostname-like, 1 / 2 zone-like
    pref_w: int = 0          # the duel class prefers the term with this weight: raw += pref_w * (pods matching it in the domain)
    owned: bool = False      # counter pods OWN the term (weights per group) and the duel class matches it: raw += their weights in the domain
    soft: int = -1           # position in the duel class's soft-constraint list (-1: not a constraint)
    skew: int = 1


@dataclass
class Group:
    """n counter pods of one class on one node: they match `rows` (own them, with these weights, where the row is `owned`)"""
    node: int
    rows: tuple
    n: int
    own_w: dict = field(default_factory=dict)


@dataclass
class TNode:
    cap_c: int
    cap_m: int
    r_c: int                 # NonZeroRequested + the duel pod's request: the state the duel pod is scored on (counter pods included)
    r_m: int
    admitted: bool = True    # False: the ballast node, which only raises the largest counter of the hostname-like row


@dataclass
class TDuel:
    kind: str
    term: str                # "ipa" / "pts": the term the fragile pair sits on
    pair: tuple              # (x, d) / (y, m) of the probe
    nodes: list              # canonical order; nodes[first] wins the exact tie against nodes[first + 1]
    first: int
    probe: int               # index of the probe: first (the models under-estimate it) or first + 1
    rows: list
    groups: list
    q_c: int
    q_m: int
    cq_c: int
    cq_m: int
    flavour: str = "preset"
    laba: list = None        # exact LeastAllocated + BalancedAllocation per node
    direction: int = 0       # -1: the targeted models under-estimate the probe against the judge, +1: over

    @property
    def judge(self):
        return 2 * self.first + 1 - self.probe

    @property
    def soft_rows(self):
        return sorted((r for r in range(len(self.rows)) if self.rows[r].soft >= 0), key=lambda r: self.rows[r].soft)

    @property
    def has_ipa(self):
        return any(r.pref_w or r.owned for r in self.rows)


def duel_raws(duel):
    """-> (InterPodAffinity raw score, PodTopologySpread raw score) per ADMITTED node in canonical order (None: the duel class has no such
    term), from the counters alone -- every key gives every node of a duel its own domain"""
    n = len(duel.nodes)
    cnt = [[0] * n for _ in duel.rows]
    own = [[0] * n for _ in duel.rows]
    for g in duel.groups:
        for r in g.rows:
            if duel.rows[r].owned:
                own[r][g.node] += g.n * g.own_w[r]
            else:
                cnt[r][g.node] += g.n
    adm = [j for j in range(n) if duel.nodes[j].admitted]
    ipa = pts = None
    if duel.has_ipa:
        ipa = [sum(row.pref_w * cnt[r][j] + own[r][j] for r, row in enumerate(duel.rows)) for j in adm]
    soft = duel.soft_rows
    if soft:
        w = float(spread_log_table(MAX_POS)[len(adm)])           # hostname-like: the scored nodes; zone-like: their distinct domains -- the same here
        pts = []
        for j in adm:
            s = 0.0
            for r in soft:
                s = s + (float(cnt[r][j]) * w + float(duel.rows[r].skew - 1))
            assert abs(s - round(s)) > 1e-6 or all(cnt[r][j] == 0 for r in soft), (s, "a raw spread score next to an integer")
            pts.append(int(s))
    return ipa, pts


def term_totals(duel, ar):
    """weighted normalised terms of the admitted nodes under `ar`"""
    ipa, pts = duel_raws(duel)
    k = len(ipa if ipa is not None else pts)
    return [(W_IPA * ar.ipa(ipa, j) if ipa is not None else 0) + (W_PTS * ar.pts(pts, j) if pts is not None else 0) for j in range(k)]


def duel_pick(duel, ar):
    """index (within the duel) of the node the duel pod goes to under `ar`: first maximum in canonical order"""
    adm = [j for j in range(len(duel.nodes)) if duel.nodes[j].admitted]
    best, best_total = -1, 0
    for j, t in zip(adm, term_totals(duel, ar)):
        if best < 0 or duel.laba[j] + t > best_total:
            best, best_total = j, duel.laba[j] + t
    return best


def describe(duel):
    return f"kind {duel.kind}, {duel.term} pair {duel.pair}, exact node {duel.first}, a slip's node {duel.first + 1} (probe {duel.probe}) of the duel"


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def _state_in(rng, cap_c, cap_m, lo, hi):
    """a state whose exact LeastAllocated + BalancedAllocation lies in [lo, hi] and that every model of duel_util leaves alone"""
    for _ in range(600):
        cf, mf = rng.uniform(0.02, 0.97), rng.uniform(0.02, 0.97)
        if rng.random() < 0.5:
            mf = min(0.97, max(0.02, cf + rng.uniform(-0.05, 0.05)))
        r_c, r_m = int(cf * cap_c), int(mf * cap_m)
        t = U.laba(U.EXACT, r_c, cap_c, r_m, cap_m)
        if lo <= t <= hi and min(r_c, r_m) >= U.MIN_STATE and all(U.laba(m, r_c, cap_c, r_m, cap_m) == t for m in U._LABA_MODELS):
            return r_c, r_m, t
    return None


def _split(rng, v):
    """a value as weight x count"""
    for c in rng.permutation([3, 2]):
        if v % int(c) == 0 and rng.random() < 0.6:
            return v // int(c), int(c)
    return v, 1


def _realise_ipa(rng, values, form, zone_only=False):
    """rows and groups whose counters give node j the raw score values[j].  "self": one row per distinct value, at most one on the
    hostname-like key, one weight per owner (what generation 7 accepts); "general": two hostname-like rows per value, one of them with a
    negative weight, or two owner classes with different weights on one term (the all-feature kernel only)."""
    distinct = sorted({v for v in values if v}, key=lambda v: rng.random())
    rows, groups = [], []
    if form == "self":
        keys = [1, 2, 1] if zone_only else [int(k) for k in rng.permutation([0, 1, 2])] + [1]
        if len(distinct) > len(keys):
            return None
        for v, key in zip(distinct, keys):
            w, c = _split(rng, abs(v))
            w = w if v > 0 else -w
            owned = rng.random() < 0.35
            rows.append(Row(key, 0 if owned else w, owned))
            for j, vj in enumerate(values):
                if vj == v:
                    groups.append(Group(j, (len(rows) - 1,), c, {len(rows) - 1: w} if owned else {}))
        return rows, groups
    for v in distinct:
        e = int(rng.integers(1, 40))
        if rng.random() < 0.5:                                   # two preferred terms on the hostname-like key, one weight negative
            rows += [Row(0, v + e), Row(int(rng.integers(0, 3)), -e)]
            for j, vj in enumerate(values):
                if vj == v:
                    groups.append(Group(j, (len(rows) - 2, len(rows) - 1), 1))
        else:                                                    # two owner classes with different weights on one term
            rows.append(Row(0, 0, True))
            for j, vj in enumerate(values):
                if vj == v:
                    groups += [Group(j, (len(rows) - 1,), 1, {len(rows) - 1: v + e}), Group(j, (len(rows) - 1,), 1, {len(rows) - 1: -e})]
    return rows, groups


def _ipa_values(kind, rng, sign):
    """raw scores of (anchors ..., probe, judge) and the pair"""
    if kind in ("ipa_min", "ipa_max"):
        d = int(rng.integers(20, PAIR_MAX))
        x, xj = int(rng.integers(1, d)), int(rng.integers(1, d))
        vals = [d, x, xj] if kind == "ipa_min" else [-d, x - d, xj - d]
        return vals, (x, d)
    table = pair_tables()[kind]
    x, d = table[int(rng.integers(len(table)))]
    k = ipa_exact(x, 0, d)
    for _ in range(200):
        xj = int(rng.integers(0, d + 1))
        kj = ipa_exact(xj, 0, d)
        if kj != k and abs(kj - k) <= 45 and all(f(xj, 0, d) == kj for f in (ipa_int, ipa_uncorrected, ipa_mul_first, ipa_round, ipa_rcp2)):
            break
    else:
        return None
    if sign > 0:
        return [d, 0, x, xj], (x, d)
    return [-d, 0, x - d, xj - d], (x, d)


def _pts_counts(kind, rng, n_soft, n_adm):
    """counter values of (anchors ..., probe, judge), the constant K = sum (maxSkew - 1) and the pair: the smallest counts that land the
    extremes and the probe on the pair's integers"""
    w = float(spread_log_table(MAX_POS)[n_adm])
    cmax = 30

    def base(c):
        s = 0.0
        for _ in range(n_soft):
            s = s + (float(c) * w + 0.0)
        return int(s)

    b = [base(c) for c in range(cmax + 2)]
    table = pair_tables()[kind]
    for _ in range(60):
        y, m = table[int(rng.integers(len(table)))]
        found = []
        for has_lo in (0, 1):
            if has_lo and n_adm < 4:
                continue
            for c_p in range(cmax + 1):
                for c_j in range(cmax + 1):
                    c_min = 0 if has_lo else min(c_p, c_j)
                    if m + b[c_min] - b[c_p] != y or c_j == c_p:
                        continue
                    c_hi = max(c_p, c_j) + 1
                    if b[c_hi] == b[max(c_p, c_j)]:
                        c_hi += 1
                    if c_hi > cmax + 1 or b[c_hi] > m:
                        continue
                    y_j = m + b[c_min] - b[c_j]
                    k_j = 100 * y_j // m
                    if any(f(m + b[c_min] - y_j, b[c_min], m) != k_j for f in (pts_naive, pts_float, pts_round, pts_fma_half, pts_divq_r)):
                        continue
                    if abs(k_j - 100 * y // m) > 40:
                        continue
                    found.append((c_p + c_j + c_hi, has_lo, c_p, c_j, c_hi))
        if not found:
            continue
        found.sort()
        _, has_lo, c_p, c_j, c_hi = found[int(rng.integers(min(3, len(found))))]
        n_anchor = n_adm - 2
        anchors = [c_hi] + ([0] if has_lo else []) + [c_hi] * (n_anchor - 1 - has_lo)
        return anchors + [c_p, c_j], m - b[c_hi], (y, m)
    return None


def _quiet_counts(rng, n_adm):
    """small counters for the spread term of a duel whose fragile pair sits on the other term (gen_duel keeps them only where no model
    moves the spread terms of the pair)"""
    while True:
        counts = [int(rng.integers(0, 4)) for _ in range(n_adm)]
        if max(counts) > min(counts):
            return counts, int(rng.integers(0, 30))


def gen_duel(kind, rng, caps, form="self", sign=1, layouts=((0,),), with_other=False, flavour="preset", ballast=0):
    """One duel.  caps: a function (index of the node in the duel) -> (cap_c, cap_m).  layouts: the key lists a spread duel may take for
    its soft constraints.  with_other: the duel class carries BOTH terms (the other one on pairs that no model moves).  ballast: that many
    counter pods of the hostname-like row on one more node, which the duel class is not admitted to."""
    term = "ipa" if kind in IPA_KINDS else "pts"
    for _ in range(400):
        rows, groups = [], []
        layout = layouts[int(rng.integers(len(layouts)))]
        if term == "ipa":
            got = _ipa_values(kind, rng, sign)
            if got is None:
                continue
            values, pair = got
            k_adm = len(values)
            counts, K = _quiet_counts(rng, k_adm) if with_other else (None, 0)
        else:
            k_adm = int(rng.integers(4, 8))
            got = _pts_counts(kind, rng, len(layout), k_adm)
            if got is None:
                continue
            counts, K, pair = got
            values = None
            if with_other:
                d = int(rng.integers(10, 200))
                values = [d * int(sign)] + [0] * (k_adm - 3) + [int(rng.integers(0, d + 1)) * int(sign) for _ in range(2)]
        if counts is not None:
            split = int(rng.integers(0, K + 1)) if len(layout) > 1 else K
            for e, key in enumerate(layout):
                rows.append(Row(key, soft=e, skew=1 + (split if e == 0 else K - split if e == 1 else 0)))
            srows = tuple(range(len(layout)))
            groups += [Group(j, srows, c) for j, c in enumerate(counts) if c]
        if values is not None:
            vals = list(values)
            host_soft = [r for r in range(len(rows)) if rows[r].key == 0]
            if counts is not None and host_soft and rng.random() < 0.5:      # the preferred term on the row the spread constraint counts
                wh = int(rng.integers(1, 4)) * int(sign)
                rows[host_soft[0]].pref_w = wh
                vals = [v - wh * c for v, c in zip(values, counts)]
            got = _realise_ipa(rng, vals, form, zone_only=bool(host_soft))
            if got is None:
                continue
            r0 = len(rows)
            rows += got[0]
            groups += [Group(g.node, tuple(r + r0 for r in g.rows), g.n, {r + r0: w for r, w in g.own_w.items()}) for g in got[1]]
        # canonical order: the anchors, the ballast node, then the pair (probe first for now)
        nodes = [TNode(0, 0, 0, 0) for _ in range(k_adm)]
        if ballast:
            host = [r for r in range(len(rows)) if rows[r].key == 0 and (rows[r].soft >= 0 or rows[r].pref_w or rows[r].owned)]
            if not host:
                continue
            nodes.insert(k_adm - 2, TNode(0, 0, 0, 0, admitted=False))
            for g in groups:
                g.node += g.node >= k_adm - 2
            r = host[0]
            groups.append(Group(k_adm - 2, (r,), ballast, {r: next(g.own_w[r] for g in groups if r in g.own_w)} if rows[r].owned else {}))
        if len(nodes) > MAX_POS:
            continue
        duel = TDuel(kind, term, pair, nodes, len(nodes) - 2, len(nodes) - 2, rows, groups, int(rng.integers(U.Q_LO, U.Q_HI)), int(rng.integers(U.Q_LO, U.Q_HI)),
                     int(rng.integers(CQ_LO, CQ_HI)), int(rng.integers(CQ_LO, CQ_HI)), flavour)
        ipa_r, pts_r = duel_raws(duel)
        if term == "ipa":                                          # the pair the counters really give
            lo0, hi0 = min(0, min(ipa_r)), max(0, max(ipa_r))
            if (ipa_r[k_adm - 2] - lo0, hi0 - lo0) != pair:
                continue
        elif (max(pts_r) + min(pts_r) - pts_r[k_adm - 2], max(pts_r)) != pair:
            continue
        exact = term_totals(duel, EXACT)
        for ar in KERNEL_FORMS:
            if term_totals(duel, ar) != exact:
                raise AssertionError(f"the kernel form {ar.name} differs from the exact reference on {describe(duel)}: {duel_raws(duel)}")
        ip, ij = k_adm - 2, k_adm - 1                              # probe and judge among the admitted nodes
        rel = {}
        for name, (ar, kinds) in MODELS.items():
            t = term_totals(duel, ar)
            rel[name] = ((t[ip] - exact[ip]) - (t[ij] - exact[ij]), t[ip] - exact[ip], t[ij] - exact[ij], ar.extremes)
        mine = targets(kind)
        signs = {(rel[m][0] > 0) - (rel[m][0] < 0) for m in mine} | {(rel[m][1] > 0) - (rel[m][1] < 0) for m in mine}
        if len(signs) != 1 or 0 in signs:
            continue                                               # teeth: every targeted model moves the probe, all in one direction
        direction = signs.pop()
        if any((r[0] * direction < 0 or (r[2] != 0 and m not in mine)) for m, r in rel.items() if not r[3] or m in mine):
            continue                                               # ... and no other model moves the judge or pulls the other way
        if any(r[2] != 0 for m, r in rel.items() if m in mine and not r[3]):
            continue
        # the tie: probe total = judge total > every anchor's (anchors are exactly full on cpu: LeastAllocated + BalancedAllocation 0)
        tp, tj, ta = exact[ip], exact[ij], max(exact[:ip])
        lo, hi = max(30, 30 + tj - tp, ta - tp + 1), min(196, 196 + tj - tp)
        if lo > hi:
            continue
        cp, cj = caps(len(nodes) - 2), caps(len(nodes) - 1)
        got = _state_in(rng, cp[0], cp[1], lo, hi)
        if got is None:
            continue
        pc, pm, pt = got
        judge = U._find_judge(rng, cj[0], cj[1], pt + tp - tj)
        if judge is None:
            continue
        per_node = [sum(g.n for g in groups if g.node == j) for j in range(len(nodes))]
        if min(pc, pm, judge[0], judge[1]) < U.MIN_STATE or max(per_node) * max(duel.cq_c, duel.cq_m) + max(duel.q_c, duel.q_m) >= U.MIN_STATE:
            continue
        for j in range(len(nodes) - 2):
            cc, cm = caps(j)
            nodes[j].cap_c, nodes[j].cap_m, nodes[j].r_c, nodes[j].r_m = cc, cm, cc, int(rng.uniform(0.985, 0.995) * cm)
        nodes[-2].cap_c, nodes[-2].cap_m, nodes[-2].r_c, nodes[-2].r_m = cp[0], cp[1], pc, pm
        nodes[-1].cap_c, nodes[-1].cap_m, nodes[-1].r_c, nodes[-1].r_m = cj[0], cj[1], judge[0], judge[1]
        if direction > 0:                                          # the models over-estimate the probe: it comes second
            a, b = len(nodes) - 2, len(nodes) - 1
            nodes[a], nodes[b] = nodes[b], nodes[a]
            for g in groups:
                g.node = b if g.node == a else a if g.node == b else g.node
            duel.probe = b
        duel.direction = direction
        duel.laba = [U.laba(U.EXACT, n.r_c, n.cap_c, n.r_m, n.cap_m) for n in nodes]
        if duel_pick(duel, EXACT) != duel.first or any(duel_pick(duel, MODELS[m][0]) == duel.first for m in mine):
            continue
        return duel
    raise RuntimeError(f"no {kind} duel found")


# ---- the problem ------------------------------------------------------------------------------------------------------------------------------
def build(seed, kinds, n_duels, form="self", flavour="preset", shapes="one", signs=(1,), layouts=((0,),), with_other=False, ballast=None):
    """-> (capi.Problem, orders [4][P], expected placement [P], duels, duel of every pod [P]).  flavour "preset" / "placed" / "mixed" (by
    duel in turn); shapes "one": every node of the problem has one capacity shape (few internal node classes: only the zone split tells them
    apart), "distinct": every node its own (one internal class per node); ballast = (every k-th duel, pods)."""
    rng = np.random.default_rng(seed)
    shape = (U._odd(rng, 1 << 28, 1 << 30), U._odd(rng, 1 << 28, 1 << 30))
    seen = {shape}

    def caps(_):
        if shapes == "one":
            return shape
        while True:
            s = (U._odd(rng, 1 << 28, 1 << 30), U._odd(rng, 1 << 28, 1 << 30))
            if s not in seen:
                seen.add(s)
                return s

    duels = []
    for d in range(n_duels):
        fl = ("preset", "placed")[d % 2] if flavour == "mixed" else flavour
        bl = ballast[1] if ballast and d % ballast[0] == ballast[0] - 1 else 0
        duels.append(gen_duel(kinds[d % len(kinds)], rng, caps, form, signs[(d // len(kinds)) % len(signs)], layouts, with_other, fl, bl))
    N = sum(len(d.nodes) for d in duels)
    a_c, a_m, i_c, i_m = [], [], [], []
    topo = np.full((3, N), -1, np.int32)
    req_c, req_m, pcls, preset, gate, expected, pod_duel = [], [], [], [], [], [], []
    masks, term_key = [], []
    lists = {k: [] for k in ("match", "pref", "pref_w", "own", "own_w", "soft", "skew")}      # per pod class
    j0 = 0

    def new_class(admit, **kw):
        row = np.zeros((N + 63) // 64, np.uint64)
        for j in admit:
            row[j // 64] |= np.uint64(1) << np.uint64(j % 64)
        masks.append(row)
        for k in lists:
            lists[k].append(list(kw.get(k, ())))
        return len(masks) - 1

    for d, duel in enumerate(duels):
        t0 = len(term_key)
        term_key += [r.key for r in duel.rows]
        for i, n in enumerate(duel.nodes):
            k = sum(g.n for g in duel.groups if g.node == i)
            a_c.append(n.cap_c); a_m.append(n.cap_m)
            adm = 1 if n.admitted else 0
            i_c.append(n.r_c - adm * duel.q_c - k * duel.cq_c if n.admitted else int(rng.integers(1 << 20, 1 << 24)))
            i_m.append(n.r_m - adm * duel.q_m - k * duel.cq_m if n.admitted else int(rng.integers(1 << 20, 1 << 24)))
            assert i_c[-1] >= 0 and i_m[-1] >= 0
            topo[0, j0 + i], topo[1, j0 + i], topo[2, j0 + i] = j0 + i, i, (3 * i + 1) % MAX_POS
        last = j0 + len(duel.nodes) - 1
        for g in duel.groups:
            c = new_class([j0 + g.node], match=[t0 + r for r in g.rows if not duel.rows[r].owned],
                          own=[t0 + r for r in g.rows if duel.rows[r].owned], own_w=[g.own_w[r] for r in g.rows if duel.rows[r].owned])
            for _ in range(g.n):
                req_c.append(duel.cq_c); req_m.append(duel.cq_m); pcls.append(c); gate.append(last); pod_duel.append(d)
                preset.append(j0 + g.node if duel.flavour == "preset" else -1)
                expected.append(j0 + g.node)
        soft = duel.soft_rows
        c = new_class([j0 + i for i, n in enumerate(duel.nodes) if n.admitted],
                      match=[t0 + r for r, row in enumerate(duel.rows) if row.owned or row.soft >= 0],
                      pref=[t0 + r for r, row in enumerate(duel.rows) if row.pref_w], pref_w=[row.pref_w for row in duel.rows if row.pref_w],
                      soft=[t0 + r for r in soft], skew=[duel.rows[r].skew for r in soft])
        req_c.append(duel.q_c); req_m.append(duel.q_m); pcls.append(c); gate.append(last); pod_duel.append(d); preset.append(-1)
        expected.append(j0 + duel.first)
        j0 += len(duel.nodes)
    Cp = len(masks)
    csr = lambda name: np.cumsum([0] + [len(v) for v in lists[name]]).astype(np.int32)
    flat = lambda name: np.array([x for v in lists[name] for x in v] or [0], np.int32)
    reason = np.full((Cp, N), capi.REASON_NODE_AFFINITY, np.uint8)
    for c, row in enumerate(masks):
        for j in range(N):
            if (int(row[j // 64]) >> (j % 64)) & 1:
                reason[c, j] = 0
    prob = capi.Problem(alloc_cpu=np.array(a_c, np.int64), alloc_mem=np.array(a_m, np.int64), alloc_pods=np.full(N, 110, np.int32),
                        node_class=np.zeros(N, np.int32), init_req_cpu=np.array(i_c, np.int64), init_req_mem=np.array(i_m, np.int64),
                        init_nz_cpu=np.array(i_c, np.int64), init_nz_mem=np.array(i_m, np.int64),
                        req_cpu=np.array(req_c, np.int64), req_mem=np.array(req_m, np.int64), nz_cpu=np.array(req_c, np.int64), nz_mem=np.array(req_m, np.int64),
                        pod_class=np.array(pcls, np.int32), gate_node=np.array(gate, np.int32), preset_node=np.array(preset, np.int32),
                        n_pod_classes=Cp, n_node_classes=1, static_mask=np.array(masks, np.uint64), static_reason=reason,
                        simon_raw=np.full((Cp, 1), 57, np.int64),
                        topo_dom=topo, topo_n_dom=np.array([N, MAX_POS, MAX_POS], np.int32), topo_is_hostname=np.array([1, 0, 0], np.uint8),
                        term_topo_key=np.array(term_key, np.int32), match_off=csr("match"), match_idx=flat("match"),
                        spread_log=spread_log_table(N))
    if any(lists["pref"]):
        prob.pref_off, prob.pref_idx, prob.pref_w = csr("pref"), flat("pref"), flat("pref_w")
    if any(lists["own"]):
        prob.own_off, prob.own_idx, prob.own_w = csr("own"), flat("own"), flat("own_w")
    if any(lists["soft"]):
        prob.spread_soft_off, prob.spread_soft_idx, prob.spread_soft_skew = csr("soft"), flat("soft"), flat("skew")
    prob.normalise()
    # the domain of the narrow route (simon_hip.hip: choose_variant): gcd 1, largest node + all pods below 2^31; byte counters
    for alloc, irq, prq in ((prob.alloc_cpu, prob.init_req_cpu, prob.req_cpu), (prob.alloc_mem, prob.init_req_mem, prob.req_mem)):
        g = 0
        for arr in (alloc, irq, prq):
            g = math.gcd(g, int(np.gcd.reduce(arr)))
        assert g == 1, g
        assert max(int(alloc.max()), int(irq.max())) + int(prq.sum()) < U.LIM31
    assert len({(d.q_c, d.q_m) for d in duels}) == len(duels)
    pod_duel = np.array(pod_duel, np.int32)
    return prob, _orders(rng, pod_duel), np.array(expected, np.int32), duels, pod_duel


def _orders(rng, pod_duel):
    """four permutations of the pods that keep a duel's counter pods ahead of its duel pod (the last pod of the duel)"""
    D = int(pod_duel.max()) + 1
    pods = [np.nonzero(pod_duel == d)[0].tolist() for d in range(D)]
    o0 = [p for d in range(D) for p in pods[d]]
    o1 = [p for d in reversed(range(D)) for p in pods[d][:-1][::-1] + pods[d][-1:]]
    o2 = [p for d in rng.permutation(D) for p in pods[int(d)][:-1]] + [pods[int(d)][-1] for d in rng.permutation(D)]
    keys = np.empty(len(pod_duel))
    for d in range(D):
        keys[pods[d]] = np.sort(rng.random(len(pods[d])))
    o3 = [int(p) for p in np.argsort(keys, kind="stable")]
    return np.array([o0, o1, o2, o3], np.int32)


def check_against_oracle(prob, orders, duels, pod_duel):
    """Every duel, before anything else sees it: the C oracle's per-node totals of the duel pod (all of its counter pods scheduled) --
    probe and judge equal, every other admitted node strictly below, and total = LeastAllocated + BalancedAllocation + the terms that
    duel_raws derives from the counters."""
    import oracle_lib as O
    order = orders[0].tolist()
    j0 = 0
    for d, duel in enumerate(duels):
        pod = int(np.nonzero(pod_duel == d)[0][-1])
        best, sc = O.score_pod_after(prob, prob.n_nodes, order.index(pod), pod, orders[0])
        adm = [j for j in range(len(duel.nodes)) if duel.nodes[j].admitted]
        want = [duel.laba[j] + t for j, t in zip(adm, term_totals(duel, EXACT))]
        got = [int(sc["total"][j0 + j]) for j in adm]
        feas = [int(sc["feasible"][j0 + j]) for j in range(len(duel.nodes))]
        assert feas == [int(n.admitted) for n in duel.nodes] and int(sc["feasible"].sum()) == len(adm), (d, feas)
        assert got == want, (d, describe(duel), got, want)
        a, b = adm.index(duel.first), adm.index(duel.first + 1)
        assert got[a] == got[b] and all(got[i] < got[a] for i in range(len(adm)) if i not in (a, b)), (d, got)
        assert best == j0 + duel.first, (d, best)
        j0 += len(duel.nodes)


# ---- route facts, derived from the problem alone -----------------------------------------------------------------------------------------------
def route_facts(fx):
    """What decides a fixture's way through generation 7, from the fixture alone:
      classes   internal node classes = distinct (allocatable cpu, allocatable memory, domains on the zone-like keys in use) -- simon_hip.hip,
                stage_narrow: `key = make_tuple(content_of[node_class[j]], a_cpu[j], a_mem[j], spread ? zone_sub(j) : ...)`; beyond
                kTableMaxClasses = 64 the CN2 instantiations run
      per duel  simple = nh == 0 || (nh == 1 && eh == 0 && soft_n <= 2)   (simon_table.hip, spread_select: `const bool simple = ...`),
                tabulated = simple && (classes << lg) <= TABMAX, lg = bit length of the largest counter of the pod's hostname-like row
                (`const int lg = 32 - __clz(hmx); const int E = Cn << lg; if (simple && E <= TABMAX)`), TABMAX = SIMON_SPREAD_TAB_MAX
                (512) or SIMON_SPREAD_TAB_MAX2 (2 048) under CN2 (simon_table.h)."""
    prob = fx.prob
    zone_keys = sorted({int(prob.term_topo_key[t]) for t in range(len(prob.term_topo_key))} - {0})
    classes = {(int(prob.alloc_cpu[j]), int(prob.alloc_mem[j]), tuple(int(prob.topo_dom[k, j]) for k in zone_keys)) for j in range(prob.n_nodes)}
    Cn = len(classes)
    tabmax = SPREAD_TAB_MAX2 if Cn > TABLE_MAX_CLASSES else SPREAD_TAB_MAX
    per = []
    for duel in fx.duels:
        soft = duel.soft_rows
        host = [e for e, r in enumerate(soft) if duel.rows[r].key == 0]
        nh = len(host)
        simple = nh == 0 or (nh == 1 and host[0] == 0 and len(soft) <= 2)
        ipa_host = [r for r, row in enumerate(duel.rows) if row.key == 0 and (row.pref_w or row.owned)]
        hrow = soft[host[0]] if nh == 1 else (ipa_host[0] if nh == 0 and ipa_host else None)
        hmax = 0
        if hrow is not None and simple:
            hmax = max(sum(g.n for g in duel.groups if g.node == j and hrow in g.rows) for j in range(len(duel.nodes)))
        E = Cn << hmax.bit_length()
        per.append({"simple": simple, "entries": E, "tabulated": simple and E <= tabmax, "n_host_ipa": len(ipa_host), "nh": nh})
    return {"classes": Cn, "cn2": Cn > TABLE_MAX_CLASSES, "duels": per}


# ---- the named fixtures ------------------------------------------------------------------------------------------------------------------------
@dataclass
class TermFixture(U.Fixture):
    pod_duel: np.ndarray = None
    form: str = "self"


SELF_IPA = ("ipa_over", "ipa_unc_up", "ipa_unc_down", "ipa_round", "ipa_min")
SIMPLE_LAYOUTS = ((0,), (0, 1), (0, 2), (1,), (1, 2))
WALK_LAYOUTS = ((1, 0), (0, 1, 2), (2, 0, 1), (2, 0))
# name -> (seed, kinds, duels, arguments of build)
FIXTURES = {
    "ipa_self_preset": (31, SELF_IPA, 15, {"flavour": "preset"}),
    "ipa_self_placed": (32, SELF_IPA, 15, {"flavour": "placed"}),
    # one capacity shape per node and 16 pods on a further node of the hostname-like row: classes << 5 > 512, the general walk scores it
    "ipa_self_walk": (39, SELF_IPA, 10, {"flavour": "mixed", "shapes": "distinct", "ballast": (1, 16)}),
    "ipa_general": (33, IPA_KINDS, 12, {"form": "general", "flavour": "mixed", "signs": (1, -1)}),
    "ipa_negative": (34, ("ipa_over", "ipa_unc_up", "ipa_unc_down", "ipa_round", "ipa_max"), 15, {"flavour": "mixed", "signs": (-1,)}),
    "pts_simple": (35, PTS_KINDS, 12, {"flavour": "mixed", "layouts": SIMPLE_LAYOUTS}),
    "pts_walk": (36, PTS_KINDS, 12, {"flavour": "mixed", "layouts": WALK_LAYOUTS}),
    "pts_ipa_self": (37, ("ipa_over", "pts_naive", "ipa_unc_down", "pts_float", "ipa_unc_up", "pts_round", "ipa_round"), 14,
                     {"flavour": "mixed", "layouts": ((0,), (0, 1)), "with_other": True}),
    "cn2": (38, ("ipa_over", "pts_naive", "ipa_unc_down", "pts_float", "ipa_unc_up", "pts_round", "ipa_round"), 14,
            {"flavour": "mixed", "layouts": ((0,), (0, 1)), "with_other": True, "shapes": "distinct", "ballast": (2, 16)}),
}
MAX_DUELS, MAX_NODES, MAX_PODS = 16, 130, 1500


@functools.lru_cache(maxsize=None)
def fixture(name):
    seed, kinds, n, extra = FIXTURES[name]
    prob, orders, expected, duels, pod_duel = build(seed, kinds, n, **extra)
    assert n <= MAX_DUELS and prob.n_nodes <= MAX_NODES and prob.n_pods <= MAX_PODS, (name, n, prob.n_nodes, prob.n_pods)
    check_against_oracle(prob, orders, duels, pod_duel)
    ends = np.cumsum([len(d.nodes) for d in duels])
    N = prob.n_nodes
    scen = [[N, o] for o in range(len(orders))] + [[int(ends[n // 3 - 1]), 1], [int(ends[2 * n // 3 - 1]), 2]]
    return TermFixture(name, prob, orders, expected, np.array(scen, np.int32), duels, tuple(kinds), pod_duel, extra.get("form", "self"))

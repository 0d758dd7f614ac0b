#!/usr/bin/env python3
"""Randomised parity sweep of SEGMENTED batches on the all-feature kernel's own-nodes run forms (simon_set_own_nodes_all_feature,
simon_wide_own.hip).  Two regimes:

  mix    fuzz_mix's own cases (draw, reference, compare through fuzz_mix.one_case) with a device function that sets the option and
         SIMON_FORCE_WIDE=1, so that every case fuzz_mix runs on the score-table kernel runs here on the all-feature kernel: 1 ... 8
         segments, caller rank rows, gates, pins, priorities, plan caps, up to 3 000 nodes;
  local  cases from LOCAL_FIRST on: fuzz_mix's draw with the problem drawn again with Open-Local storage (randprob local=True) next to
         the case's other features; used_vg of every scenario is compared too.

Every placement, unscheduled count, used cpu / memory (/ volume-group bytes), GPU slice, preempt-risk flag and plan of every scenario
is compared with the CPU oracle on that scenario's own node set.  A case the library refuses counts as a mismatch: with the option on
nothing is refused.  Not collected by pytest; by hand on a GPU box, each process under a time limit of its own:

    timeout 600 python tests/fuzz_own_wide.py [n_cases] [first_case] [--verbose]"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401
import fuzz_mix as FM  # noqa: E402
import mix_util as MU  # noqa: E402
import randprob  # noqa: E402
from open_simulator_amd import capi  # noqa: E402

LOCAL_FIRST = 100000
_DROP = ("SIMON_TABLE_COARSE", "SIMON_LDS_WS", "SIMON_NO_GPU_FOLD", "SIMON_NO_FOLD", "SIMON_TEAM")   # score-table knobs of fuzz_mix's runs


def run_device(inp, env):
    """fuzz_mix.run_device on a context with the option set, under SIMON_FORCE_WIDE=1; adds used_vg.  None: refused."""
    env = {"SIMON_FORCE_WIDE": "1", "SIMON_DEBUG_ROUTE": "1"}
    saved = {k: os.environ.get(k) for k in (*env, *_DROP)}
    for k in _DROP:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        with FM._Stderr(), capi.Context(0) as ctx:
            ctx.set_own_nodes_all_feature(True)
            ctx.load_problem(inp.prob)
            ctx.load_scenarios(inp.scen, inp.orders)
            ctx.set_scenario_segments(inp.seg_start, inp.counts)
            if inp.ranks is not None:
                ctx.set_node_ranks(inp.ranks)
            try:
                ctx.run_loaded(True, inp.want_gpu)
            except capi.SimonError as e:
                if getattr(e, "code", None) != capi.ESTATE:
                    raise
                return None
            res = ctx.fetch(True, inp.want_gpu)
            out = SimpleNamespace(placement=res.placement, unscheduled=res.unscheduled, used_cpu=res.used_cpu, used_mem=res.used_mem,
                                  used_vg=res.used_vg, gpu_slices=res.gpu_slices if inp.want_gpu else None,
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
    out.route = dict(variant=st.kernel_variant, generation=st.kernel_generation, wg=st.workgroup_size, lds=int(st.lds_bytes), env=env)
    return out


def one_mix_case(case):
    """(ok, info) of fuzz_mix's case on the all-feature kernel; its runs differ in score-table knobs only, so one of them is made."""
    calls = []

    def device(inp, env):
        if calls:
            return None
        calls.append(run_device(inp, env))
        return calls[0]
    ok, info = FM.one_case(case, device=device)
    wide = bool(calls) and calls[0] is not None and calls[0].route["variant"] == capi.KERNEL_WIDE and calls[0].route["generation"] == 0
    if not wide:
        info["bad"] = info["bad"] + ["refused" if not calls or calls[0] is None else "not the all-feature kernel"]
    return ok and wide, info


def draw_local(case):
    """fuzz_mix's draw of `case` with the problem drawn again with Open-Local storage; the segments, counts, orders and ranks stay."""
    inp = FM.draw(case)
    feat = {k: v for k, v in inp.feat.items() if k != "priority"}
    prob = randprob.rand_problem(74000 + case, N=inp.N, P=inp.P, n_node_classes=inp.n_node_classes, n_pod_classes=inp.n_pod_classes, local=True, **feat)
    if inp.prob.priority is not None:
        prob.priority, prob.init_min_priority = inp.prob.priority, inp.prob.init_min_priority
    inp.prob, _ = MU.segmentable(prob, fixed=inp.F)
    inp.want_gpu = inp.prob.gpu_mem is not None
    inp.feat = dict(inp.feat, local=True)
    return inp


def one_local_case(case):
    inp = draw_local(case)
    ref = FM.reference(inp)
    vg = np.zeros(inp.S, np.int64)
    for s in range(inp.S):                                             # (reference() keeps no used_vg: once more for it)
        _, r = MU.oracle_of_scenario(inp.prob, FM.present_of(inp, s), inp.orders[inp.scen[s, 1]], None if inp.ranks is None else inp.ranks[s])
        vg[s] = r.used_vg[0]
    out = run_device(inp, {})
    if out is None:
        bad = ["refused"]
    else:
        bad = FM.compare(inp, ref, out)
        if out.used_vg is None or np.asarray(out.used_vg).tolist() != vg.tolist():
            bad.append("used_vg")
        if (out.route["variant"], out.route["generation"]) != (capi.KERNEL_WIDE, 0):
            bad.append("not the all-feature kernel")
    info = dict(case=case, kind="local", sub=inp.sub, N=inp.N, P=inp.P, S=inp.S, segs=FM.n_segments(inp), F=inp.F, feat=sorted(inp.feat),
                classes=inp.n_node_classes, ranks=inp.ranks is not None, unscheduled=int(ref.unscheduled.sum()), used_vg=int(vg.sum()), bad=bad)
    return not bad, info


def one_case(case):
    return one_local_case(case - LOCAL_FIRST) if case >= LOCAL_FIRST else one_mix_case(case)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_cases = int(args[0]) if len(args) > 0 else 40
    first = int(args[1]) if len(args) > 1 else 0
    bad = multi = unsched = 0
    for case in range(first, first + n_cases):
        ok, info = one_case(case)
        if "--verbose" in sys.argv:
            print("CASE", info, flush=True)
        multi += info.get("segs", 0) > 1
        unsched += info.get("unscheduled", 0) > 0
        if not ok:
            bad += 1
            print("MISMATCH", info, flush=True)
    print(f"fuzz_own_wide: {n_cases} cases from {first} ({'local' if first >= LOCAL_FIRST else 'mix'} regime), with two or more segments {multi}, "
          f"with unscheduled pods {unsched}, mismatches {bad}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

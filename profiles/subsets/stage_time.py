"""Staging time of a node-subset batch against the same batch as one pool segment (profiles/subsets/README.md).

    python profiles/subsets/stage_time.py nodes      # simon_set_scenario_nodes; SIMON_SUBSET_STAGE=host times the host loops
    python profiles/subsets/stage_time.py segments   # simon_set_scenario_segments, one segment behind the smallest size

The batch is config 3's (synth.config3: 1 512 nodes, 1 024 sizes x 4 orders = 4 096 scenarios, seed in synth.SEED); every call ends in
a stream synchronise, so the host clock around it is the call's time.  SUBSETS_TREE=<dir> imports the package from another checkout
(the parent commit's, for the alternated pairs): `segments` needs nothing this tree adds."""
import json
import os
import sys
import time

ROOT = os.environ.get("SUBSETS_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from open_simulator_amd import capi, synth  # noqa: E402


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "nodes"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    prob, scen, orders = synth.config3()
    N, F = prob.n_nodes, int(scen[:, 0].min())
    mask = np.arange(N)[None, :] < scen[:, :1]
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        if mode == "nodes":
            call = lambda: ctx.set_scenario_nodes(mask)                                   # noqa: E731
        else:
            cnt = (scen[:, :1] - F).astype(np.int32)
            call = lambda: ctx.set_scenario_segments([F], cnt)                            # noqa: E731
        call()                                                                            # (first call: buffers, code object)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        ctx.run_loaded(False)
        res = ctx.fetch(False)
    print(json.dumps({"mode": mode, "stage": os.environ.get("SIMON_SUBSET_STAGE", "device") if mode == "nodes" else "host loops",
                      "tree": "other" if os.environ.get("SUBSETS_TREE") else "this", "S": len(scen), "N": N, "ms": ms, "median_ms": float(np.median(ms)),
                      "unscheduled_sum": int(res.unscheduled.sum())}))


if __name__ == "__main__":
    main()

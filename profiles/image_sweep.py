#!/usr/bin/env python3
"""ImageLocality in a batched sweep (ABI v7) against the size-by-size path it replaces.

Workloads (64 candidate sizes each, counts 0..63, a new-node template that lists an image):
  kubeconfig  about 1 000 nodes (3 shapes, 3 zones, about half of them listing the apps' images);
  few_listers 300 nodes in one zone, 3 % of them listing images (what stays within the score table's class limits).
Reports the end-to-end sweep() time of one batch (flatten once, one launch) against sim._sweep_per_size (one flattening + one
one-scenario launch per size), the batch's kernel time (simon_get_stats), which kernel ran, the engine's own node-class counts (its
SIMON_DEBUG_ROUTE lines: classes after the image split, internal classes of the score table) and whether both paths agree.
    python profiles/image_sweep.py [--json OUT]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SIMON_DEBUG_ROUTE"] = "1"           # (read when a context is created: the engine's own class counts)
import conftest  # noqa: E402,F401
import image_util as IU  # noqa: E402
from open_simulator_amd import capi, simulate as sim  # noqa: E402

WORKLOADS = {"kubeconfig": dict(n_nodes=1000, zones=True, listing_share=0.5),
             "few_listers": dict(n_nodes=300, zones=False, listing_share=0.03)}


def stderr_of(fn):
    """(fn(), what the process wrote to file descriptor 2 meanwhile)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def one(name, seed, sizes, workloads):
    kw = WORKLOADS[name]
    cluster, apps, template = IU.image_sweep_case(seed, n_nodes=kw["n_nodes"], n_workloads=workloads, template_images=True,
                                                  zones=kw["zones"], max_replicas=120, listing_share=kw["listing_share"])
    counts = list(range(sizes))
    eng = sim.HipEngine()
    sim.sweep(cluster, apps, template, counts[:2], engine=eng)            # warm-up: library load, device init
    t0 = time.perf_counter()
    got, route = stderr_of(lambda: sim.sweep(cluster, apps, template, counts, engine=eng))
    t_batch = time.perf_counter() - t0
    st = eng.last_stats
    split = re.findall(r"image split: (\d+) node classes \(caller (\d+)\)", route)
    cn_t = re.findall(r"Cn_t (\d+)", route)
    t0 = time.perf_counter()
    ref, _ = stderr_of(lambda: sim._sweep_per_size(cluster, apps, template, counts, sim.HipEngine(), 100, 100, 100))
    t_per = time.perf_counter() - t0
    agree = all(getattr(got, f) == getattr(ref, f) for f in ("unscheduled", "cpu_pct", "mem_pct", "best"))
    prob = sim.sweep_batch(cluster, apps, template, counts, image_batch=True).flat.problem
    return {"workload": name, "nodes": len(cluster["Node"]),
            "listing_nodes": sum(1 for n in cluster["Node"] if (n.get("status") or {}).get("images")),
            "pods": prob.n_pods, "sizes": len(counts), "pod_classes": prob.n_pod_classes,
            "caller_node_classes": int(split[-1][1]) if split else None, "engine_node_classes_after_image_split": int(split[-1][0]) if split else None,
            "score_table_internal_classes": int(cn_t[-1]) if cn_t else None,
            "batched_sweep_s": round(t_batch, 3), "per_size_sweep_s": round(t_per, 3), "speedup": round(t_per / t_batch, 2),
            "batch_kernel_ms": round(st.kernel_ms, 3),
            "kernel": "all-feature" if st.kernel_variant == capi.KERNEL_WIDE else f"score table, generation {st.kernel_generation}",
            "best": got.best, "agree": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, default=64)
    ap.add_argument("--workloads", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    recs = [one(name, a.seed, a.sizes, a.workloads) for name in WORKLOADS]
    for r in recs:
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(recs, f, indent=1)
    return 0 if all(r["agree"] for r in recs) else 1


if __name__ == "__main__":
    sys.exit(main())

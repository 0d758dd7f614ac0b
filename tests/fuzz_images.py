#!/usr/bin/env python3
"""Randomised parity sweep of ImageLocality in batched sweeps (ABI v7): random clusters whose nodes list the pods' images (tagged and
untagged names, sizes on both sides of 23 MB and 1000 MB x containers), pods of one to three containers, templates that list an image or
not, Services, GPU share, several zones -- one batch over several cluster sizes on the library, every scenario compared row by row
(placement, unscheduled, used cpu / memory, GPU slices) with the C oracle on that size's one-size problem (tests/image_util.py).
Not collected by pytest; by hand on a GPU box:
    python tests/fuzz_images.py [n_cases] [first_seed]"""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401
import image_util as IU  # noqa: E402
import oracle_lib as O  # noqa: E402
from open_simulator_amd import capi, flatten as fl, simulate as sim, workloads as wl  # noqa: E402

MB = IU.MB
IMAGES = ["busybox", "busybox:latest", "nginx:1.25", "registry.local:5000/app/web:2", "registry.local:5000/app/web", "redis", "tiny:1"]


def _plain_case(rng):
    """cpu+memory pods over nodes of a few shapes, half of them listing images: the score-table kernel's ground"""
    shapes = [("4", "8Gi"), ("8", "16Gi"), ("16", "32Gi"), ("32", "64Gi")][: int(rng.integers(1, 5))]
    def imgs():
        out = []
        for nm in IMAGES:
            norm = nm if nm.rfind(":") > nm.rfind("/") else nm + ":latest"
            if rng.random() < 0.4 and norm not in [o["names"][0] for o in out]:
                size = int(rng.choice([1, 20, 23, 24, 200, 999, 1000, 1001, 1500, 3000])) * MB + int(rng.integers(0, 5))
                out.append({"names": [norm, nm.split(":")[0] + "@sha256:" + str(int(rng.integers(1 << 20)))], "sizeBytes": size})
        return out
    n_cluster = int(rng.integers(2, 40))
    nodes = []
    for j in range(n_cluster):
        cpu, mem = shapes[int(rng.integers(len(shapes)))]
        n = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": f"n{j}", "labels": {"kubernetes.io/hostname": f"n{j}"}},
             "status": {"allocatable": {"cpu": cpu, "memory": mem, "pods": str(int(rng.integers(5, 40)))}, "capacity": {"cpu": cpu, "memory": mem}}}
        if rng.random() < 0.5:
            n["status"]["images"] = imgs()
        nodes.append(n)
    tmpl = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": "tmpl", "labels": {}},
            "status": {"allocatable": {"cpu": "16", "memory": "32Gi", "pods": "30"}, "capacity": {"cpu": "16", "memory": "32Gi"}}}
    if rng.random() < 0.5:
        tmpl["status"]["images"] = imgs()
    clones = int(rng.integers(0, 10))
    pool = nodes + (wl.new_fake_nodes(tmpl, clones) if clones else [])
    pods = []
    for i in range(int(rng.integers(10, 250))):
        conts = [{"name": f"c{k}", "image": IMAGES[int(rng.integers(len(IMAGES)))] if rng.random() < 0.9 else "unlisted:9",
                  "resources": {"requests": {"cpu": f"{int(rng.integers(1, 40)) * 100}m", "memory": f"{int(rng.integers(1, 16)) * 256}Mi"}}}
                 for k in range(int(rng.integers(1, 4)))]
        pods.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": f"p{i}", "namespace": "default"}, "spec": {"containers": conts}})
    flat = fl.flatten(pool, pods, image_batch=True)
    sizes = sorted(set([n_cluster, len(pool)] + [int(x) for x in rng.integers(n_cluster, len(pool) + 1, 3)]))
    return flat.problem, np.array([[n, 0] for n in sizes], np.int32), np.arange(len(pods), dtype=np.int32)[None], None, "plain"


def _k8s_case(rng, seed):
    kind = int(rng.integers(4))
    cluster, apps, template = IU.image_sweep_case(seed, n_nodes=int(rng.integers(3, 14)), n_workloads=int(rng.integers(3, 12)),
                                                  template_images=rng.random() < 0.5, zones=kind == 2, gpu=kind == 3)
    counts = sorted(set(int(x) for x in rng.integers(0, 8, 4)))
    batch = sim.sweep_batch(cluster, apps, template, counts, image_batch=True)
    return batch.flat.problem, batch.scen, batch.orders, batch.node_ranks, ["services", "services", "zones", "gpu"][kind]


def one_case(case):
    rng = np.random.default_rng(77000 + case)
    prob, scen, orders, ranks, kind = _plain_case(rng) if case % 2 == 0 else _k8s_case(rng, 77000 + case)
    want_gpu = prob.gpu_mem is not None
    with capi.Context(0) as ctx:
        ctx.load_problem(prob)
        ctx.load_scenarios(scen, orders)
        if ranks is not None:
            ctx.set_node_ranks(ranks)
        ctx.run_loaded(True, want_gpu)
        res = ctx.fetch(True, want_gpu)
        st = ctx.stats()
    info = {"case": case, "kind": kind, "images": prob.image_locality is not None, "generation": int(st.kernel_generation),
            "variant": int(st.kernel_variant), "N": prob.n_nodes, "P": prob.n_pods, "S": len(scen)}
    for s, (n, o) in enumerate(scen):
        ref = O.run(IU.fold_images(prob, int(n)), [[int(n), int(o)]], orders, want_gpu_slices=want_gpu,
                    node_ranks=None if ranks is None else ranks[s:s + 1])
        same = res.placement[s].tolist() == ref.placement[0].tolist() and int(res.unscheduled[s]) == int(ref.unscheduled[0]) and \
            int(res.used_cpu[s]) == int(ref.used_cpu[0]) and int(res.used_mem[s]) == int(ref.used_mem[0]) and \
            (not want_gpu or res.gpu_slices[s].tolist() == ref.gpu_slices[0].tolist())
        if not same:
            return False, dict(info, scenario=s, n_nodes=int(n))
    return True, info


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad, kinds, kernels, with_images = 0, Counter(), Counter(), 0
    for case in range(first, first + n_cases):
        ok, info = one_case(case)
        kinds[info["kind"]] += 1
        kernels["all-feature" if info["variant"] == capi.KERNEL_WIDE else f"generation {info['generation']}"] += 1
        with_images += info["images"]
        if not ok:
            bad += 1
            print("MISMATCH", info, flush=True)
    print(f"fuzz_images: {n_cases} cases from {first} ({with_images} with image inputs), kinds {dict(kinds)}, kernels {dict(kernels)}, "
          f"mismatches {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

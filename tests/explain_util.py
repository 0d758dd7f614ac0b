"""Shared inputs of the batched-explain tests (test_explain_batch_host.py, test_gpu_explain_batch.py)."""
import copy

import numpy as np

import mix_util as MU


def example_gpushare_crowded():
    """example/ gpushare fits its own cluster; with six more copies of its two-GPU pod the devices run out at every size tried, so
    Open-Gpu-Share is the filter that fails (reason text `Node:<name>`)."""
    cluster, apps, types = MU.example_gpushare()
    apps = copy.deepcopy(apps)
    pods = apps[0].resource["Pod"]
    (src,) = [p for p in pods if p["metadata"]["name"] == "gpu-pod-02"]
    for i in range(6):
        clone = copy.deepcopy(src)
        clone["metadata"]["name"] = f"gpu-pod-02-{i}"
        pods.append(clone)
    return cluster, apps, types


# case -> (cluster, apps, new-node types), counts to sweep, a text its reasons must hold
CASES = {"simple": (MU.example_simple, [0, 1, 2, 4], "anti-affinity rules"), "gpushare": (example_gpushare_crowded, [0, 1, 2], " Node:"),
         "open_local": (MU.example_open_local, [0, 1, 3], "Insufficient Device storage, requested")}


def binned(row):
    """(sorted distinct codes, their counts) of one pod's code row: what simon_explain_batch's bins must hold."""
    codes, counts = np.unique(np.asarray(row, np.uint16), return_counts=True)
    return codes.tolist(), counts.tolist()

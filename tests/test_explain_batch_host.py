"""Batched explain, host side: the C-ABI entry (header, binding, built library), the histogram -> FitError text path of fiterror.py and
sweep(..., reasons=True) against simulate() of every size on the CPU oracle.  No GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import explain_util as XU
import mix_util as MU
from open_simulator_amd import capi, fiterror, simulate as sim, workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPE = """
#define SIMON_EXPLAIN_BINS 64
typedef struct simon_fail_bin { uint16_t code, pad; int32_t count; } simon_fail_bin;
int simon_explain_batch(simon_ctx* ctx, const int32_t* scenarios, int32_t n_scen,
                        int32_t max_failed, int32_t max_bins,
                        int32_t* n_failed,
                        int32_t* failed_pods,
                        int32_t* n_bins,
                        simon_fail_bin* bins,
                        uint16_t* fail_codes, int32_t code_stride);
"""


def _squash(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)).replace(" ,", ",").replace(" )", ")").strip()


def test_header_binding_and_library_carry_the_entry():
    header = _squash(open(os.path.join(ROOT, "include", "simon_hip.h")).read())
    for line in _squash(PROTOTYPE).split(";"):
        assert line.strip() in header, line
    assert re.search(r"#define SIMON_EXPLAIN_BINS 64\b", header)
    assert re.search(r"#define SIMON_HIP_ABI_VERSION 7\b", header)
    assert "simon_explain_batch" in capi.EXPORTS
    assert capi.ABI_VERSION == 7 and capi.EXPLAIN_BINS == 64 and capi.FAIL_BIN_DTYPE.itemsize == 8
    path = capi.library_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: build() first")
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "simon_explain_batch")
    assert lib.simon_hip_version() == 7


def _random_rows(n_rows=300):
    """Seeded code rows over everything a histogram can be turned into text for: static ids, every NodeResourcesFit bit subset (scalar
    names included), the anti / affinity / spread / ports codes, the reasonless Open-Local code and 0; n from 1 to 200."""
    rng = np.random.default_rng(20260)
    fit_bits = [capi.FIT_PODS, capi.FIT_CPU, capi.FIT_MEM, capi.FIT_EPH] + [capi.FIT_SCALAR0 << k for k in range(4)]
    fits = [capi.FAIL_FIT | sum(c) for r in range(1, len(fit_bits) + 1) for c in itertools.combinations(fit_bits, r)]
    assert len(fits) == 255
    statics = [capi.FAIL_STATIC | rid for rid in (1, 2, 3, 4, 7, 200)]
    others = [capi.FAIL_ANTI_INCOMING, capi.FAIL_ANTI_EXISTING, capi.FAIL_AFFINITY, capi.FAIL_SPREAD, capi.FAIL_SPREAD_LABEL, capi.FAIL_PORTS,
              capi.FAIL_LOCAL, 0]
    pool = np.array(fits + statics + others, np.uint16)
    rows, seen = [], set()
    for i in range(n_rows):
        n = int(rng.integers(1, 201)) if i >= 2 else (1, 200)[i]
        few = pool[rng.choice(len(pool), int(rng.integers(1, 12)), replace=False)]
        row = few[rng.integers(0, len(few), n)] if i % 3 else pool[rng.integers(0, len(pool), n)]
        if i < len(fits):
            row[int(rng.integers(n))] = fits[i]               # every fit subset occurs
        seen.update(row.tolist())
        rows.append(row)
    assert set(fits) <= seen and set(statics) <= seen and set(others) <= seen
    return rows


def test_fit_error_bins_equals_fit_error_on_random_rows():
    static = {4: fiterror.taint_reason("dedicated", "gpu"), 7: fiterror.taint_reason("zzz"), 200: "a host-defined reason"}
    scalars = ["nvidia.com/gpu", "example.com/foo", "hugepages-2Mi", "alibabacloud.com/gpu-mem"]
    rows = _random_rows()
    for row in rows:
        codes, counts = np.unique(row, return_counts=True)
        want = fiterror.fit_error(row, static_reasons=static, scalar_names=scalars)
        got = fiterror.fit_error_bins(len(row), list(zip(codes.tolist(), counts.tolist())), static, scalars)
        assert got == want
        assert got.startswith(f"0/{len(row)} nodes are available: ")
    # shuffled bins give the same text; the wrapper adds simulator.go's prefix
    row = rows[4]
    codes, counts = np.unique(row, return_counts=True)
    bins = list(zip(codes.tolist(), counts.tolist()))
    assert fiterror.fit_error_bins(len(row), bins[::-1], static, scalars) == fiterror.fit_error(row, static_reasons=static, scalar_names=scalars)
    assert fiterror.unscheduled_reason_bins("ns", "p", len(row), bins, static_reasons=static, scalar_names=scalars) == \
        fiterror.unscheduled_reason("ns", "p", row, static_reasons=static, scalar_names=scalars)


def test_fit_error_bins_refuses_node_specific_codes():
    assert fiterror.NODE_SPECIFIC_CODES == {capi.FAIL_GPUSHARE, capi.FAIL_LOCAL_LVM, capi.FAIL_LOCAL_DEV}
    for code in sorted(fiterror.NODE_SPECIFIC_CODES):
        with pytest.raises(ValueError):
            fiterror.fit_error_bins(3, [(capi.FAIL_FIT | capi.FIT_CPU, 2), (code, 1)])
    # fit_error itself still names the node
    assert fiterror.fit_error([capi.FAIL_GPUSHARE, capi.FAIL_FIT | capi.FIT_CPU], ["a", "b"]) == "0/2 nodes are available: 1 Insufficient cpu, 1 Node:a."


CASES = XU.CASES


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_reasons_equal_simulate_of_every_size(name):
    make, counts, text = CASES[name]
    cluster, apps, types = make()
    new_node = types[0]
    engine = MU.OracleEngine()
    got = sim.sweep(cluster, apps, new_node, counts, engine=engine, reasons=True)
    assert len(got.unscheduled_pods) == len(counts)
    assert any(got.unscheduled), "no size of the case leaves a pod unscheduled: nothing to explain"
    texts = " ".join(u["reason"] for lst in got.unscheduled_pods for u in lst)
    assert text in texts
    for s, k in enumerate(counts):
        want = sim.simulate(cluster, apps, engine, wl.new_fake_nodes(new_node, k) if k else ()).unscheduled_pods
        assert len(want) == got.unscheduled[s]
        assert got.unscheduled_pods[s] == want, (name, k)
        assert all(u["reason"].startswith("failed to schedule pod (") for u in want)
    plain = sim.sweep(cluster, apps, new_node, counts, engine=engine)
    assert plain.unscheduled_pods == [] and plain.unscheduled == got.unscheduled and plain.best == got.best


def test_a_size_whose_pod_stream_differs_is_listed_from_its_own_simulate(monkeypatch):
    """The simple example's app has a DaemonSet: one pod per node of the cluster it is expanded on, so the app's queue at a size need
    not be the pool's queue without the gated pods (simulate._same_stream).  Such a failing size is listed from simulate() of the size --
    pods and texts are simulate()'s by construction -- and every other failing size from the batch, never through simulate()."""
    make, counts, _ = CASES["simple"]
    cluster, apps, types = make()
    assert any(app.resource.get("DaemonSet") for app in apps)
    engine = MU.OracleEngine()
    same, replayed = {}, []
    real_same, real_simulate = sim._same_stream, sim.simulate
    monkeypatch.setattr(sim, "_same_stream", lambda c, a, b, o, s: same.setdefault(s, real_same(c, a, b, o, s)))
    monkeypatch.setattr(sim, "simulate", lambda c, a, e=None, new_nodes=(): (replayed.append(len(new_nodes)), real_simulate(c, a, e, new_nodes))[1])
    got = sim.sweep(cluster, apps, types[0], counts, engine=engine, reasons=True)
    failing = [s for s in range(len(counts)) if got.unscheduled[s] > 0]
    print("same stream per failing size:", same, "replayed counts:", replayed)
    assert sorted(same) == failing                                      # asked once per failing size, never for a size that fits
    assert replayed == [counts[s] for s in failing if not same[s]]
    assert not all(same.values()), "no size of the case has a stream of its own: the replay is not exercised"
    for s in failing:
        want = real_simulate(cluster, apps, engine, wl.new_fake_nodes(types[0], counts[s]) if counts[s] else ()).unscheduled_pods
        assert got.unscheduled_pods[s] == want
    # without the DaemonSet no stream is built and nothing is replayed
    for app in apps:
        app.resource.pop("DaemonSet", None)
    same.clear(); replayed.clear()
    got = sim.sweep(cluster, apps, types[0], counts, engine=engine, reasons=True)
    assert replayed == [] and all(same.values()) and any(got.unscheduled)
    for s, k in enumerate(counts):
        assert got.unscheduled_pods[s] == real_simulate(cluster, apps, engine, wl.new_fake_nodes(types[0], k) if k else ()).unscheduled_pods

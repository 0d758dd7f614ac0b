"""Shared pieces of the Open-Local usage / headroom tests (test_local_usage_host.py, test_local_usage.py): problems built by hand from
node and pod descriptions, the random cases of both files, the probes worth asking about, the refusal rules of
simon_fetch_local_usage / simon_fetch_headroom_local restated, and oracle-backed engines with and without supports_local_usage."""
import numpy as np

import gpu_usage_util as GU
import randprob
import usage_util as UU
from open_simulator_amd import capi, simulate as sim

GiB = 1 << 30
SSD, HDD = 1, 2
CASES = [(5, 30), (9, 50), (16, 70), (23, 90), (31, 100), (40, 120)]      # (N, P) of the random cases, host and device


def node(vgs=(), devs=(), annotated=True, cpu=64000, mem=256 * GiB, pods=110):
    """One pool node: vgs = [(interned name, capacity GiB, requested before the stream GiB)], devs = [(media, capacity GiB, allocated
    before the stream)]."""
    return dict(vgs=list(vgs), devs=list(devs), annotated=annotated, cpu=cpu, mem=mem, pods=pods)


def pod(lvm=(), ssd=(), hdd=(), cpu=100, mem=64 << 20, preset=-1):
    """One pod: lvm = [(size GiB, interned VG name or -1 = any)], ssd / hdd = sizes GiB.  Sizes may be 0."""
    return dict(lvm=list(lvm), ssd=sorted(ssd), hdd=sorted(hdd), cpu=cpu, mem=mem, preset=preset)


def problem(nodes, pods):
    """The capi.Problem of a hand-made pool and stream: one pod class per distinct description, one node class, no static
    scores -- so Open-Local's filter and Binpack score decide where storage pods go."""
    N, P = len(nodes), len(pods)
    vg_cnt, vg_cap, vg_req, vg_name = np.zeros(N, np.int32), np.ones((N, capi.MAX_VG), np.int64), np.zeros((N, capi.MAX_VG), np.int64), np.full((N, capi.MAX_VG), -7, np.int32)
    dev_cnt, dev_cap, media, alloc = np.zeros(N, np.int32), np.ones((N, capi.MAX_LDEV), np.int64), np.zeros(N, np.int32), np.zeros(N, np.int32)
    for j, n in enumerate(nodes):
        vg_cnt[j], dev_cnt[j] = len(n["vgs"]), len(n["devs"])
        for v, (name, cap, req) in enumerate(n["vgs"]):
            vg_name[j, v], vg_cap[j, v], vg_req[j, v] = name, cap * GiB, req * GiB
        for d, (m, cap, taken) in enumerate(n["devs"]):
            dev_cap[j, d] = cap * GiB
            media[j] |= m << (2 * d)
            alloc[j] |= int(bool(taken)) << d
    shapes, cls = {}, np.zeros(P, np.int32)                                  # one class per distinct pod description
    for p, q in enumerate(pods):
        key = (tuple(q["lvm"]), tuple(q["ssd"]), tuple(q["hdd"]), q["cpu"], q["mem"])
        cls[p] = shapes.setdefault(key, len(shapes))
    Cp = len(shapes)
    specs = np.zeros(Cp, capi.LOCAL_SPEC_DTYPE)
    spec_of = np.full(Cp, -1, np.int32)
    for (lvm, ssd, hdd, _, _), c in shapes.items():
        if not (lvm or ssd or hdd):
            continue
        lvm = sorted(lvm, key=lambda x: x[1] < 0)                            # volumes that name a VG first, pod order kept
        sp = specs[c]
        sp["n_lvm"], sp["n_ssd"], sp["n_hdd"] = len(lvm), len(ssd), len(hdd)
        sp["lvm_vg"][:] = -1
        for k, (size, vg) in enumerate(lvm):
            sp["lvm_size"][k], sp["lvm_vg"][k] = int(size * GiB), vg
        sp["ssd_size"][:len(ssd)] = [int(x * GiB) for x in ssd]
        sp["hdd_size"][:len(hdd)] = [int(x * GiB) for x in hdd]
        spec_of[c] = c
    preset = np.array([q["preset"] for q in pods], np.int32)
    return capi.Problem(alloc_cpu=np.array([n["cpu"] for n in nodes], np.int64), alloc_mem=np.array([n["mem"] for n in nodes], np.int64),
                        alloc_pods=np.array([n["pods"] for n in nodes], np.int32), node_class=np.zeros(N, np.int32),
                        req_cpu=np.array([q["cpu"] for q in pods], np.int64), req_mem=np.array([q["mem"] for q in pods], np.int64),
                        pod_class=cls, n_pod_classes=Cp, n_node_classes=1,
                        simon_raw=np.zeros((Cp, 1), np.int64), const_score=np.full(Cp, 1000300, np.int64),
                        preset_node=preset if (preset >= 0).any() else None, gate_node=preset if (preset >= 0).any() else None,
                        local_flags=np.array([int(n["annotated"]) for n in nodes], np.int32), local_vg_cnt=vg_cnt, local_vg_cap=vg_cap,
                        init_vg_req=vg_req, local_vg_name=vg_name, local_dev_cnt=dev_cnt, local_dev_cap=dev_cap, local_dev_media=media,
                        init_dev_alloc=alloc, local_specs=specs, local_spec_of=spec_of).normalise()


def random_case(N, P):
    """(problem, scen [2][2], orders [2][P]) of one random case: Open-Local nodes and specs, a static mask, state before the stream,
    gated pods; the whole pool and a prefix of it, identity and a permuted order."""
    prob = randprob.rand_problem(1000 + N, N=N, P=P, local=True, static_mask=True, init_state=True, gates=True)
    orders = np.stack([np.arange(P), np.random.default_rng(N).permutation(P)]).astype(np.int32)
    scen = np.array([[N, 1], [max(1, (2 * N) // 3), 0]], np.int32)
    return prob, scen, orders


def spec_of_pod(prob, p):
    return sim._local_spec(prob, int(prob.pod_class[p]) if prob.pod_class is not None else 0)


def probe_exact_local(prob, p):
    """simon_fetch_headroom_local's exact: simon_fetch_headroom_gpu's conditions, an Open-Local spec no longer disqualifying."""
    cls = int(prob.pod_class[p]) if prob.pod_class is not None else 0
    at = lambda v, d=0: d if v is None else int(np.asarray(v)[p])                                         # noqa: E731
    if at(prob.pin_node, -1) >= 0 or at(prob.preset_node, -1) >= 0:
        return False
    if not GU.probe_bound(prob, p) and (at(prob.gpu_mem) or at(prob.pod_gpu_cnt) or at(prob.gpu_index)):
        return False
    if prob.term_topo_key is not None and len(prob.term_topo_key):
        for off in (prob.match_off, prob.anti_off, prob.port_off, prob.aff_off, prob.spread_hard_off):
            if off is not None and off[cls + 1] != off[cls]:
                return False
    return True


def storage_probes(prob, n=8):
    """Distinct exact probes whose class has volumes, one per spec and request shape, at most n."""
    seen, out = set(), []
    for p in range(prob.n_pods):
        sp = spec_of_pod(prob, p)
        if sp is None or not probe_exact_local(prob, p):
            continue
        key = (int(prob.local_spec_of[prob.pod_class[p]]), int(prob.req_cpu[p]), int(prob.req_mem[p]), int(prob.pod_class[p]))
        if key not in seen:
            seen.add(key)
            out.append(p)
    return out[:n]


def kinds_of(prob, p):
    """Which kinds of volume probe p carries: a subset of {"named", "any", "device"}."""
    sp = spec_of_pod(prob, p)
    k = set()
    for i in range(int(sp["n_lvm"])):
        k.add("named" if int(sp["lvm_vg"][i]) >= 0 else "any")
    if int(sp["n_ssd"]) + int(sp["n_hdd"]) > 0:
        k.add("device")
    return k


def local_usage_errors(S, scen_ids, n, have_vg_req=True, struct_ok=True, have_placement=True, reloaded=False):
    """simon_fetch_local_usage's refusals, restated: those of simon_fetch_node_usage with vg_req the one required array."""
    return UU.usage_errors(S, scen_ids, n, have=("req_cpu", "req_mem", "npods") if have_vg_req else (), struct_ok=struct_ok,
                           have_placement=have_placement, reloaded=reloaded)


def headroom_local_errors(P, probes, K, have_fit=True, have_placement=True, reloaded=False, gpu=False, have_slices=True):
    """simon_fetch_headroom_local's refusals, restated: those of simon_fetch_headroom_gpu."""
    return GU.headroom_gpu_errors(P, probes, K, have_fit, have_placement, reloaded, gpu, have_slices)


class GpuUsageOnlyEngine(GU.GpuUsageOracleEngine):
    """Oracle-backed engine without supports_local_usage: with storage=True the sweeps compute everything on the host and warn."""


class LocalUsageOracleEngine(GU.GpuUsageOracleEngine):
    """Oracle-backed engine that answers local_usage_of / headroom_storage as HipEngine does, from the host restatement."""
    supports_local_usage = True

    def run(self, prob, scen, orders, want_placement=True, node_ranks=None, want_gpu_slices=False, present=None, pod_present=None,
            pod_groups=None, headroom_pods=None, usage_of=None, gpu_usage_of=None, headroom_devices=False, local_usage_of=None,
            headroom_storage=False):
        record = want_gpu_slices or (headroom_storage and headroom_pods is not None and prob.gpu_mem is not None)
        res = super().run(prob, scen, orders, True, node_ranks, record, present, pod_present, pod_groups,
                          None if headroom_storage else headroom_pods, usage_of, gpu_usage_of, headroom_devices)
        held = UU.held_rows(prob, capi.scenarios_array(scen), None if present is None else present[0])
        if headroom_pods is not None and headroom_storage:
            res.headroom, _, res.headroom_exact = sim.host_headroom(prob, res.placement, held, headroom_pods, res.gpu_slices, storage=True,
                                                                    orders=orders, scen=scen)
        if local_usage_of is not None:
            res.local_usage = sim.host_local_usage(prob, res.placement, held, orders, scen, local_usage_of)
        if not want_gpu_slices:
            res.gpu_slices = None
        return res


"""ctypes binding of include/simon_hip.h (the C-ABI of libsimon_hip.so).

This is the Python twin of the cgo stub shown in INTEGRATION.md: plain pointers and sizes, no torch
types.  The struct layouts below mirror include/simon_hip.h field for field; `Problem` is a
numpy-side container that keeps the arrays alive while the C structs point into them.

The product path fails loudly when the HIP library is missing: `load_library()` raises, there is no
CPU fallback (the oracle under oracle/ is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

ABI_VERSION = 7
MAX_GPU_DEV = 8
MAX_SCALAR = 4

UNSCHEDULED = -1
GATED = -2
ESTATE = -1      # SIMON_ESTATE (SimonError.code)
EINVAL = -22     # SIMON_EINVAL
MAX_SEGMENTS = 8 # SIMON_MAX_SEGMENTS
MAX_ZONES = 64 # SIMON_MAX_ZONES
MAX_POD_GROUPS = 1024 # SIMON_MAX_POD_GROUPS
MAX_PROBES = 64 # SIMON_MAX_PROBES

FAIL_STATIC = 0x8000
REASON_NODE_AFFINITY = 3
FAIL_FIT = 0x4000
FIT_PODS, FIT_CPU, FIT_MEM, FIT_EPH, FIT_SCALAR0 = 0x1, 0x2, 0x4, 0x8, 0x10
FAIL_ANTI_INCOMING = 0x2001
FAIL_ANTI_EXISTING = 0x2002
FAIL_AFFINITY = 0x2003
FAIL_SPREAD = 0x2010
FAIL_SPREAD_LABEL = 0x2011
FAIL_GPUSHARE = 0x1000
FAIL_PORTS = 0x0800
CLASS_AFF_SELF = 0x1
MAX_SPREAD = 4
MAX_VG, MAX_LDEV, MAX_LVOL = 4, 8, 4
FAIL_LOCAL, FAIL_LOCAL_LVM, FAIL_LOCAL_DEV = 0x0400, 0x0401, 0x0402
LOCAL_ERR_NONE, LOCAL_ERR_NO_SUCH_VG, LOCAL_ERR_NO_VG, LOCAL_ERR_LVM, LOCAL_ERR_DEVICE = 0, 1, 2, 3, 4   # simon_explain_local_detail
SPREAD_DUP_KEY = 0x40000000

KERNEL_NARROW = 1
KERNEL_WIDE = 2
KERNEL_NARROW_FAST = 3
KERNEL_NARROW_CACHE = 4

_p64 = C.POINTER(C.c_int64)
_p32 = C.POINTER(C.c_int32)
_pu64 = C.POINTER(C.c_uint64)
_pu8 = C.POINTER(C.c_uint8)
_pu16 = C.POINTER(C.c_uint16)
_pf64 = C.POINTER(C.c_double)


class NodesSoA(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_nodes", C.c_int32),
        ("alloc_cpu", _p64), ("alloc_mem", _p64), ("alloc_eph", _p64), ("alloc_pods", _p32),
        ("init_req_cpu", _p64), ("init_req_mem", _p64), ("init_req_eph", _p64),
        ("init_nz_cpu", _p64), ("init_nz_mem", _p64), ("init_npods", _p32),
        ("node_class", _p32),
        ("n_scalar", C.c_int32), ("scalar_alloc", _p64), ("init_scalar_req", _p64),
        ("gpu_cnt", _p32), ("gpu_mem_total", _p64), ("init_gpu_used", _p64),
        ("local_flags", _p32), ("local_vg_cnt", _p32), ("local_vg_cap", _p64), ("init_vg_req", _p64), ("local_vg_name", _p32),
        ("local_dev_cnt", _p32), ("local_dev_cap", _p64), ("local_dev_media", _p32), ("init_dev_alloc", _p32),
        ("n_topo_keys", C.c_int32), ("topo_dom", _p32), ("topo_n_dom", _p32),
    ]


class PodsSoA(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_pods", C.c_int32),
        ("req_cpu", _p64), ("req_mem", _p64), ("req_eph", _p64), ("nz_cpu", _p64), ("nz_mem", _p64),
        ("scalar_req", _p64), ("pod_class", _p32), ("preset_node", _p32), ("gate_node", _p32),
        ("gpu_mem", _p64), ("gpu_cnt", _p32), ("pin_node", _p32), ("gpu_index", C.POINTER(C.c_uint32)),
    ]


class LocalSpec(C.Structure):
    _fields_ = [("n_lvm", C.c_int32), ("n_ssd", C.c_int32), ("n_hdd", C.c_int32), ("pad", C.c_int32),
                ("lvm_size", C.c_int64 * MAX_LVOL), ("lvm_vg", C.c_int32 * MAX_LVOL),
                ("ssd_size", C.c_int64 * MAX_LVOL), ("hdd_size", C.c_int64 * MAX_LVOL)]


LOCAL_SPEC_DTYPE = np.dtype([("n_lvm", "<i4"), ("n_ssd", "<i4"), ("n_hdd", "<i4"), ("pad", "<i4"), ("lvm_size", "<i8", (MAX_LVOL,)),
                             ("lvm_vg", "<i4", (MAX_LVOL,)), ("ssd_size", "<i8", (MAX_LVOL,)), ("hdd_size", "<i8", (MAX_LVOL,))])
assert LOCAL_SPEC_DTYPE.itemsize == C.sizeof(LocalSpec)


class ClassTables(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_pod_classes", C.c_int32), ("n_node_classes", C.c_int32),
        ("static_mask", _pu64), ("static_reason", _pu8), ("simon_raw", _p64), ("const_score", _p64),
        ("node_affinity_raw", _p64), ("taint_prefer_raw", _p64), ("static_add", _p64),
        ("n_terms", C.c_int32), ("term_topo_key", _p32), ("term_node_set", _p32),
        ("n_node_sets", C.c_int32), ("node_sets", _pu64),
        ("match_off", _p32), ("match_idx", _p32), ("anti_off", _p32), ("anti_idx", _p32),
        ("port_off", _p32), ("port_idx", _p32),
        ("aff_off", _p32), ("aff_idx", _p32), ("class_flags", _pu8),
        ("pref_off", _p32), ("pref_idx", _p32), ("pref_w", _p32),
        ("own_off", _p32), ("own_idx", _p32), ("own_w", _p32),
        ("spread_hard_off", _p32), ("spread_hard_idx", _p32), ("spread_hard_skew", _p32),
        ("spread_hard_self", _p32), ("spread_hard_set", _p32),
        ("spread_soft_off", _p32), ("spread_soft_idx", _p32), ("spread_soft_skew", _p32),
        ("local_spec_of", _p32), ("n_local_specs", C.c_int32), ("local_specs", C.POINTER(LocalSpec)),
        ("topo_is_hostname", _pu8), ("spread_log", _pf64),
    ]


class ImageLocalityC(C.Structure):
    _fields_ = [
        ("n_images", C.c_int32), ("size", _p64), ("node_off", _p32), ("node_image", _p32), ("node_count", _p32),
        ("class_off", _p32), ("class_image", _p32),
    ]


@dataclass
class ImageLocality:
    """ABI v7 (simon_image_locality): the inputs of ImageLocality.Score for a batch of cluster sizes.  Image ids are the caller's own.
    size[i] = ImageStateSummary.Size (the first lister's sizeBytes); per pool node a CSR of (image id, NumNodes as the arrival order leaves
    it); per pod class one image id per container (-1: no node lists it; it still counts in numContainers)."""
    size: np.ndarray          # [I] int64
    node_off: np.ndarray      # [N+1] int32
    node_image: np.ndarray    # [nnz] int32
    node_count: np.ndarray    # [nnz] int32
    class_off: np.ndarray     # [Cp+1] int32
    class_image: np.ndarray   # [class_off[-1]] int32
    # [nnz] int64: the sizeBytes node j's own entry lists (simon_set_image_node_sizes).  With it segmented and node-subset batches take the
    # problem and score every scenario by its own image states; node_count / size must then be the pool-order reading.
    node_size: Optional[np.ndarray] = None

    def normalise(self):
        self.size = np.ascontiguousarray(self.size, dtype=np.int64).reshape(-1)
        if self.node_size is not None:
            self.node_size = np.ascontiguousarray(self.node_size, dtype=np.int64).reshape(-1)
        for name in ("node_off", "node_image", "node_count", "class_off", "class_image"):
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=np.int32).reshape(-1))
        return self

    def c_struct(self) -> "ImageLocalityC":
        self.normalise()
        return ImageLocalityC(len(self.size), _ptr(self.size, C.c_int64), _ptr(self.node_off, C.c_int32), _ptr(self.node_image, C.c_int32),
                              _ptr(self.node_count, C.c_int32), _ptr(self.class_off, C.c_int32), _ptr(self.class_image, C.c_int32))

    def score(self, c: int, j: int, n: int) -> int:
        """The engine's formula (include/simon_hip.h, simon_image_locality) for pod class c on pool node j in a cluster of n nodes."""
        e0, e1 = int(self.class_off[c]), int(self.class_off[c + 1])
        if e1 == e0 or n <= 0:
            return 0
        mine = {int(self.node_image[q]): int(self.node_count[q]) for q in range(int(self.node_off[j]), int(self.node_off[j + 1]))}
        total = 0
        for e in range(e0, e1):
            i = int(self.class_image[e])
            if i >= 0 and i in mine:
                total += int(float(int(self.size[i])) * (float(mine[i]) / float(n)))
        mb = 1024 * 1024
        hi = 1000 * mb * (e1 - e0)
        total = min(max(total, 23 * mb), hi)
        return 100 * (total - 23 * mb) // (hi - 23 * mb)


class Scenario(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("order_id", C.c_int32)]


class BatchOut(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("unscheduled", _p32), ("used_cpu", _p64), ("used_mem", _p64), ("placement", _p32), ("used_vg", _p64),
        ("gpu_slices", _pu64),
    ]


class Plan(C.Structure):
    _fields_ = [
        ("found", C.c_int32), ("scenario", C.c_int32), ("n_nodes", C.c_int32), ("order_id", C.c_int32),
        ("cpu_pct", C.c_int32), ("mem_pct", C.c_int32), ("used_cpu", C.c_int64), ("used_mem", C.c_int64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [
        ("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
        ("n_launches", C.c_int32), ("kernel_variant", C.c_int32), ("workgroup_size", C.c_int32),
        ("slots_per_lane", C.c_int32), ("lds_bytes", C.c_int64), ("kernel_generation", C.c_int32), ("reserved", C.c_int32),
    ]


def _arr(a, dtype, shape=None) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _ptr(a: Optional[np.ndarray], ctype):
    if a is None:
        return C.cast(None, C.POINTER(ctype))
    return a.ctypes.data_as(C.POINTER(ctype))


@dataclass
class Problem:
    """Numpy-side mirror of (simon_nodes_soa, simon_pods_soa, simon_class_tables).

    Field meaning is documented in include/simon_hip.h; None = optional array omitted.
    """
    # nodes
    alloc_cpu: np.ndarray = None
    alloc_mem: np.ndarray = None
    alloc_pods: np.ndarray = None
    alloc_eph: Optional[np.ndarray] = None
    init_req_cpu: Optional[np.ndarray] = None
    init_req_mem: Optional[np.ndarray] = None
    init_req_eph: Optional[np.ndarray] = None
    init_nz_cpu: Optional[np.ndarray] = None
    init_nz_mem: Optional[np.ndarray] = None
    init_npods: Optional[np.ndarray] = None
    node_class: Optional[np.ndarray] = None
    scalar_alloc: Optional[np.ndarray] = None      # [K][N]
    init_scalar_req: Optional[np.ndarray] = None   # [K][N]
    gpu_cnt: Optional[np.ndarray] = None
    gpu_mem_total: Optional[np.ndarray] = None
    init_gpu_used: Optional[np.ndarray] = None     # [N][8]
    local_flags: Optional[np.ndarray] = None       # [N]
    local_vg_cnt: Optional[np.ndarray] = None
    local_vg_cap: Optional[np.ndarray] = None      # [N][4]
    init_vg_req: Optional[np.ndarray] = None
    local_vg_name: Optional[np.ndarray] = None     # [N][4]
    local_dev_cnt: Optional[np.ndarray] = None
    local_dev_cap: Optional[np.ndarray] = None     # [N][8]
    local_dev_media: Optional[np.ndarray] = None
    init_dev_alloc: Optional[np.ndarray] = None
    topo_dom: Optional[np.ndarray] = None          # [Kt][N]
    topo_n_dom: Optional[np.ndarray] = None        # [Kt]
    # pods
    req_cpu: np.ndarray = None
    req_mem: np.ndarray = None
    req_eph: Optional[np.ndarray] = None
    nz_cpu: Optional[np.ndarray] = None
    nz_mem: Optional[np.ndarray] = None
    scalar_req: Optional[np.ndarray] = None        # [K][P]
    pod_class: Optional[np.ndarray] = None
    preset_node: Optional[np.ndarray] = None
    gate_node: Optional[np.ndarray] = None
    pin_node: Optional[np.ndarray] = None          # [P] >= 0: the only node the pod's node affinity admits (DaemonSet pods)
    gpu_mem: Optional[np.ndarray] = None
    pod_gpu_cnt: Optional[np.ndarray] = None
    gpu_index: Optional[np.ndarray] = None         # [P] uint32: gpu-index annotation the pod arrives with, packed (pack_gpu_index)
    scalar_entries: Optional[np.ndarray] = None    # [P] uint8, ABI v6: bit k = the request holds an ENTRY for extended resource k (bit 7: one no node tracks), a zero quantity included
    priority: Optional[np.ndarray] = None          # [P] int32, ABI v6: spec.priority (None: all equal)
    init_min_priority: int = 0x7fffffff            # lowest priority among the pods bound before the stream (behind init_*)
    image_locality: Optional[ImageLocality] = None  # ABI v7: ImageLocality per cluster size, on the device (static_add then leaves it out)
    # class tables
    n_pod_classes: int = 1
    n_node_classes: int = 1
    static_mask: Optional[np.ndarray] = None       # [Cp][ceil(N/64)] uint64
    static_reason: Optional[np.ndarray] = None     # [Cp][N] uint8
    simon_raw: Optional[np.ndarray] = None         # [Cp][Cn]
    const_score: Optional[np.ndarray] = None       # [Cp]
    node_affinity_raw: Optional[np.ndarray] = None  # [Cp][Cn]
    taint_prefer_raw: Optional[np.ndarray] = None   # [Cp][Cn]
    static_add: Optional[np.ndarray] = None         # [Cp][Cn]
    term_topo_key: Optional[np.ndarray] = None     # [T]
    term_node_set: Optional[np.ndarray] = None     # [T]
    node_sets: Optional[np.ndarray] = None         # [R][ceil(N/64)] uint64
    anti_off: Optional[np.ndarray] = None
    anti_idx: Optional[np.ndarray] = None
    match_off: Optional[np.ndarray] = None
    match_idx: Optional[np.ndarray] = None
    port_off: Optional[np.ndarray] = None
    port_idx: Optional[np.ndarray] = None
    aff_off: Optional[np.ndarray] = None
    aff_idx: Optional[np.ndarray] = None
    class_flags: Optional[np.ndarray] = None       # [Cp] uint8
    pref_off: Optional[np.ndarray] = None
    pref_idx: Optional[np.ndarray] = None
    pref_w: Optional[np.ndarray] = None
    own_off: Optional[np.ndarray] = None
    own_idx: Optional[np.ndarray] = None
    own_w: Optional[np.ndarray] = None
    spread_hard_off: Optional[np.ndarray] = None
    spread_hard_idx: Optional[np.ndarray] = None
    spread_hard_skew: Optional[np.ndarray] = None
    spread_hard_self: Optional[np.ndarray] = None
    spread_hard_set: Optional[np.ndarray] = None
    spread_soft_off: Optional[np.ndarray] = None
    spread_soft_idx: Optional[np.ndarray] = None
    spread_soft_skew: Optional[np.ndarray] = None
    local_spec_of: Optional[np.ndarray] = None     # [Cp]
    local_specs: Optional[np.ndarray] = None       # structured array LOCAL_SPEC_DTYPE
    topo_is_hostname: Optional[np.ndarray] = None  # [Kt] uint8
    spread_log: Optional[np.ndarray] = None        # [N+1] float64
    _keep: list = field(default_factory=list, repr=False)

    @property
    def n_nodes(self) -> int:
        return int(len(self.alloc_cpu))

    @property
    def n_pods(self) -> int:
        return int(len(self.req_cpu))

    def normalise(self) -> "Problem":
        N, P = self.n_nodes, self.n_pods
        i64, i32 = np.int64, np.int32
        self.alloc_cpu = _arr(self.alloc_cpu, i64, (N,))
        self.alloc_mem = _arr(self.alloc_mem, i64, (N,))
        self.alloc_pods = _arr(self.alloc_pods, i32, (N,))
        for name in ("alloc_eph", "init_req_cpu", "init_req_mem", "init_req_eph", "init_nz_cpu", "init_nz_mem",
                     "gpu_mem_total"):
            setattr(self, name, _arr(getattr(self, name), i64, (N,)))
        for name in ("init_npods", "node_class", "gpu_cnt"):
            setattr(self, name, _arr(getattr(self, name), i32, (N,)))
        K = 0
        if self.scalar_alloc is not None:
            self.scalar_alloc = _arr(self.scalar_alloc, i64)
            K = self.scalar_alloc.shape[0]
            assert self.scalar_alloc.shape == (K, N) and K <= MAX_SCALAR
        self.init_scalar_req = _arr(self.init_scalar_req, i64, (K, N)) if self.init_scalar_req is not None else None
        self.init_gpu_used = _arr(self.init_gpu_used, i64, (N, MAX_GPU_DEV)) if self.init_gpu_used is not None else None
        if self.local_flags is not None:
            self.local_flags = _arr(self.local_flags, i32, (N,))
            self.local_vg_cnt = _arr(self.local_vg_cnt if self.local_vg_cnt is not None else np.zeros(N), i32, (N,))
            self.local_vg_cap = _arr(self.local_vg_cap if self.local_vg_cap is not None else np.zeros((N, MAX_VG)), i64, (N, MAX_VG))
            self.init_vg_req = _arr(self.init_vg_req, i64, (N, MAX_VG)) if self.init_vg_req is not None else None
            self.local_vg_name = _arr(self.local_vg_name if self.local_vg_name is not None else np.zeros((N, MAX_VG)), i32, (N, MAX_VG))
            self.local_dev_cnt = _arr(self.local_dev_cnt if self.local_dev_cnt is not None else np.zeros(N), i32, (N,))
            self.local_dev_cap = _arr(self.local_dev_cap if self.local_dev_cap is not None else np.zeros((N, MAX_LDEV)), i64, (N, MAX_LDEV))
            self.local_dev_media = _arr(self.local_dev_media if self.local_dev_media is not None else np.zeros(N), i32, (N,))
            self.init_dev_alloc = _arr(self.init_dev_alloc, i32, (N,)) if self.init_dev_alloc is not None else None
        Kt = 0
        if self.topo_dom is not None:
            self.topo_dom = _arr(self.topo_dom, i32)
            Kt = self.topo_dom.shape[0]
            assert self.topo_dom.shape == (Kt, N)
            self.topo_n_dom = _arr(self.topo_n_dom, i32, (Kt,))
        self.req_cpu = _arr(self.req_cpu, i64, (P,))
        self.req_mem = _arr(self.req_mem, i64, (P,))
        for name in ("req_eph", "nz_cpu", "nz_mem", "gpu_mem"):
            setattr(self, name, _arr(getattr(self, name), i64, (P,)))
        for name in ("pod_class", "preset_node", "gate_node", "pod_gpu_cnt", "pin_node"):
            setattr(self, name, _arr(getattr(self, name), i32, (P,)))
        self.gpu_index = _arr(self.gpu_index, np.uint32, (P,))
        self.scalar_entries = _arr(self.scalar_entries, np.uint8, (P,))
        self.priority = _arr(self.priority, i32, (P,))
        self.scalar_req = _arr(self.scalar_req, i64, (K, P)) if self.scalar_req is not None else None
        Cp, Cn = self.n_pod_classes, self.n_node_classes
        words = (N + 63) // 64
        self.static_mask = _arr(self.static_mask, np.uint64, (Cp, words)) if self.static_mask is not None else None
        self.static_reason = _arr(self.static_reason, np.uint8, (Cp, N)) if self.static_reason is not None else None
        if self.simon_raw is None:
            self.simon_raw = np.zeros((Cp, Cn), dtype=i64)
        self.simon_raw = _arr(self.simon_raw, i64, (Cp, Cn))
        self.const_score = _arr(self.const_score, i64, (Cp,)) if self.const_score is not None else None
        for name in ("node_affinity_raw", "taint_prefer_raw", "static_add"):
            v = getattr(self, name)
            setattr(self, name, _arr(v, i64, (Cp, Cn)) if v is not None else None)
        if self.local_spec_of is not None:
            self.local_spec_of = _arr(self.local_spec_of, i32, (Cp,))
            self.local_specs = np.ascontiguousarray(self.local_specs, dtype=LOCAL_SPEC_DTYPE)
        if self.term_topo_key is not None:
            self.term_topo_key = _arr(self.term_topo_key, i32)
            T = len(self.term_topo_key)
            if self.term_node_set is not None:
                self.term_node_set = _arr(self.term_node_set, i32, (T,))
            if self.node_sets is not None:
                self.node_sets = _arr(self.node_sets, np.uint64)
                assert self.node_sets.ndim == 2 and self.node_sets.shape[1] == words
            zero_off = np.zeros(Cp + 1, i32)
            for off, cols in (("match_off", ("match_idx",)), ("anti_off", ("anti_idx",)), ("port_off", ("port_idx",)), ("aff_off", ("aff_idx",)),
                              ("pref_off", ("pref_idx", "pref_w")), ("own_off", ("own_idx", "own_w")),
                              ("spread_hard_off", ("spread_hard_idx", "spread_hard_skew", "spread_hard_self",
                                                   "spread_hard_set")),
                              ("spread_soft_off", ("spread_soft_idx", "spread_soft_skew"))):
                o = getattr(self, off)
                if o is None:
                    if off in ("match_off", "anti_off"):       # always materialised (ABI v1 compatibility of callers)
                        setattr(self, off, zero_off.copy())
                        for cname in cols:
                            setattr(self, cname, np.zeros(1, i32))
                    continue
                o = _arr(o, i32, (Cp + 1,))
                setattr(self, off, o)
                for cname in cols:
                    v = getattr(self, cname)
                    if v is None and cname == "spread_hard_set":
                        continue
                    v = _arr(v if v is not None and len(v) else np.zeros(1, i32), i32)
                    assert len(v) >= max(1, int(o[-1])), (cname, len(v), int(o[-1]))
                    setattr(self, cname, v)
            if self.class_flags is not None:
                self.class_flags = _arr(self.class_flags, np.uint8, (Cp,))
            if self.topo_is_hostname is not None:
                self.topo_is_hostname = _arr(self.topo_is_hostname, np.uint8, (Kt,))
            if self.spread_log is not None:
                self.spread_log = _arr(self.spread_log, np.float64, (N + 1,))
        return self

    # --- C views ---------------------------------------------------------------------------
    def c_nodes(self) -> NodesSoA:
        self.normalise()
        s = NodesSoA()
        s.struct_size = C.sizeof(NodesSoA)
        s.n_nodes = self.n_nodes
        for name in ("alloc_cpu", "alloc_mem", "alloc_eph", "init_req_cpu", "init_req_mem", "init_req_eph",
                     "init_nz_cpu", "init_nz_mem", "scalar_alloc", "init_scalar_req", "gpu_mem_total",
                     "init_gpu_used"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int64))
        for name in ("alloc_pods", "init_npods", "node_class", "gpu_cnt", "topo_dom", "topo_n_dom", "local_flags", "local_vg_cnt",
                     "local_vg_name", "local_dev_cnt", "local_dev_media", "init_dev_alloc"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int32))
        for name in ("local_vg_cap", "init_vg_req", "local_dev_cap"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int64))
        s.n_scalar = 0 if self.scalar_alloc is None else self.scalar_alloc.shape[0]
        s.n_topo_keys = 0 if self.topo_dom is None else self.topo_dom.shape[0]
        return s

    def c_pods(self) -> PodsSoA:
        self.normalise()
        s = PodsSoA()
        s.struct_size = C.sizeof(PodsSoA)
        s.n_pods = self.n_pods
        for name in ("req_cpu", "req_mem", "req_eph", "nz_cpu", "nz_mem", "scalar_req", "gpu_mem"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int64))
        for name in ("pod_class", "preset_node", "gate_node", "pin_node"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int32))
        s.gpu_cnt = _ptr(self.pod_gpu_cnt, C.c_int32)
        s.gpu_index = _ptr(self.gpu_index, C.c_uint32)
        return s

    def c_tables(self) -> ClassTables:
        self.normalise()
        s = ClassTables()
        s.struct_size = C.sizeof(ClassTables)
        s.n_pod_classes = self.n_pod_classes
        s.n_node_classes = self.n_node_classes
        s.static_mask = _ptr(self.static_mask, C.c_uint64)
        s.static_reason = _ptr(self.static_reason, C.c_uint8)
        s.simon_raw = _ptr(self.simon_raw, C.c_int64)
        s.const_score = _ptr(self.const_score, C.c_int64)
        for name in ("node_affinity_raw", "taint_prefer_raw", "static_add"):
            setattr(s, name, _ptr(getattr(self, name), C.c_int64))
        s.n_terms = 0 if self.term_topo_key is None else len(self.term_topo_key)
        s.n_node_sets = 0 if self.node_sets is None else int(self.node_sets.shape[0])
        s.node_sets = _ptr(self.node_sets, C.c_uint64)
        for name in ("term_topo_key", "term_node_set", "match_off", "match_idx", "anti_off", "anti_idx", "port_off", "port_idx", "aff_off",
                     "aff_idx", "pref_off", "pref_idx", "pref_w", "own_off", "own_idx", "own_w", "spread_hard_off",
                     "spread_hard_idx", "spread_hard_skew", "spread_hard_self", "spread_hard_set", "spread_soft_off",
                     "spread_soft_idx", "spread_soft_skew"):
            setattr(s, name, _ptr(getattr(self, name) if s.n_terms else None, C.c_int32))
        s.local_spec_of = _ptr(self.local_spec_of, C.c_int32)
        s.n_local_specs = 0 if self.local_specs is None else len(self.local_specs)
        s.local_specs = C.cast(None, C.POINTER(LocalSpec)) if self.local_specs is None else \
            self.local_specs.ctypes.data_as(C.POINTER(LocalSpec))
        s.class_flags = _ptr(self.class_flags, C.c_uint8)
        s.topo_is_hostname = _ptr(self.topo_is_hostname, C.c_uint8)
        s.spread_log = _ptr(self.spread_log, C.c_double)
        return s


@dataclass
class BatchResult:
    unscheduled: np.ndarray
    used_cpu: np.ndarray
    used_mem: np.ndarray
    placement: Optional[np.ndarray]
    used_vg: Optional[np.ndarray] = None
    gpu_slices: Optional[np.ndarray] = None        # [S][P] uint64: byte d = gpu-mem slices booked on device d (gpu_ids_of)
    preempt_risk: Optional[np.ndarray] = None      # [S] uint8 (oracle runs; the library: Context.fetch_preempt_risk)
    group_unscheduled: Optional[np.ndarray] = None # [S][G] int32: pods of group g left unscheduled (Context.fetch_group_counts; engines fill it on request)
    group_placed: Optional[np.ndarray] = None      # [S][G] int32: pods of group g placed
    headroom: Optional[np.ndarray] = None          # [S][K] int64: further pods like probe k that fit (Context.fetch_headroom; engines fill it on request)
    headroom_exact: Optional[np.ndarray] = None    # [K] bool: headroom[:, k] is what the scheduler would place, not an upper bound
    node_usage: Optional["NodeUsage"] = None       # per-node end state of the listed scenarios (Context.fetch_node_usage; on request)
    gpu_usage: Optional["GpuUsage"] = None         # per-device end state of the listed scenarios (Context.fetch_gpu_usage; on request)
    local_usage: Optional["LocalUsage"] = None     # Open-Local end state of the listed scenarios (Context.fetch_local_usage; on request)

    def c_out(self) -> BatchOut:
        o = BatchOut()
        o.struct_size = C.sizeof(BatchOut)
        o.flags = 0
        o.unscheduled = _ptr(self.unscheduled, C.c_int32)
        o.used_cpu = _ptr(self.used_cpu, C.c_int64)
        o.used_mem = _ptr(self.used_mem, C.c_int64)
        o.placement = _ptr(self.placement, C.c_int32)
        o.used_vg = _ptr(self.used_vg, C.c_int64)
        o.gpu_slices = _ptr(self.gpu_slices, C.c_uint64)
        return o

    @staticmethod
    def alloc(S: int, P: int, want_placement: bool = True, want_gpu_slices: bool = False) -> "BatchResult":
        return BatchResult(np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S, np.int64),
                           np.full((S, P), -9, np.int32) if want_placement else None, np.zeros(S, np.int64),
                           np.zeros((S, P), np.uint64) if want_gpu_slices else None)


@dataclass
class NodeUsage:
    """simon_fetch_node_usage: the per-node end state of the listed scenarios (row i = scenarios[i], column j = pool node j)."""
    scenarios: np.ndarray               # [n] the indices as listed
    req_cpu: np.ndarray                 # [n][N] int64 Requested.MilliCPU
    req_mem: np.ndarray                 # [n][N] int64
    npods: np.ndarray                   # [n][N] int32 len(NodeInfo.Pods); -1 = the scenario does not hold node j
    req_eph: Optional[np.ndarray] = None      # [n][N] int64, on request
    scalar_req: Optional[np.ndarray] = None   # [n][K][N] int64, on request


class NodeUsageC(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("req_cpu", _p64), ("req_mem", _p64), ("req_eph", _p64), ("scalar_req", _p64), ("npods", _p32)]


@dataclass
class GpuUsage:
    """simon_fetch_gpu_usage: the GPU-share devices at the end of the listed scenarios (row i = scenarios[i], pool node j, device d)."""
    scenarios: np.ndarray               # [n] the indices as listed
    dev_used: np.ndarray                # [n][N][MAX_GPU_DEV] int64 GPU memory booked on the device (state before the stream included)
    dev_pods: Optional[np.ndarray] = None     # [n][N][MAX_GPU_DEV] int32 stream pods holding a slice of the device, on request; -1 = the scenario lacks node j


class GpuUsageC(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("dev_used", _p64), ("dev_pods", _p32)]


@dataclass
class LocalUsage:
    """simon_fetch_local_usage: the Open-Local storage at the end of the listed scenarios (row i = scenarios[i], pool node j)."""
    scenarios: np.ndarray               # [n] the indices as listed
    vg_req: np.ndarray                  # [n][N][MAX_VG] int64 SharedResource.Requested of the node's volume groups (state before the stream included)
    dev_alloc: Optional[np.ndarray] = None    # [n][N] int32 bit d = device d is allocated; -1 = the scenario lacks node j


class LocalUsageC(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vg_req", _p64), ("dev_alloc", _p32)]


WANT_PLACEMENT, WANT_GPU_SLICES = 1, 2


def pack_gpu_index(ids: Sequence[int]) -> int:
    """simon_pods_soa.gpu_index: device ids of an alibabacloud.com/gpu-index annotation ("0-0-1" -> [0, 0, 1]) as nibbles, low first."""
    ids = list(ids)
    if not 0 < len(ids) <= 8 or any(not 0 <= i < MAX_GPU_DEV for i in ids):
        raise ValueError(f"gpu-index {ids}: 1..8 ids in 0..{MAX_GPU_DEV - 1} can be packed")
    return sum((i + 1) << (4 * k) for k, i in enumerate(ids))


def gpu_ids_of(slices: int) -> List[int]:
    """Device ids of one simon_batch_out.gpu_slices entry, in the order GpuNodeInfo.AllocateGpuId lists them (ascending, an id once
    per slice): the content of the alibabacloud.com/gpu-index annotation ("-".join)."""
    out = []
    for d in range(MAX_GPU_DEV):
        out += [d] * ((int(slices) >> (8 * d)) & 0xFF)
    return out


MAX_ORDER_SEGMENTS = 64     # SIMON_MAX_ORDER_SEGMENTS
MAX_ORDER_VARIANTS = 1 << 24   # SIMON_MAX_ORDER_VARIANTS


class OrderSegmentsC(C.Structure):       # simon_order_segments
    _fields_ = [("struct_size", C.c_uint32), ("n_seg", C.c_int32), ("seg_start", _p32), ("n_variants", _p32), ("variant_pods", _p32),
                ("variant_live", _p32), ("choice", _p32)]


@dataclass
class OrderSegments:
    """Order rows as concatenations of per-segment variants (simon_load_scenarios_composed): order o = variants[g][choice[o][g]] for
    g = 0 .. G-1, one after the other; with `live`, order o holds the first live[g][choice[o][g]] pods of each piece and no others."""
    seg_start: np.ndarray                    # [G+1] stream positions, 0 .. P
    variants: List[np.ndarray]               # per segment [V_g][len_g] pod ids: every row a permutation of the segment's set
    live: Optional[List[np.ndarray]]         # per segment [V_g], or None = every pod of every row
    choice: np.ndarray                       # [n_orders][G]

    def __post_init__(self):
        self.seg_start = np.ascontiguousarray(self.seg_start, dtype=np.int32).reshape(-1)
        G = len(self.seg_start) - 1
        lens = np.diff(self.seg_start)
        # (an empty segment still has its variants: [V_g][0])
        self.variants = [np.asarray(v, np.int32) if g >= G else np.zeros((len(v), 0), np.int32) if lens[g] <= 0 else
                         np.ascontiguousarray(v, dtype=np.int32).reshape(-1, int(lens[g])) for g, v in enumerate(self.variants)]
        if self.live is not None:
            self.live = [np.ascontiguousarray(l, dtype=np.int32).reshape(-1) for l in self.live]
        self.choice = np.ascontiguousarray(self.choice, dtype=np.int32).reshape(-1, max(G, 1))
        if len(self.variants) != G or (self.live is not None and [len(l) for l in self.live] != [len(v) for v in self.variants]):
            raise ValueError(f"{G} segments, {len(self.variants)} variant tables" + ("" if self.live is None else f", live rows {[len(l) for l in self.live]}"))

    @property
    def n_orders(self) -> int:
        return len(self.choice)

    @property
    def n_pods(self) -> int:
        return int(self.seg_start[-1])

    def order(self, o: int) -> np.ndarray:
        """Row o of compose()'s orders alone."""
        return np.concatenate([rows[self.choice[o, g]] for g, rows in enumerate(self.variants)] + [np.zeros(0, np.int32)]).astype(np.int32)

    def compose(self):
        """The explicit rows: (orders int32 [n_orders][P], present bool [n_orders][P] by pod id) -- what the library composes on the device."""
        P, n = self.n_pods, self.n_orders
        orders = np.zeros((n, P), np.int32)
        present = np.zeros((n, P), bool)
        for g, rows in enumerate(self.variants):
            lo, hi = int(self.seg_start[g]), int(self.seg_start[g + 1])
            if hi == lo:
                continue
            pick = self.choice[:, g]
            piece = rows[pick]                                         # [n][len_g]
            orders[:, lo:hi] = piece
            n_live = np.full(n, hi - lo) if self.live is None else self.live[g][pick]
            keep = np.arange(hi - lo)[None, :] < n_live[:, None]
            present[np.nonzero(keep)[0], piece[keep]] = True
        return orders, present

    def c_struct(self):
        """(simon_order_segments, the arrays it points into)."""
        G = len(self.seg_start) - 1
        nv = np.array([len(v) for v in self.variants], np.int32)
        pods = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in self.variants] + [np.zeros(0, np.int32)]), dtype=np.int32)
        live = None if self.live is None else np.ascontiguousarray(np.concatenate(self.live + [np.zeros(0, np.int32)]), dtype=np.int32)
        o = OrderSegmentsC()
        o.struct_size, o.n_seg = C.sizeof(OrderSegmentsC), G
        o.seg_start, o.n_variants, o.variant_pods = _ptr(self.seg_start, C.c_int32), _ptr(nv, C.c_int32), _ptr(pods, C.c_int32)
        o.variant_live, o.choice = _ptr(live, C.c_int32), _ptr(self.choice, C.c_int32)
        return o, (nv, pods, live)


def scenarios_array(scen: Sequence) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(scen, dtype=np.int32).reshape(-1, 2))
    return a


def _pkg_dir() -> str:
    return os.path.dirname(os.path.abspath(__file__))


def library_path() -> str:
    """In-tree libsimon_hip.so; SIMON_HIP_LIB names another build of the SAME library (kernel A/B runs, profile builds)."""
    return os.environ.get("SIMON_HIP_LIB") or os.path.join(_pkg_dir(), "csrc", "libsimon_hip.so")


_LIB = None

EXPORTS = [
    "simon_hip_version", "simon_hip_device_count", "simon_ctx_create", "simon_ctx_destroy", "simon_last_error",
    "simon_load_nodes", "simon_load_pods", "simon_load_class_tables", "simon_load_scenarios", "simon_run_loaded",
    "simon_fetch_results", "simon_fetch_placement", "simon_fetch_gpu_slices", "simon_run_batch", "simon_min_plan", "simon_min_plan_vg", "simon_min_plan_device", "simon_explain", "simon_set_node_ranks",
    "simon_get_stats", "simon_device_results", "simon_explain_loaded", "simon_explain_local_detail", "simon_explain_batch",
    "simon_explain_own_batch",
    "simon_set_scalar_entries", "simon_set_pod_priorities", "simon_fetch_preempt_risk",
    "simon_group_set_scalar_entries", "simon_group_set_pod_priorities", "simon_group_fetch_preempt_risk",
    "simon_set_image_locality", "simon_group_set_image_locality", "simon_set_image_node_sizes", "simon_fetch_image_scores",
    "simon_set_scenario_segments", "simon_set_scenario_nodes", "simon_fetch_node_ranks", "simon_set_pod_eviction",
    "simon_set_own_nodes_all_feature",
    "simon_set_scenario_pods", "simon_fetch_group_counts", "simon_fetch_node_usage", "simon_fetch_headroom",
    "simon_fetch_gpu_usage", "simon_fetch_headroom_gpu", "simon_fetch_local_usage", "simon_fetch_headroom_local",
    "simon_load_scenarios_composed", "simon_fetch_orders",
    "simon_group_create", "simon_group_destroy", "simon_group_last_error", "simon_group_size", "simon_group_member",
    "simon_group_load_nodes", "simon_group_load_pods", "simon_group_load_class_tables", "simon_group_load_scenarios",
    "simon_group_run_loaded", "simon_group_fetch_results", "simon_group_run_batch", "simon_group_fetch_placement", "simon_group_fetch_gpu_slices",
    "simon_group_min_plan", "simon_group_collective",
]


def load_library(path: Optional[str] = None):
    """dlopen libsimon_hip.so and declare prototypes.  Raises if the library is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    path = path or library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.simon_hip_version.restype = C.c_int
    lib.simon_hip_device_count.restype = C.c_int
    lib.simon_ctx_create.restype = vp
    lib.simon_ctx_create.argtypes = [C.c_int]
    lib.simon_ctx_destroy.argtypes = [vp]
    lib.simon_ctx_destroy.restype = None
    lib.simon_last_error.restype = C.c_char_p
    lib.simon_last_error.argtypes = [vp]
    lib.simon_load_nodes.argtypes = [vp, C.POINTER(NodesSoA)]
    lib.simon_load_pods.argtypes = [vp, C.POINTER(PodsSoA)]
    lib.simon_load_class_tables.argtypes = [vp, C.POINTER(ClassTables)]
    lib.simon_load_scenarios.argtypes = [vp, C.POINTER(Scenario), C.c_int32, _p32, C.c_int32]
    lib.simon_run_loaded.argtypes = [vp, C.c_int32]
    lib.simon_fetch_results.argtypes = [vp, C.POINTER(BatchOut)]
    lib.simon_fetch_placement.argtypes = [vp, C.c_int32, _p32]
    lib.simon_fetch_gpu_slices.argtypes = [vp, C.c_int32, _pu64]
    lib.simon_run_batch.argtypes = [vp, C.POINTER(Scenario), C.c_int32, _p32, C.c_int32, C.POINTER(BatchOut)]
    lib.simon_set_node_ranks.argtypes = [vp, _p32]
    lib.simon_set_scenario_segments.argtypes = [vp, C.c_int32, _p32, _p32]
    lib.simon_set_scenario_nodes.argtypes = [vp, C.POINTER(C.c_uint32), _p32, C.c_int32]
    lib.simon_set_scenario_nodes.restype = C.c_int
    lib.simon_fetch_node_ranks.argtypes = [vp, _p32]
    lib.simon_set_image_node_sizes.argtypes = [vp, _p64]
    lib.simon_set_image_node_sizes.restype = C.c_int
    lib.simon_fetch_image_scores.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint8)]
    lib.simon_set_pod_eviction.argtypes = [vp, C.POINTER(C.c_uint8)]
    lib.simon_set_pod_eviction.restype = C.c_int
    lib.simon_set_own_nodes_all_feature.argtypes = [vp, C.c_int32]
    lib.simon_set_own_nodes_all_feature.restype = C.c_int
    lib.simon_set_scenario_pods.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.simon_set_scenario_pods.restype = C.c_int
    lib.simon_load_scenarios_composed.argtypes = [vp, C.POINTER(Scenario), C.c_int32, C.POINTER(OrderSegmentsC), C.c_int32]
    lib.simon_load_scenarios_composed.restype = C.c_int
    lib.simon_fetch_orders.argtypes = [vp, C.c_int32, C.c_int32, _p32, C.POINTER(C.c_uint32)]
    lib.simon_fetch_orders.restype = C.c_int
    lib.simon_fetch_group_counts.argtypes = [vp, _p32, C.c_int32, _p32, _p32]
    lib.simon_fetch_group_counts.restype = C.c_int
    lib.simon_fetch_node_usage.argtypes = [vp, _p32, C.c_int32, C.POINTER(NodeUsageC)]
    lib.simon_fetch_node_usage.restype = C.c_int
    lib.simon_fetch_headroom.argtypes = [vp, _p32, C.c_int32, _p64, _p32, C.POINTER(C.c_uint8)]
    lib.simon_fetch_headroom.restype = C.c_int
    lib.simon_fetch_gpu_usage.argtypes = [vp, _p32, C.c_int32, C.POINTER(GpuUsageC)]
    lib.simon_fetch_gpu_usage.restype = C.c_int
    lib.simon_fetch_headroom_gpu.argtypes = [vp, _p32, C.c_int32, _p64, _p32, C.POINTER(C.c_uint8)]
    lib.simon_fetch_headroom_gpu.restype = C.c_int
    lib.simon_fetch_local_usage.argtypes = [vp, _p32, C.c_int32, C.POINTER(LocalUsageC)]
    lib.simon_fetch_local_usage.restype = C.c_int
    lib.simon_fetch_headroom_local.argtypes = [vp, _p32, C.c_int32, _p64, _p32, C.POINTER(C.c_uint8)]
    lib.simon_fetch_headroom_local.restype = C.c_int
    lib.simon_min_plan.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(Plan)]
    lib.simon_min_plan_vg.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Plan), C.POINTER(C.c_int32)]
    lib.simon_explain.argtypes = [vp, Scenario, _p32, _p32, _pu16, C.c_int32]
    lib.simon_explain_loaded.argtypes = [vp, C.c_int32, _p32, _pu16, C.c_int32]
    lib.simon_explain_local_detail.argtypes = [vp, _p64, C.c_int32]
    lib.simon_explain_batch.argtypes = [vp, _p32, C.c_int32, C.c_int32, C.c_int32, _p32, _p32, _p32, C.c_void_p, _pu16, C.c_int32]
    lib.simon_explain_own_batch.argtypes = lib.simon_explain_batch.argtypes
    _pu8 = C.POINTER(C.c_uint8)
    for pre in ("simon_", "simon_group_"):
        getattr(lib, pre + "set_scalar_entries").argtypes = [vp, _pu8]
        getattr(lib, pre + "set_scalar_entries").restype = C.c_int
        getattr(lib, pre + "set_pod_priorities").argtypes = [vp, _p32, C.c_int32]
        getattr(lib, pre + "set_pod_priorities").restype = C.c_int
        getattr(lib, pre + "fetch_preempt_risk").argtypes = [vp, _pu8]
        getattr(lib, pre + "fetch_preempt_risk").restype = C.c_int
        getattr(lib, pre + "set_image_locality").argtypes = [vp, C.POINTER(ImageLocalityC)]
        getattr(lib, pre + "set_image_locality").restype = C.c_int
    lib.simon_group_create.restype = vp
    lib.simon_group_create.argtypes = [_p32, C.c_int32]
    lib.simon_group_destroy.argtypes = [vp]
    lib.simon_group_destroy.restype = None
    lib.simon_group_last_error.restype = C.c_char_p
    lib.simon_group_last_error.argtypes = [vp]
    lib.simon_group_size.restype = C.c_int32
    lib.simon_group_size.argtypes = [vp]
    lib.simon_group_member.restype = vp
    lib.simon_group_member.argtypes = [vp, C.c_int32]
    lib.simon_group_load_nodes.argtypes = [vp, C.POINTER(NodesSoA)]
    lib.simon_group_load_pods.argtypes = [vp, C.POINTER(PodsSoA)]
    lib.simon_group_load_class_tables.argtypes = [vp, C.POINTER(ClassTables)]
    lib.simon_group_load_scenarios.argtypes = [vp, C.POINTER(Scenario), C.c_int32, _p32, C.c_int32]
    lib.simon_group_run_loaded.argtypes = [vp, C.c_int32]
    lib.simon_group_fetch_results.argtypes = [vp, C.POINTER(BatchOut)]
    lib.simon_group_run_batch.argtypes = [vp, C.POINTER(Scenario), C.c_int32, _p32, C.c_int32, C.POINTER(BatchOut)]
    lib.simon_group_fetch_placement.argtypes = [vp, C.c_int32, _p32]
    lib.simon_group_fetch_gpu_slices.argtypes = [vp, C.c_int32, _pu64]
    lib.simon_group_min_plan.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Plan), C.POINTER(C.c_int32)]
    lib.simon_group_collective.argtypes = [vp]
    lib.simon_group_collective.restype = C.c_int32
    lib.simon_min_plan_device.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp)]
    lib.simon_get_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.simon_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int or name.startswith(("simon_load", "simon_run", "simon_fetch", "simon_min",
                                                        "simon_explain", "simon_get", "simon_device", "simon_group_load",
                                                        "simon_group_run", "simon_group_fetch", "simon_group_min")):
            fn.restype = C.c_int
    if lib.simon_hip_version() != ABI_VERSION:
        raise RuntimeError(f"ABI mismatch: library {lib.simon_hip_version()} != binding {ABI_VERSION}")
    if path == library_path():
        _LIB = lib
    return lib


def presence_words(present) -> np.ndarray:
    """bool [S][N] -> uint32 [S][ceil(N / 32)], node j = bit (j & 31) of word j >> 5 (simon_set_scenario_nodes)."""
    m = np.ascontiguousarray(present, dtype=bool)
    if m.ndim != 2:
        raise ValueError("presence rows are [S][N]")
    m = np.pad(m, ((0, 0), (0, -m.shape[1] % 32)))
    return np.ascontiguousarray(np.packbits(m, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(len(m), -1)


EXPLAIN_BINS = 64     # SIMON_EXPLAIN_BINS
FAIL_BIN_DTYPE = np.dtype([("code", np.uint16), ("pad", np.uint16), ("count", np.int32)])     # simon_fail_bin


@dataclass
class ExplainBatch:
    """What simon_explain_batch returns for the listed scenarios (list position k, recorded failed pod i < min(n_failed[k], max_failed))."""
    scenarios: np.ndarray       # [k] the indices as listed
    n_nodes: np.ndarray         # [k] node count of every listed scenario
    n_failed: np.ndarray        # [k] unscheduled pods (may exceed max_failed)
    failed_pods: np.ndarray     # [k][max_failed]
    n_bins: np.ndarray          # [k][max_failed] distinct codes (may exceed max_bins); -1: more than EXPLAIN_BINS, take the row
    bins: np.ndarray            # [k][max_failed][max_bins] FAIL_BIN_DTYPE, ascending code
    rows: Optional[np.ndarray]  # [k][max_failed][code_stride] uint16 with rows=True: scenario k's codes in the first n_nodes[k] entries

    def recorded(self, k: int) -> int:
        return min(int(self.n_failed[k]), self.failed_pods.shape[1])

    def pod_bins(self, k: int, i: int):
        """(code, node count) pairs of failed pod i of listed scenario k, or None when they are incomplete (n_bins -1 or beyond max_bins)."""
        nb = int(self.n_bins[k, i])
        if nb < 0 or nb > self.bins.shape[2]:
            return None
        b = self.bins[k, i, :nb]
        return list(zip(b["code"].tolist(), b["count"].tolist()))


class SimonError(RuntimeError):
    pass


class Context:
    """RAII wrapper over simon_ctx (one HIP device, one stream)."""

    def __init__(self, device_id: int = 0, lib=None):
        self.lib = lib or load_library()
        self.h = self.lib.simon_ctx_create(int(device_id))
        if not self.h:
            raise SimonError("simon_ctx_create failed (no gfx950 device visible?)")
        self.problem: Optional[Problem] = None
        self.S = 0
        self.scen: Optional[np.ndarray] = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.simon_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc < 0:
            msg = self.lib.simon_last_error(self.h)
            err = SimonError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
            err.code = rc
            raise err
        return rc

    def load_problem(self, prob: Problem):
        prob.normalise()
        n, p, t = prob.c_nodes(), prob.c_pods(), prob.c_tables()
        self._check(self.lib.simon_load_nodes(self.h, C.byref(n)), "simon_load_nodes")
        self._check(self.lib.simon_load_pods(self.h, C.byref(p)), "simon_load_pods")
        if prob.scalar_entries is not None:
            self._check(self.lib.simon_set_scalar_entries(self.h, _ptr(prob.scalar_entries, C.c_uint8)), "simon_set_scalar_entries")
        if prob.priority is not None:
            self._check(self.lib.simon_set_pod_priorities(self.h, _ptr(prob.priority, C.c_int32), int(prob.init_min_priority)), "simon_set_pod_priorities")
        self._check(self.lib.simon_load_class_tables(self.h, C.byref(t)), "simon_load_class_tables")
        if prob.image_locality is not None:
            im = prob.image_locality.c_struct()
            self._check(self.lib.simon_set_image_locality(self.h, C.byref(im)), "simon_set_image_locality")
            if prob.image_locality.node_size is not None:
                self.set_image_node_sizes(prob.image_locality.node_size, nnz=len(prob.image_locality.node_image))
        self.problem = prob

    def load_scenarios(self, scen, orders: np.ndarray):
        scen = scenarios_array(scen)
        orders = np.ascontiguousarray(orders, dtype=np.int32).reshape(-1, self.problem.n_pods)
        self._check(self.lib.simon_load_scenarios(self.h, scen.ctypes.data_as(C.POINTER(Scenario)), len(scen),
                                                  _ptr(orders, C.c_int32), orders.shape[0]), "simon_load_scenarios")
        self.S = len(scen)
        self.scen = scen

    def load_scenarios_composed(self, scen, segments: OrderSegments):
        """load_scenarios with the order rows -- and, with segments.live, the pod rows -- composed on the device from the segment table
        (include/simon_hip.h: simon_load_scenarios_composed)."""
        scen = scenarios_array(scen)
        o, keep = segments.c_struct()
        self._check(self.lib.simon_load_scenarios_composed(self.h, scen.ctypes.data_as(C.POINTER(Scenario)), len(scen), C.byref(o), segments.n_orders),
                    "simon_load_scenarios_composed")
        del keep
        self.S = len(scen)
        self.scen = scen

    def fetch_orders(self, first: int = 0, n: Optional[int] = None, present: bool = False):
        """Rows [first, first + n) of the loaded orders (simon_fetch_orders); present=True: the pair (orders, bool [n][P] by pod id);
        present="words": the pair (orders, the packed uint32 words [n][ceil(P / 32)] as the library wrote them)."""
        P = self.problem.n_pods
        n = 1 if n is None else int(n)
        orders = np.zeros((max(n, 0), P), np.int32)
        words = np.zeros((max(n, 0), (P + 31) // 32), np.uint32) if present else None
        self._check(self.lib.simon_fetch_orders(self.h, int(first), n, _ptr(orders, C.c_int32), _ptr(words, C.c_uint32)), "simon_fetch_orders")
        if not present:
            return orders
        if present == "words":
            return orders, words
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little").astype(bool)
        if bits[:, P:].any():
            raise SimonError("simon_fetch_orders set presence bits beyond P")
        return orders, bits[:, :P]

    def run_loaded(self, want_placement: bool = True, want_gpu_slices: bool = False):
        flags = (WANT_PLACEMENT if want_placement else 0) | (WANT_GPU_SLICES if want_gpu_slices else 0)
        self._check(self.lib.simon_run_loaded(self.h, flags), "simon_run_loaded")

    def fetch(self, want_placement: bool = True, want_gpu_slices: bool = False) -> BatchResult:
        res = BatchResult.alloc(self.S, self.problem.n_pods, want_placement, want_gpu_slices)
        out = res.c_out()
        self._check(self.lib.simon_fetch_results(self.h, C.byref(out)), "simon_fetch_results")
        return res

    def fetch_gpu_slices(self, scenario: int) -> np.ndarray:
        row = np.zeros(self.problem.n_pods, np.uint64)
        self._check(self.lib.simon_fetch_gpu_slices(self.h, int(scenario), _ptr(row, C.c_uint64)), "simon_fetch_gpu_slices")
        return row

    def fetch_preempt_risk(self) -> np.ndarray:
        """[S] uint8: 1 = some pod failed while a pod of lower priority was placed -- DefaultPreemption could have evicted there, the
        scenario needs the reference's own path; 0 = exact (include/simon_hip.h: simon_fetch_preempt_risk)."""
        risk = np.zeros(self.S, np.uint8)
        self._check(self.lib.simon_fetch_preempt_risk(self.h, _ptr(risk, C.c_uint8)), "simon_fetch_preempt_risk")
        return risk

    def fetch_placement(self, scenario: int) -> np.ndarray:
        row = np.zeros(self.problem.n_pods, np.int32)
        self._check(self.lib.simon_fetch_placement(self.h, int(scenario), _ptr(row, C.c_int32)),
                    "simon_fetch_placement")
        return row

    def run_batch(self, scen, orders: np.ndarray, want_placement: bool = True, want_gpu_slices: bool = False) -> BatchResult:
        scen = scenarios_array(scen)
        orders = np.ascontiguousarray(orders, dtype=np.int32).reshape(-1, self.problem.n_pods)
        res = BatchResult.alloc(len(scen), self.problem.n_pods, want_placement, want_gpu_slices)
        out = res.c_out()
        self._check(self.lib.simon_run_batch(self.h, scen.ctypes.data_as(C.POINTER(Scenario)), len(scen),
                                             _ptr(orders, C.c_int32), orders.shape[0], C.byref(out)),
                    "simon_run_batch")
        self.S = len(scen)
        self.scen = scen
        return res

    def set_node_ranks(self, ranks) -> None:
        """Per-scenario nodeTree order: ranks[s][j] = position of pool node j in scenario s's canonical order (None: pool order)."""
        if ranks is None:
            self._check(self.lib.simon_set_node_ranks(self.h, None), "simon_set_node_ranks")
            return
        r = np.ascontiguousarray(ranks, dtype=np.int32)
        self._check(self.lib.simon_set_node_ranks(self.h, _ptr(r, C.c_int32)), "simon_set_node_ranks")

    def set_scenario_segments(self, seg_start, counts) -> None:
        """Pool segments (node-type mixes): fixed nodes [0, seg_start[0]), segment g = [seg_start[g], seg_start[g+1]); scenario s holds
        the fixed nodes and the first counts[s][g] nodes of every segment (include/simon_hip.h: simon_set_scenario_segments).
        seg_start None: back to prefix scenarios."""
        if seg_start is None or len(seg_start) == 0:
            self._check(self.lib.simon_set_scenario_segments(self.h, 0, None, None), "simon_set_scenario_segments")
            return
        st = np.ascontiguousarray(seg_start, dtype=np.int32)
        cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1, len(st))
        self._check(self.lib.simon_set_scenario_segments(self.h, len(st), _ptr(st, C.c_int32), _ptr(cn, C.c_int32)),
                    "simon_set_scenario_segments")

    def set_scenario_nodes(self, present, node_zone=None, n_zones: Optional[int] = None) -> None:
        """Node subsets: scenario s holds exactly the pool nodes with present[s][j] true (bool [S][N]); node_zone [N] = nodeTree zone id of
        every node (None: one zone, each scenario in pool order) -- include/simon_hip.h: simon_set_scenario_nodes.  present None: back to
        prefix scenarios.  n_zones: default the largest id + 1."""
        if present is None:
            self._check(self.lib.simon_set_scenario_nodes(self.h, None, None, 0), "simon_set_scenario_nodes")
            return
        words = presence_words(present)
        if node_zone is None:
            self._check(self.lib.simon_set_scenario_nodes(self.h, _ptr(words, C.c_uint32), None, 0), "simon_set_scenario_nodes")
            return
        z = np.ascontiguousarray(node_zone, dtype=np.int32)
        if z.shape != (np.asarray(present).shape[1],):
            raise ValueError(f"node_zone has shape {z.shape}, the pool {np.asarray(present).shape[1]} nodes")
        self._check(self.lib.simon_set_scenario_nodes(self.h, _ptr(words, C.c_uint32), _ptr(z, C.c_int32),
                                                       int(z.max(initial=0)) + 1 if n_zones is None else int(n_zones)),
                    "simon_set_scenario_nodes")

    def set_pod_eviction(self, evict) -> None:
        """evict bool [P]: the preset pods that a node-subset batch schedules like fresh pods in the scenarios that lack their node
        (include/simon_hip.h: simon_set_pod_eviction).  After load_problem, before set_scenario_nodes; None detaches."""
        if evict is None:
            self._check(self.lib.simon_set_pod_eviction(self.h, None), "simon_set_pod_eviction")
            return
        e = np.ascontiguousarray(np.asarray(evict) != 0, dtype=np.uint8)
        if e.shape != (self.problem.n_pods,):
            raise ValueError(f"evict has shape {e.shape}, the problem {self.problem.n_pods} pods")
        self._check(self.lib.simon_set_pod_eviction(self.h, _ptr(e, C.c_uint8)), "simon_set_pod_eviction")

    def set_own_nodes_all_feature(self, on: bool = True) -> None:
        """Context option (include/simon_hip.h: simon_set_own_nodes_all_feature): a segmented / node-subset batch whose problem routes to
        the all-feature kernel runs there instead of being refused.  Off by default; survives every load."""
        self._check(self.lib.simon_set_own_nodes_all_feature(self.h, 1 if on else 0), "simon_set_own_nodes_all_feature")

    def set_scenario_pods(self, present) -> None:
        """Pod subsets: scenario s holds pod p iff present[s][p] (bool [S][P], or the packed uint32 words [S][ceil(P / 32)]) and its gate
        admits it; an absent pod reads GATED and is counted nowhere (include/simon_hip.h: simon_set_scenario_pods).  After load_scenarios,
        before or after the node rows; None detaches."""
        if present is None:
            self._check(self.lib.simon_set_scenario_pods(self.h, None), "simon_set_scenario_pods")
            return
        P = self.problem.n_pods
        a = np.asarray(present)
        if a.dtype == np.uint32:
            words = np.ascontiguousarray(a)
            if words.ndim != 2 or words.shape[1] != (P + 31) // 32:
                raise ValueError(f"packed pod rows have shape {words.shape}, the problem {(P + 31) // 32} words per scenario")
        else:
            if a.ndim != 2 or a.shape[1] != P:
                raise ValueError(f"pod rows have shape {a.shape}, the problem {P} pods")
            words = presence_words(a)
            if words.shape[1] == 0:
                words = np.zeros((len(a), 0), np.uint32)
        if len(words) != self.S:
            raise ValueError(f"{len(words)} pod rows for {self.S} loaded scenarios")
        self._check(self.lib.simon_set_scenario_pods(self.h, _ptr(words, C.c_uint32)), "simon_set_scenario_pods")

    def fetch_group_counts(self, pod_group, G: int, placed: bool = False):
        """simon_fetch_group_counts: per scenario of the last run and pod group, the pods left unscheduled [S][G] -- and with placed=True
        the pair (unscheduled, placed).  pod_group [P] in [0, G) or -1 (not counted)."""
        g = np.ascontiguousarray(pod_group, dtype=np.int32)
        if g.shape != (self.problem.n_pods,):
            raise ValueError(f"pod_group has shape {g.shape}, the problem {self.problem.n_pods} pods")
        cells = (self.S, max(int(G), 0))
        uns = np.zeros(cells, np.int32)
        pl = np.zeros(cells, np.int32) if placed else None
        self._check(self.lib.simon_fetch_group_counts(self.h, _ptr(g, C.c_int32), int(G), _ptr(uns, C.c_int32), _ptr(pl, C.c_int32)),
                    "simon_fetch_group_counts")
        return (uns, pl) if placed else uns

    def fetch_node_usage(self, scen_ids=None, eph: bool = False, scalars: bool = False) -> NodeUsage:
        """simon_fetch_node_usage: requested cpu / memory (ephemeral storage, scalars on request) and pod count of every pool node at the
        end of the listed scenarios of the last run (None: all of them), reduced on the device from the placement matrix."""
        ids = np.arange(self.S, dtype=np.int32) if scen_ids is None else np.ascontiguousarray(scen_ids, dtype=np.int32).reshape(-1)
        n, N, K = len(ids), self.problem.n_nodes, 0 if self.problem.scalar_alloc is None else int(np.asarray(self.problem.scalar_alloc).shape[0])
        res = NodeUsage(ids, np.zeros((n, N), np.int64), np.zeros((n, N), np.int64), np.zeros((n, N), np.int32),
                        np.zeros((n, N), np.int64) if eph else None, np.zeros((n, K, N), np.int64) if scalars else None)
        o = NodeUsageC()
        o.struct_size = C.sizeof(NodeUsageC)
        o.req_cpu, o.req_mem, o.npods = _ptr(res.req_cpu, C.c_int64), _ptr(res.req_mem, C.c_int64), _ptr(res.npods, C.c_int32)
        o.req_eph = _ptr(res.req_eph, C.c_int64)
        o.scalar_req = _ptr(res.scalar_req if scalars and K else None, C.c_int64)
        self._check(self.lib.simon_fetch_node_usage(self.h, None if scen_ids is None else _ptr(ids, C.c_int32), n, C.byref(o)),
                    "simon_fetch_node_usage")
        return res

    def fetch_gpu_usage(self, scen_ids=None, pods: bool = False) -> GpuUsage:
        """simon_fetch_gpu_usage: GPU memory booked on every device of every pool node at the end of the listed scenarios of the last run
        (None: all of them; pods=True: also the stream pods per device), reduced on the device from the placement matrix and the recorded
        devices (run with want_gpu_slices)."""
        ids = np.arange(self.S, dtype=np.int32) if scen_ids is None else np.ascontiguousarray(scen_ids, dtype=np.int32).reshape(-1)
        n, N = len(ids), self.problem.n_nodes
        res = GpuUsage(ids, np.zeros((n, N, MAX_GPU_DEV), np.int64), np.zeros((n, N, MAX_GPU_DEV), np.int32) if pods else None)
        o = GpuUsageC()
        o.struct_size = C.sizeof(GpuUsageC)
        o.dev_used, o.dev_pods = _ptr(res.dev_used, C.c_int64), _ptr(res.dev_pods, C.c_int32)
        self._check(self.lib.simon_fetch_gpu_usage(self.h, None if scen_ids is None else _ptr(ids, C.c_int32), n, C.byref(o)),
                    "simon_fetch_gpu_usage")
        return res

    def fetch_local_usage(self, scen_ids=None) -> LocalUsage:
        """simon_fetch_local_usage: what every volume group of every pool node has requested and which exclusive devices are allocated at
        the end of the listed scenarios of the last run (None: all of them), replayed on the device from the placement matrix in the
        order of every scenario's stream."""
        ids = np.arange(self.S, dtype=np.int32) if scen_ids is None else np.ascontiguousarray(scen_ids, dtype=np.int32).reshape(-1)
        n, N = len(ids), self.problem.n_nodes
        res = LocalUsage(ids, np.zeros((n, N, MAX_VG), np.int64), np.zeros((n, N), np.int32))
        o = LocalUsageC()
        o.struct_size = C.sizeof(LocalUsageC)
        o.vg_req, o.dev_alloc = _ptr(res.vg_req, C.c_int64), _ptr(res.dev_alloc, C.c_int32)
        self._check(self.lib.simon_fetch_local_usage(self.h, None if scen_ids is None else _ptr(ids, C.c_int32), n, C.byref(o)),
                    "simon_fetch_local_usage")
        return res

    def fetch_headroom(self, probe_pods, nodes: bool = False, devices: bool = False, storage: bool = False):
        """simon_fetch_headroom: (fit [S][K] int64, fit_nodes [S][K] int32 or None, exact [K] bool) -- how many more pods like pod
        probe_pods[k] fit in every scenario of the last run, on how many nodes, and whether that count is what the scheduler would place
        (exact) or the resource-and-static-filter upper bound.  devices=True: simon_fetch_headroom_gpu -- a probe with a GPU request is
        also bounded by the slices the nodes' devices still hold, and is exact (run with want_gpu_slices).  storage=True:
        simon_fetch_headroom_local -- the device bound as above where the problem has GPUs, and a probe whose class has Open-Local
        volumes is bounded by what the nodes' volume groups and exclusive devices still hold, and is exact."""
        pp = np.ascontiguousarray(probe_pods, dtype=np.int32).reshape(-1)
        K = len(pp)
        fit = np.zeros((self.S, K), np.int64)
        fn = np.zeros((self.S, K), np.int32) if nodes else None
        ex = np.zeros(K, np.uint8)
        call, name = (self.lib.simon_fetch_headroom_gpu, "simon_fetch_headroom_gpu") if devices else (self.lib.simon_fetch_headroom, "simon_fetch_headroom")
        if storage:
            call, name = self.lib.simon_fetch_headroom_local, "simon_fetch_headroom_local"
        self._check(call(self.h, _ptr(pp, C.c_int32), K, _ptr(fit, C.c_int64), _ptr(fn, C.c_int32), _ptr(ex, C.c_uint8)), name)
        return fit, fn, ex.astype(bool)

    def set_image_node_sizes(self, node_size, nnz: Optional[int] = None) -> None:
        """simon_set_image_node_sizes: int64 [nnz] sizeBytes of every node entry (parallel to ImageLocality.node_image), None detaches."""
        if node_size is None:
            self._check(self.lib.simon_set_image_node_sizes(self.h, None), "simon_set_image_node_sizes")
            return
        a = np.ascontiguousarray(node_size, dtype=np.int64).reshape(-1)
        if nnz is None:                          # (the library reads as many entries as the loaded image input lists)
            prob = getattr(self, "problem", None)
            # (no image input went through load_problem: the library refuses with SIMON_ESTATE before it reads anything)
            nnz = len(a) if prob is None or prob.image_locality is None else len(prob.image_locality.node_image)
        if len(a) != nnz:
            raise ValueError(f"node_size has {len(a)} entries, the image input lists {nnz}")
        keep = a if len(a) else np.zeros(1, np.int64)
        self._check(self.lib.simon_set_image_node_sizes(self.h, _ptr(keep, C.c_int64)), "simon_set_image_node_sizes")

    def fetch_image_scores(self, scenario: int) -> np.ndarray:
        """[Cp][N] uint8: ImageLocality of every (pod class, pool node) in one scenario of the loaded batch, read back from the staged
        device table (0 for absent nodes and for classes that run no listed image); SIMON_ESTATE without a batch or without images."""
        out = np.zeros((self.problem.n_pod_classes, self.problem.n_nodes), np.uint8)
        self._check(self.lib.simon_fetch_image_scores(self.h, int(scenario), out.ctypes.data_as(C.POINTER(C.c_uint8))), "simon_fetch_image_scores")
        return out

    def fetch_node_ranks(self) -> np.ndarray:
        """[S][N] the rank rows in effect (nodes a segmented / node-subset scenario lacks: N); SIMON_ESTATE for a batch without rows."""
        rank = np.zeros((self.S, self.problem.n_nodes), np.int32)
        self._check(self.lib.simon_fetch_node_ranks(self.h, _ptr(rank, C.c_int32)), "simon_fetch_node_ranks")
        return rank

    def min_plan(self, max_cpu_pct: int = 100, max_mem_pct: int = 100) -> Plan:
        plan = Plan()
        self._check(self.lib.simon_min_plan(self.h, int(max_cpu_pct), int(max_mem_pct), C.byref(plan)),
                    "simon_min_plan")
        return plan

    def min_plan_vg(self, max_cpu_pct: int = 100, max_mem_pct: int = 100, max_vg_pct: int = 100):
        """simon_min_plan with the MaxVG cap; returns (Plan, vg_pct of the winning scenario)."""
        plan, vg = Plan(), C.c_int32(0)
        self._check(self.lib.simon_min_plan_vg(self.h, int(max_cpu_pct), int(max_mem_pct), int(max_vg_pct), C.byref(plan),
                                               C.byref(vg)), "simon_min_plan_vg")
        return plan, int(vg.value)

    def explain(self, n_nodes: int, order: np.ndarray, max_failed: int = 64):
        order = np.ascontiguousarray(order, dtype=np.int32)
        failed = np.full(max_failed, -1, np.int32)
        codes = np.zeros((max_failed, n_nodes), np.uint16)
        sc = Scenario(int(n_nodes), 0)
        n = self._check(self.lib.simon_explain(self.h, sc, _ptr(order, C.c_int32), _ptr(failed, C.c_int32),
                                               _ptr(codes, C.c_uint16), int(max_failed)), "simon_explain")
        k = min(n, max_failed)
        return n, failed[:k], codes[:k]

    def explain_loaded(self, scenario: int, max_failed: int = 64):
        """simon_explain_loaded: replay scenario `scenario` of the loaded batch (its order, its own node ranks)."""
        if not (self.scen is not None and 0 <= int(scenario) < len(self.scen)):
            raise SimonError(f"simon_explain_loaded: scenario {scenario} is not one of the {0 if self.scen is None else len(self.scen)} loaded")
        n_nodes = int(self.scen[scenario, 0])
        failed = np.full(max_failed, -1, np.int32)
        codes = np.zeros((max_failed, n_nodes), np.uint16)
        n = self._check(self.lib.simon_explain_loaded(self.h, int(scenario), _ptr(failed, C.c_int32), _ptr(codes, C.c_uint16),
                                                      int(max_failed)), "simon_explain_loaded")
        k = min(n, max_failed)
        return n, failed[:k], codes[:k]

    def explain_batch(self, scenarios, max_failed: int = 64, max_bins: int = 32, rows: bool = False,
                      code_stride: Optional[int] = None) -> "ExplainBatch":
        """simon_explain_batch: replay the listed scenarios of the loaded batch (indices in any order, repeats allowed) in one launch;
        per failed pod the (code, node count) histogram of its per-node failure codes, and with rows=True the full code rows too
        (row stride: the largest listed n_nodes unless code_stride says otherwise)."""
        idx = np.ascontiguousarray(scenarios, dtype=np.int32).reshape(-1)
        k = len(idx)
        if rows and code_stride is None:
            ok = self.scen is not None and k > 0 and bool(((idx >= 0) & (idx < len(self.scen))).all())
            code_stride = max(int(self.scen[idx, 0].max()), 1) if ok else 1        # (a bad index is the library's to refuse)
        stride = int(code_stride) if rows else 0
        n_failed = np.zeros(k, np.int32)
        failed = np.zeros((k, max(int(max_failed), 0)), np.int32)
        n_bins = np.zeros((k, max(int(max_failed), 0)), np.int32)
        bins = np.zeros((k, max(int(max_failed), 0), max(int(max_bins), 0)), FAIL_BIN_DTYPE)
        codes = np.zeros((k, max(int(max_failed), 0), max(stride, 0)), np.uint16) if rows else None
        self._check(self.lib.simon_explain_batch(self.h, _ptr(idx, C.c_int32), k, int(max_failed), int(max_bins), _ptr(n_failed, C.c_int32),
                                                 _ptr(failed, C.c_int32), _ptr(n_bins, C.c_int32), bins.ctypes.data_as(C.c_void_p),
                                                 _ptr(codes, C.c_uint16), stride), "simon_explain_batch")
        n_nodes = self.scen[idx, 0].astype(np.int32)
        return ExplainBatch(idx, n_nodes, n_failed, failed, n_bins, bins, codes)

    def explain_own_batch(self, scenarios, max_failed: int = 64, max_bins: int = 32, rows: bool = False) -> "ExplainBatch":
        """simon_explain_own_batch: explain_batch for the loaded segmented / node-subset batch.  Bins count each scenario's own nodes; with
        rows=True the code rows are [k][max_failed][N], indexed by POOL node, 0 on the nodes a scenario lacks."""
        idx = np.ascontiguousarray(scenarios, dtype=np.int32).reshape(-1)
        k, mf, mb = len(idx), max(int(max_failed), 0), max(int(max_bins), 0)
        stride = self.problem.n_nodes if rows else 0
        n_failed = np.zeros(k, np.int32)
        failed = np.zeros((k, mf), np.int32)
        n_bins = np.zeros((k, mf), np.int32)
        bins = np.zeros((k, mf, mb), FAIL_BIN_DTYPE)
        codes = np.zeros((k, mf, stride), np.uint16) if rows else None
        self._check(self.lib.simon_explain_own_batch(self.h, _ptr(idx, C.c_int32), k, int(max_failed), int(max_bins), _ptr(n_failed, C.c_int32),
                                                     _ptr(failed, C.c_int32), _ptr(n_bins, C.c_int32), bins.ctypes.data_as(C.c_void_p),
                                                     _ptr(codes, C.c_uint16), stride), "simon_explain_own_batch")
        return ExplainBatch(idx, self.scen[idx, 0].astype(np.int32), n_failed, failed, n_bins, bins, codes)

    def explain_local_detail(self, n_failed: int, n_nodes: int) -> Optional[np.ndarray]:
        """simon_explain_local_detail after explain / explain_loaded: [n_failed][n_nodes][4] int64 {LOCAL_ERR_*, a, b, c} -- what
        Open-Local's error texts carry -- or None when the problem has no local storage."""
        if n_failed <= 0:
            return None
        detail = np.zeros((int(n_failed), int(n_nodes), 4), np.int64)
        k = self._check(self.lib.simon_explain_local_detail(self.h, _ptr(detail, C.c_int64), int(n_failed)), "simon_explain_local_detail")
        return detail[:k] if k > 0 else None

    def stats(self) -> Stats:
        st = Stats()
        self._check(self.lib.simon_get_stats(self.h, C.byref(st)), "simon_get_stats")
        return st

    def device_results(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.simon_device_results(self.h, C.byref(a), C.byref(b), C.byref(c)),
                    "simon_device_results")
        return a.value, b.value, c.value


class Group:
    """RAII wrapper over simon_group: several devices of one node behind one handle (scenario s runs on member
    s % n_dev; all scenario indices are the caller's)."""

    def __init__(self, device_ids: Sequence[int], lib=None):
        self.lib = lib or load_library()
        ids = np.ascontiguousarray(device_ids, np.int32)
        self.h = self.lib.simon_group_create(_ptr(ids, C.c_int32), len(ids))
        if not self.h:
            raise SimonError(f"simon_group_create({list(device_ids)}) failed (no such gfx950 device?)")
        self.problem: Optional[Problem] = None
        self.S = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.simon_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc < 0:
            msg = self.lib.simon_group_last_error(self.h)
            raise SimonError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    @property
    def size(self) -> int:
        return int(self.lib.simon_group_size(self.h))

    def member_stats(self, i: int) -> Stats:
        st = Stats()
        rc = self.lib.simon_get_stats(self.lib.simon_group_member(self.h, int(i)), C.byref(st))
        if rc < 0:
            raise SimonError(f"simon_get_stats(member {i}) failed ({rc})")
        return st

    def load_problem(self, prob: Problem):
        prob.normalise()
        n, p, t = prob.c_nodes(), prob.c_pods(), prob.c_tables()
        self._check(self.lib.simon_group_load_nodes(self.h, C.byref(n)), "simon_group_load_nodes")
        self._check(self.lib.simon_group_load_pods(self.h, C.byref(p)), "simon_group_load_pods")
        if prob.scalar_entries is not None:
            self._check(self.lib.simon_group_set_scalar_entries(self.h, _ptr(prob.scalar_entries, C.c_uint8)), "simon_group_set_scalar_entries")
        if prob.priority is not None:
            self._check(self.lib.simon_group_set_pod_priorities(self.h, _ptr(prob.priority, C.c_int32), int(prob.init_min_priority)), "simon_group_set_pod_priorities")
        self._check(self.lib.simon_group_load_class_tables(self.h, C.byref(t)), "simon_group_load_class_tables")
        if prob.image_locality is not None:
            im = prob.image_locality.c_struct()
            self._check(self.lib.simon_group_set_image_locality(self.h, C.byref(im)), "simon_group_set_image_locality")
        self.problem = prob

    def load_scenarios(self, scen, orders: np.ndarray):
        scen = scenarios_array(scen)
        orders = np.ascontiguousarray(orders, dtype=np.int32).reshape(-1, self.problem.n_pods)
        self._check(self.lib.simon_group_load_scenarios(self.h, scen.ctypes.data_as(C.POINTER(Scenario)), len(scen),
                                                        _ptr(orders, C.c_int32), orders.shape[0]), "simon_group_load_scenarios")
        self.S = len(scen)

    def run_loaded(self, want_placement: bool = True, want_gpu_slices: bool = False):
        flags = (WANT_PLACEMENT if want_placement else 0) | (WANT_GPU_SLICES if want_gpu_slices else 0)
        self._check(self.lib.simon_group_run_loaded(self.h, flags), "simon_group_run_loaded")

    def fetch(self, want_placement: bool = True, want_gpu_slices: bool = False) -> BatchResult:
        res = BatchResult.alloc(self.S, self.problem.n_pods, want_placement, want_gpu_slices)
        out = res.c_out()
        self._check(self.lib.simon_group_fetch_results(self.h, C.byref(out)), "simon_group_fetch_results")
        return res

    def run_batch(self, scen, orders: np.ndarray, want_placement: bool = True, want_gpu_slices: bool = False) -> BatchResult:
        self.load_scenarios(scen, orders)
        self.run_loaded(want_placement, want_gpu_slices)
        return self.fetch(want_placement, want_gpu_slices)

    def fetch_placement(self, scenario: int) -> np.ndarray:
        row = np.zeros(self.problem.n_pods, np.int32)
        self._check(self.lib.simon_group_fetch_placement(self.h, int(scenario), _ptr(row, C.c_int32)), "simon_group_fetch_placement")
        return row

    def fetch_gpu_slices(self, scenario: int) -> np.ndarray:
        row = np.zeros(self.problem.n_pods, np.uint64)
        self._check(self.lib.simon_group_fetch_gpu_slices(self.h, int(scenario), _ptr(row, C.c_uint64)), "simon_group_fetch_gpu_slices")
        return row

    def fetch_preempt_risk(self) -> np.ndarray:
        risk = np.zeros(self.S, np.uint8)
        self._check(self.lib.simon_group_fetch_preempt_risk(self.h, _ptr(risk, C.c_uint8)), "simon_group_fetch_preempt_risk")
        return risk

    def min_plan(self, max_cpu_pct: int = 100, max_mem_pct: int = 100, max_vg_pct: int = 100):
        plan, vg = Plan(), C.c_int32(0)
        self._check(self.lib.simon_group_min_plan(self.h, int(max_cpu_pct), int(max_mem_pct), int(max_vg_pct), C.byref(plan),
                                                  C.byref(vg)), "simon_group_min_plan")
        return plan, int(vg.value)

    def collective(self) -> str:
        """How the last min_plan combined the members' plans: "rccl_all_gather" (members on distinct devices: one ncclAllGather of the
        8-byte plan keys, device to device) or "host" (one member / shared devices / librccl unavailable)."""
        return {0: "host", 1: "rccl_all_gather"}.get(int(self.lib.simon_group_collective(self.h)), "?")

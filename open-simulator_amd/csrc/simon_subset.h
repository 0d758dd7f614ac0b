// simon_subset.h -- device-side staging of a node-subset batch (simon_set_scenario_nodes): what the host builds for a segmented batch
// (rank rows, per-class node lists, class counts, allocatable totals), from the presence words of every scenario.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace simon {

constexpr int kSubsetMaxZones = 64;          // SIMON_MAX_ZONES: one lane of the staging wave per zone

struct SubsetStage {
    // inputs
    const uint32_t* present;                 // [S][W] node j = bit (j & 31) of word j >> 5
    const int32_t* node_zone;                // [N] ids in [0, kSubsetMaxZones), or nullptr = one zone
    const int32_t* ncls;                     // [N] table class of every node, or nullptr = no class outputs (rk_ids, rk_pos, scls)
    const int32_t* cls_off;                  // [Ct + 1] class offsets into a scenario's row of rk_ids
    const int64_t *prefix_cpu, *prefix_mem, *prefix_vg;   // [N + 1] prefix sums over the pool: node j's value = prefix[j + 1] - prefix[j]
    int32_t S, N, W, Ct;
    // outputs
    int32_t *rank, *inv;                     // [S][N] rank of node j in the scenario's nodeTree order (absent: N); node of rank r (zeroed by the caller)
    int32_t *rk_ids, *rk_pos;                // [S][N] per-class node lists in rank order; a node's index inside its class (both zeroed by the caller)
    int32_t* scls;                           // [S][Ct] nodes of class d the scenario holds
    int64_t* tot;                            // [3][S] allocatable cpu / memory and VG capacity of the scenario's own nodes
};

// one wave per scenario on `st`; nothing is read back here
hipError_t launch_subset_stage(const SubsetStage& a, hipStream_t st);

// image_states_kernel: the ImageLocality score table of an own-nodes batch, one 256-thread workgroup per slot (image state: a node count
// and a presence row).  schedulerCache.addNodeImageStates over the slot's nodes in pool order (cache.go:675-698): NumNodes of node j's
// entry of image i = present listers of i at or before j, Size(i) = the first present lister's own sizeBytes.  Phase A derives both from
// the lister lists (a CSR by image, pool order) with ballots and a carry across 64-lister chunks; phase B scores every (image-scoring
// row, node class) at the class's representative node in plain IEEE fp64, as img_score of simon_hip.hip does.
constexpr size_t kImageLdsBudget = 48 * 1024;   // counts [nnz] + first listers [I] as int32 stay in LDS up to this, else in a global row per slot

struct ImageStates {
    // inputs
    const uint32_t* present;                 // [T][W] presence words of every slot
    const int32_t* slot_n;                   // [T] node count of the slot, >= 1
    const int32_t *lis_off, *lis_node, *lis_ent;   // [I + 1]; [nnz] listers of image i in pool order: the node, its entry index q
    const int64_t* node_size;                // [nnz] sizeBytes of entry q
    const int32_t *node_off, *node_image;    // [N + 1]; [nnz] entries by node
    const int32_t *class_off, *class_image;  // [Cp + 1]; containers by pod class (-1: listed nowhere)
    const int32_t* row_class;                // [R] pod class of image-scoring row r
    const int32_t* rep;                      // [Cn] representative node of a node class, -1 = the class is empty
    int32_t T, W, I, nnz, R, Cn;
    int32_t* scratch;                        // [T][nnz + I], or nullptr = LDS ((nnz + I) * 4 <= kImageLdsBudget)
    // output
    uint8_t* out;                            // [T][R][Cn]
};

hipError_t launch_image_states(const ImageStates& a, hipStream_t st);

// simon_fetch_group_counts: per scenario and pod group, the pods left unscheduled (placement == -1) and the pods placed (>= 0) -- a pod that
// is not part of the scenario (-2) counts in neither.  placement [S][P] by pod id, pod_group [P] in [0, G) or -1 (validated by the caller),
// unscheduled / placed [S][G] (placed may be null).  One workgroup per scenario, two G-entry histograms in LDS.
constexpr int kMaxPodGroups = 1024;          // SIMON_MAX_POD_GROUPS
hipError_t launch_group_counts(const int32_t* placement, const int32_t* pod_group, int S, int P, int G, int32_t* unscheduled, int32_t* placed,
                               hipStream_t st);

// simon_fetch_node_usage / simon_fetch_headroom: the placement matrix reduced over the node dimension.  One 256-thread workgroup per
// scenario accumulates, per tile of `tile` pool nodes, the request sums and pod counts of the pods placed on the tile's nodes in LDS
// (LDS atomics; integer sums, so the result does not depend on the order), re-reading the placement row per tile.  Resource rows:
// 0 cpu, 1 memory, 2 ephemeral storage, 3 + k scalar k; pod_req [kUsageRows][P] and node_init / node_alloc [kUsageRows][N] are compact
// int64 copies of the caller's arrays (rows the problem lacks are zero).  A scenario holds node j iff rank ? rank[s][j] < N : j < n_nodes.
constexpr int kUsageMaxScalar = 4;           // SIMON_MAX_SCALAR
constexpr int kUsageRows = 3 + kUsageMaxScalar;
constexpr int kMaxProbes = 64;               // SIMON_MAX_PROBES
constexpr size_t kUsageLdsBudget = 40 * 1024;   // default tile: the largest multiple of 64 nodes whose rows fit (four workgroups per CU)

struct UsageCommon {
    const int32_t* placement;                // [S][P] by pod id
    const int32_t* scen;                     // [S][2] ScenarioDesc: n_nodes, order_id
    const int32_t* rank;                     // [S][N] rank rows of an own-nodes batch, or nullptr = prefix scenarios
    const int64_t* pod_req;                  // [kUsageRows][P]
    const int64_t* node_init;                // [kUsageRows][N] requested before the stream
    const int32_t* init_npods;               // [N]
    int32_t P, N, tile;
    int32_t nrows;                           // accumulated rows
    int32_t row_src[kUsageRows];             // their resource row (ascending)
};

struct UsageOut {
    const int32_t* scen_ids;                 // [n] listed scenarios, or nullptr = 0 .. n-1
    int64_t* rows[kUsageRows];               // per accumulated row i: [n][N]  (scalars: the caller's [n][K][N] is written with stride_n)
    size_t row_stride[kUsageRows];           // elements between two listed scenarios of row i
    int32_t* npods;                          // [n][N]
};

struct ProbeRow {                            // one probe of simon_fetch_headroom
    int64_t q[kUsageRows];                   // its request
    uint32_t checked;                        // bit r: fitsRequest compares resource row r (0 = the all-zero shortcut: pod slots only)
    uint32_t pad;
};

struct HeadroomArgs {
    const int64_t* node_alloc;               // [kUsageRows][N]
    const int32_t* alloc_pods;               // [N]
    const ProbeRow* probes;                  // [K]
    const uint64_t* probe_mask;              // [K][ceil(N / 64)] static_mask row of every probe's class
    int32_t K;
    int64_t* fit;                            // [S][K]
    int32_t* fit_nodes;                      // [S][K] or nullptr
};

// GPU-share devices (simon_fetch_gpu_usage, simon_fetch_headroom_gpu): the recorded slices reduced next to the placement matrix.  Per
// tile the device sums sit in LDS as s_dev[tile][8] u64 (s_dpods[tile][8] i32 where asked for), 64 (96) bytes per node; device d of tile
// node jj is slot dev_slot(jj, d): the eight devices of a node stay in the node's own 64 bytes, rotated by the node index, so that the
// same device of neighbouring nodes (device 0 takes most bookings) does not fall on one pair of banks (docs/KERNELS.md).
constexpr int kGpuDev = 8;                   // SIMON_MAX_GPU_DEV
constexpr int kDevBytes = kGpuDev * 8, kDevPodsBytes = kGpuDev * 4;

struct DevUsage {
    const uint64_t* slices;                  // [S][P] byte d = slices booked on device d, or nullptr = no GPU request anywhere (nothing was booked)
    const int64_t* gpu_mem;                  // [P] GPU memory per slice (0: the pod's slices word is not read)
    const int32_t* node_cnt;                 // [N] devices of node j: min(gpu_cnt, kGpuDev), 0 = none
    const int64_t* per_dev;                  // [N] bytes per device: gpu_mem_total / gpu_cnt (0 without devices)
    const int64_t* init_used;                // [N][kGpuDev] booked before the stream
    // headroom only: the device bound of every probe
    const int64_t* probe_mem;                // [K] GPU memory per slice; 0 = no device bound for this probe
    const int32_t* probe_cnt;                // [K] min(gpu_cnt, 64); <= 0 = the pod fits no device (cap 0)
};

struct GpuUsageOut {
    const int32_t* scen_ids;                 // [n] listed scenarios, or nullptr = 0 .. n-1
    int64_t* dev_used;                       // [n][N][kGpuDev]
    int32_t* dev_pods;                       // [n][N][kGpuDev] or nullptr
};

__host__ __device__ inline int dev_slot(int jj, int d) { return jj * kGpuDev + ((d + (jj >> 1)) & (kGpuDev - 1)); }

// bytes of LDS one node of a tile costs in the two listed-scenario kernels (`dev`: 0, kDevBytes or kDevBytes + kDevPodsBytes on top of the
// resource rows; nrows = 0: devices only)
inline size_t usage_node_bytes(int nrows, int dev = 0) { return (nrows > 0 ? (size_t)nrows * 8 + 4 : 0) + (size_t)dev; }
// what the tile rule leaves free of a workgroup's 64 KB whatever the call: the headroom counters of kMaxProbes probes (16 B each kept)
constexpr size_t kTileReserve = 2 * kMaxProbes * 8;
// The node tile of every usage / headroom launch: N nodes of `per` bytes each next to `fixed` bytes of LDS that do not grow with the
// tile.  forced = 0: the largest multiple of 64 nodes inside the LDS budget; forced > 0 (SIMON_USAGE_TILE; 1 << 30 = a workgroup has a
// CU to itself): that, capped at what one workgroup's 64 KB hold.
inline int usage_tile(int N, size_t per, size_t fixed, int forced) {
    int t = forced > 0 ? forced : (int)(kUsageLdsBudget / per) / 64 * 64;
    const int cap = (int)((64 * 1024 - fixed) / per);
    t = t > cap ? cap : t;
    return t < 1 ? 1 : (t > N ? N : t);
}
// a.tile from usage_tile(N, usage_node_bytes(nrows), kTileReserve, forced)
hipError_t launch_node_usage(const UsageCommon& a, const UsageOut& o, int n, hipStream_t st);
// a.tile from usage_tile(N, usage_node_bytes(0, kDevBytes (+ kDevPodsBytes with dev_pods)), kTileReserve, forced); a.pod_req / node_init /
// init_npods are not read
hipError_t launch_gpu_usage(const UsageCommon& a, const DevUsage& g, const GpuUsageOut& o, int n, hipStream_t st);

// Open-Local storage (simon_fetch_local_usage, simon_fetch_headroom_local).  The state of a node is not a sum: which volume group a
// volume lands in and which devices a pod takes depend on the node's state at that moment, so the scheduled storage pods are REPLAYED
// in stream order -- per node, which is all the order that matters (a node's state depends only on the pods placed on it).  Per tile
// node LDS holds vg_req[4] int64 and the allocated-device mask, 36 bytes; the storage pods of the scenario's order (compact list, built
// on the host per order) are staged in chunks of kLocalChunk, and thread t applies the pods that sit on its tile nodes t, t + 256, ...
// front to back (broadcast LDS reads, no atomics).  docs/KERNELS.md has the layout.
constexpr int kLocalVG = 4, kLocalDev = 8, kLocalVol = 4;   // SIMON_MAX_VG, SIMON_MAX_LDEV, SIMON_MAX_LVOL
constexpr int kLocalBytes = kLocalVG * 8 + 4;
constexpr int kLocalChunk = 512;             // storage pods staged per pass (node and spec of each: 8 bytes)
constexpr size_t kLocalStageBytes = (size_t)kLocalChunk * 8;

struct LocalSpec {                           // simon_local_spec, field for field
    int32_t n_lvm, n_ssd, n_hdd, pad;
    int64_t lvm_size[kLocalVol];
    int32_t lvm_vg[kLocalVol];
    int64_t ssd_size[kLocalVol], hdd_size[kLocalVol];
};

struct LocalUsage {
    const LocalSpec* specs;                  // [n_local_specs]
    const int32_t* pod_spec;                 // [P] spec of the pod's class; -1 = no volumes or bound by Spec.NodeName (never reaches LocalPlugin.Bind)
    const int32_t* list;                     // the pods with pod_spec >= 0 in the sequence of every order, one order after the other
    const int32_t* list_off;                 // [n_orders + 1] order o's pods are list[list_off[o] .. list_off[o + 1])
    const int32_t* flags;                    // [N] bit0: the node carries the storage annotation; nullptr = a problem without Open-Local
    const int32_t* vg_cnt;                   // [N]
    const int64_t* vg_cap;                   // [N][kLocalVG]
    const int64_t* vg_init;                  // [N][kLocalVG] requested before the stream
    const int32_t* vg_name;                  // [N][kLocalVG]
    const int32_t* dev_cnt;                  // [N]
    const int64_t* dev_cap;                  // [N][kLocalDev]
    const int32_t* dev_media;                // [N] 2 bits per device
    const int32_t* dev_init;                 // [N] allocated before the stream
    const int32_t* probe_spec;               // headroom only: [K] spec of the probe's class or -1 = no storage bound
};

struct LocalUsageOut {
    const int32_t* scen_ids;                 // [n] listed scenarios, or nullptr = 0 .. n-1
    int64_t* vg_req;                         // [n][N][kLocalVG]
    int32_t* dev_alloc;                      // [n][N] or nullptr
};

// a.tile from usage_tile(N, kLocalBytes, kTileReserve + kLocalStageBytes, forced); a.pod_req / node_init / init_npods are not read
hipError_t launch_local_usage(const UsageCommon& a, const LocalUsage& l, const LocalUsageOut& o, int n, hipStream_t st);

// The LDS of one headroom workgroup (simon_fetch_headroom / _gpu / _local), stated once: headroom_kernel carves its arrays from these
// element counts in this order -- all 8-byte arrays ahead of all 4-byte ones, an absent part has size 0 --, the launcher sizes the
// launch with bytes(tile) and the host picks the tile from node_bytes() / reserve_bytes().
struct HeadroomLds {
    int nrows, K;                            // accumulated resource rows (>= 2), probes
    bool devices, storage;                   // the device bound's sums; the storage bound's node state and staged chunk
    __host__ __device__ size_t req(int tile) const { return (size_t)nrows * tile; }                  // u64 s_req[nrows][tile]
    __host__ __device__ size_t dev(int tile) const { return devices ? (size_t)tile * kGpuDev : 0; }  // u64 s_dev[tile][8]
    __host__ __device__ size_t vg(int tile) const { return storage ? (size_t)kLocalVG * tile : 0; }  // i64 s_vg[4][tile]
    __host__ __device__ size_t fit() const { return (size_t)K; }                                     // u64 s_fit[K]
    __host__ __device__ size_t cnt(int tile) const { return (size_t)tile; }                          // i32 s_cnt[tile]
    __host__ __device__ size_t nodes() const { return (size_t)K; }                                   // i32 s_nodes[K]
    __host__ __device__ size_t ldev(int tile) const { return storage ? (size_t)tile : 0; }           // i32 s_ldev[tile]
    __host__ __device__ size_t stage() const { return storage ? (size_t)2 * kLocalChunk : 0; }       // i32 s_stage[2][kLocalChunk]
    __host__ __device__ size_t bytes(int tile) const {
        return 8 * (req(tile) + dev(tile) + vg(tile) + fit()) + 4 * (cnt(tile) + nodes() + ldev(tile) + stage());
    }
    __host__ __device__ size_t node_bytes() const { return bytes(1) - bytes(0); }    // rows x 8 + 4 (+ 64) (+ 36)
    __host__ __device__ size_t fixed_bytes() const { return bytes(0); }              // 12 K (+ 4 096)
    // the fixed bytes the tile is chosen for: a tile does not depend on K (fixed_bytes() <= reserve_bytes() for every K <= kMaxProbes)
    __host__ __device__ size_t reserve_bytes() const { return kTileReserve + 4 * stage(); }
};

// simon_fetch_headroom (neither flag), simon_fetch_headroom_gpu (`devices`: the device bound, g complete) and simon_fetch_headroom_local
// (`storage`: the storage bound, l complete or l.flags null; with `devices` all three bounds).  a.tile from usage_tile(N, lds.node_bytes(),
// lds.reserve_bytes(), forced) of HeadroomLds lds{a.nrows, h.K, devices, storage}.
hipError_t launch_headroom(const UsageCommon& a, const HeadroomArgs& h, const DevUsage& g, const LocalUsage& l, bool devices, bool storage, int S,
                           hipStream_t st);

}  // namespace simon

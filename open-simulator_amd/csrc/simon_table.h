// simon_table.h -- host/device interface of simon_table.hip (generations 4 to 6 of the cpu+memory scenario kernel:
// one wave per scenario over a (signature, node) byte table, class term folded into the block summaries; 5: two-level
// summary; 6: + Open-Gpu-Share and node-level anti-affinity as per-block position masks).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simon_device.h"

namespace simon {

struct SigRow {      // one pod request signature (48 B)
    double req_c, req_m;   // computePodResourceRequest (fit.go:148-165), gcd-normalised, exact
    double nz_c, nz_m;     // non-zero request (V/framework/types.go:601-636)
    int32_t cls;           // pod class: row of static_mask / simon_raw
    uint32_t flags;        // bit0: all-zero request (fit.go:244-249)
    int32_t pad[2];        // GPU fold (TableScalars::static_tables & kStGpuFold): gpu-mem per device in gcd units, devices requested (0: not a GPU signature; -1: a GPU request for no device)
};
static_assert(sizeof(SigRow) == 48, "SigRow must be 48 bytes");

struct ShapeRow {    // capacity of one internal node class = one distinct (Allocatable.MilliCPU, Allocatable.Memory) pair (48 B)
    double cap_c, cap_m;
    double rc_c, rc_m;         // RN(1/cap)
    double rc100_c, rc100_m;   // RN(100 * rc)
};
static_assert(sizeof(ShapeRow) == 48, "ShapeRow must be 48 bytes");

// 16 B: signature | table class << 10, preset (>= 0) or pinned (<= -2: -2 - node) node, gate, and (REST) GPU request + 1 | extra-resource
// request + 1 << 6 | entries << 12 | offset << 18 of the pod's entries in TableCold::xrows (0 = the score table alone decides the pod)
struct PodRowC { int32_t sigcls, preset, gate, rest; };

// bits of TableScalars::static_tables
enum TableStatic : int32_t {
    kStNa = 1,           // TableCold::na_raw present (NodeAffinity preferred terms)
    kStTt = 2,           // TableCold::tt_raw present (TaintToleration PreferNoSchedule)
    kStAdd = 4,          // TableCold::add_raw present (already weighted additions)
    kStGpuSlices = 8,    // record TableCold::gpu_slices
    kStTwins = 16,       // signature k + 64 is a twin of k (same request)
    kStFold = 32,        // TableCold::foldx present (required anti-affinity / host ports on node-level keys folded into the table)
    kStSpreadAff = 64,   // the SPREAD && AFF instantiations (preferred pod (anti-)affinity / hard zone constraints in spread_select)
    kStGpuFold = 128,    // Open-Gpu-Share folded into the table (SigRow::pad = GPU request, devices per position behind the workspace)
    kStImg = 256,        // TableCold::img present (ImageLocality)
    kStSegments = 512,   // segmented batch (TableCold::scls, ranked instantiations only)
    kStPodSets = 1024,   // pod-subset batch (simon_set_scenario_pods): TableCold::pod_present decides, next to the gate, which pods a scenario holds
    kStOneSize = 2048,   // env SIMON_NO_SIZE_DISPATCH: every scenario takes the launch's entries-per-lane, also where its kernel holds a body for fewer (table_kernel: LO)
    kStClassTerms = kStNa | kStTt | kStAdd | kStImg,   // any static score table next to the Simon raw scores in the class term
};

struct TableScalars {
    int32_t mask_words, Cn, Cp, P, S, K;
    int32_t rk_stride;   // 0: cls_list = the pool's per-class node lists; N: per-scenario lists in rank order (simon_set_node_ranks)
    int32_t static_tables;   // TableStatic bits
    int32_t NZ;          // REST: topology keys that are NOT node-level (a term on one marks every position of the pod's domain)
    int32_t M, G, X;     // REST: rows of the per-block position masks (G GPU requests + X extra-resource requests + 2 x terms)
    int32_t TH, TZ, NZK; // SPREAD: hostname-key term rows, zone-key term rows, zone-like topology keys (class split)
    int32_t ni_max;      // padded (class-major) scenario size bound of this launch (multiple of 16, <= 4096; coarse: of 64, <= 8192)
    uint64_t g_cpu, g_mem;
};

// pointers only the prologue, the epilogue and the rare paths (preset / pinned pods) use: one device-resident struct
struct TableCold {
    const int32_t *ncls, *rank, *cls_off, *clsprefix, *a_pods; const uint32_t *i_rq_cpu, *i_rq_mem, *i_nz_cpu, *i_nz_mem;
    const int32_t* i_npods; const SigRow* sigs; const ShapeRow* shapes; const ScenarioDesc* scen; const uint64_t* static_mask;
    const int32_t* simon_raw; int32_t* unscheduled; int64_t *used_cpu, *used_mem;
    // static score tables by (table class, internal node class), null when the plugin scores every node alike:
    // NodeAffinity preferred terms, TaintToleration PreferNoSchedule, already weighted additions (include/simon_hip.h, ABI v2)
    const int32_t *na_raw, *tt_raw, *add_raw;
    unsigned long long* prof;   // [S][12] phase ticks (builds with -DSIMON_TABLE_PROFILE and env SIMON_TABLE_PROF), else null
    // per-scenario node order (simon_set_node_ranks), [S][N] each: a node's index inside its class in rank order, the rank itself
    // (canonical index of ties); the per-class node lists in rank order (class segments at cls_off, first clsprefix[n][d]
    // entries valid) replace TableLaunch::cls_list
    const int32_t *rk_pos, *rk_rank;    // (the lists themselves travel as TableLaunch::cls_list)
    int32_t N;
    // REST (Open-Gpu-Share + required anti-affinity on node-level topology keys): mask rows per term class; GPU signatures (gpu-mem per device in gcd units, device count); the pool's devices
    const int32_t* xrows;           // per term class, <= 63 entries: mask row that must be clear | mask row the pod sets << 16 | (zone key + 1) << 28
    const uint2* gsig;              // [G]
    // extra resources = ephemeral storage (gcd units) + SIMON_MAX_SCALAR extended resources: requests [X][8], the pool's
    // allocatable and Requested at the start [N][8] (component 0 = ephemeral storage, 1.. = extended resources)
    const uint32_t *xsig, *xalloc, *i_xused;
    const int32_t* zdom;            // [NZ][N] domain of a node under a zone-like key (-1: no label)
    unsigned long long* gpu_slices; // [S][P] by pod id: devices Reserve booked (simon_batch_out.gpu_slices), written when TableScalars::static_tables & kStGpuSlices
    // SPREAD (soft PodTopologySpread constraints, generation 7): per pod class [soft constraints..., counted terms...] in sp_ent
    // (soft: term slot | maxSkew << 16 | SIMON_SPREAD_DUP_KEY bit 30; counted: term slot | multiplicity << 16), each with its term's
    // row: kind (1 hostname-like row, 2 zone-like row) | row << 2 | zone key slot << 16 | (node set + 1) << 19; Go's math.Log table;
    // node sets; zone domain of a class
    const uint32_t* foldx;          // [K][ceil(K / 32)] (TableScalars::static_tables & kStFold): bit S of row L = a pod of signature L on a node excludes signature S from it
    const int2* sp_ent;             // x = the entry, y = its term's row (kind | row << 2 | zone key slot << 16 | (node set + 1) << 19)
    const double* spread_log;       // [N + 1] math.Log(float64(i + 2)) (simon_class_tables.spread_log)
    const uint64_t* node_sets;      // [R][set_words]
    int32_t set_words;
    const signed char* cls_zdom;    // [NZK][Cn] domain of an internal node class under zone key slot z (-1: the label is missing)
    const int32_t* gpu_cnt;         // [N]
    const uint32_t *gpu_devtot, *i_gused;   // [N] per-device total, [N][8] used at the start (gcd units)
    // REST && SPREAD in one instantiation (round 6): PodRowC::rest keeps the REST descriptor (per pod: its GPU request is part of it), the
    // SPREAD descriptor travels here, by pod id
    const int32_t* sp_word;         // [P]
    // ImageLocality (ABI v7, TableScalars::static_tables & kStImg): img[img_slot[s] * img_stride + table class * Cn + internal node class],
    // 0..100, added to the class term next to add_raw
    const unsigned char* img;
    const int32_t* img_slot;        // [S] size slot of a scenario
    int32_t img_stride;             // table classes x internal node classes
    // segmented batch (simon_set_scenario_segments, TableScalars::static_tables & kStSegments): [S][Cn] nodes of class d that scenario s holds
    const int32_t* scls;
    // Shared initial image (table_image_kernel, round 8): the table, node state and block summaries of the batch's LARGEST scenario before any pod is placed,
    // written once per run; a prefix scenario copies its blocks instead of evaluating them (table_kernel: kSharedPro).  Null: every scenario evaluates its own.
    unsigned char* pro_image;       // TableImage layout
    const int32_t* pro_seg;         // [Cn + 1] first position of a class segment in the image (classes padded to 16)
    int32_t pro_nb, pro_n;          // blocks of 16 positions in the image; node count of the scenario it holds
    // pod-subset batch (simon_set_scenario_pods, TableScalars::static_tables & kStPodSets): [S][pp_words], pod p = bit (p & 31) of word p >> 5
    const uint32_t* pod_present;
    int32_t pp_words;
};

// Byte offsets inside the shared initial image of `nb` blocks: tile [nb][K][16] bytes, state [nb * 16] x 12 B, (when NonZeroRequested differs from
// Requested) nz [nb * 16] x 8 B, and per (block, signature) a u32: summary entry (best byte << 4 | 15 - position, class term 0) | feasible bytes << 16
struct TableImage { unsigned tile, state, nz, sc, total; };
__host__ __device__ inline TableImage table_image_of(int K, int nb, bool nzeq) {
    auto al = [](unsigned x) { return (x + 127u) & ~127u; };
    TableImage t;
    unsigned o = 0;
    t.tile = o; o += al((unsigned)nb * (unsigned)K * 16u);
    t.state = o; o += al((unsigned)nb * 16u * 12u);
    t.nz = o; o += nzeq ? 0u : al((unsigned)nb * 16u * 8u);
    t.sc = o; o += al((unsigned)nb * (unsigned)K * 4u);
    t.total = o;
    return t;
}

struct TableLaunch {
    const TableCold* cold;      // device pointer
    const int32_t* cls_list; const PodRowC* pods; const int32_t* orders; const int32_t* perm; int32_t* place_step;
    const unsigned long long* ws_off;   // [n_blocks] byte offset of a workgroup's slice of ws (table_ws_bytes of its own scenario)
    unsigned char* ws;   // HBM workspace: byte table + node state (+ per-16 summary entries and counters when coarse) of every scenario
    int team;            // waves per scenario: 0 / 1 = one (the throughput shape); kTeamWaves = team mode (SPREAD only; small batches)
    bool spread;         // some pod class carries soft spread constraints (generation 7; implies coarse; together with rest: simon_table_rs.hip)
    bool aff;            // some pod class carries required-affinity entries (REST)
    bool rest;           // some pods need the per-node filters of the REST path (implies coarse)
    bool coarse;         // two-level summary: LDS entries cover 64 positions, per-16 entries live in the workspace (tcarve)
    bool lds_x;          // generation 6 with its mask rows, row totals and the canonical index of every position in LDS (table_kernel: LDSX; batches resident at once)
    bool nzeq;           // NonZero == request for every pod and node (the Z instantiations)
    bool has_pin;        // some pod is pinned to a node (HAS_PIN; the REST, SPREAD and LDS-resident units know pinned pods anyway)
    bool lds_ws;         // generation 4 with the scenario's workspace in LDS (table_kernel: LDSWS; small batches of small problems): the dynamic LDS of the launch = summaries + the largest workspace
    TableScalars sc;
};

constexpr int kTableMaxNodes = 4095;    // canonical index and padded position are 12-bit fields of the arg-max keys
constexpr int kTableMaxNodesCoarse = 8191;    // ... 13-bit fields with the two-level summary
constexpr int kTableMaxPadded = 4096;   // class-major padded positions of one scenario (classes padded to 16)
constexpr int kTableMaxPaddedCoarse = 8192;   // ... with the two-level summary (classes padded to 64)
constexpr int kTableMaxSigs = 1023;     // two signatures per lane in registers + further groups of 128 read from TableCold::sigs per cycle (two with group 0's
                                        // round trip, the rest one each); 10 bits of the pod row name the signature
constexpr int kTableFastSigs = 384;     // ... the signatures whose rows travel in ONE round trip per cycle
constexpr size_t kTableLdsPerCU = 160 * 1024;
constexpr int kTableMaxGpuSigs = 32;    // distinct (gpu-mem, gpu-count) requests: one mask row and one lane each
constexpr int kTableMaxXres = 32;       // distinct (ephemeral-storage, extended-resource) requests: one mask row and one lane each
constexpr int kTableMaxTerms = 120;     // node-level anti-affinity terms: two mask rows each
constexpr int kSpreadMaxZoneDom = 16;    // domains of a zone-like key of a soft spread constraint (one u32 counter each)
constexpr int kSpreadMaxHostTerms = 4096, kSpreadMaxZoneTerms = 1024, kSpreadMaxZoneKeys = 3;
#ifndef SIMON_SPREAD_TAB_MAX
#define SIMON_SPREAD_TAB_MAX 512          // (tests build a library with a tiny table to drive every pod through the general walk)
#endif
constexpr int kSpreadTabMax = SIMON_SPREAD_TAB_MAX;       // entries of spread_select's per-pod score table in LDS: classes x (largest counter + 1, a power of two)
#ifndef SIMON_SPREAD_TAB_MAX2
#define SIMON_SPREAD_TAB_MAX2 2048
#endif
constexpr int kSpreadTabMax2 = SIMON_SPREAD_TAB_MAX2;    // ... of the instantiations for 65 .. 128 node classes (table_kernel: CN2)
constexpr int kTeamWaves = 4;           // team mode (table_kernel: NW): waves per scenario, one per SIMD of the CU.  8 and 16 were built and measured
                                        // SLOWER on every batch (profiles/r04/r04b_*: once the walks are a quarter, the leader's chain and the barriers decide)
constexpr int kTeamWavesMax = 16;       // (the exchange slots are sized for it: a wider team is one more translation unit, simon_table_team<N>.hip)
constexpr int kTableMaxClasses = 64;    // internal node classes = distinct (column content, allocatable) pairs: one lane each in the REST select and the SPREAD walks
constexpr int kTableMaxClassesSpread = 128;  // ... two per lane in the REST select and in the SPREAD walks that score soft constraints only (CN2, round 6)
constexpr int kTableMaxClassesPlain = 256;   // ... up to four per lane where only the prologue and the class terms' re-base are lane-shaped (no REST rows, no SPREAD; 129 .. 256: end of round 6)

// bits of table_lds_bytes' nzk next to the zone-key count: spread_select's second score table, team mode, CN2's larger score table
constexpr int kLdsSecondTable = 0x100, kLdsTeam = 0x200, kLdsCn2 = 0x400;
size_t table_lds_bytes(int K, int ni_max, int Cn, bool coarse, bool rest, int nzk = -1);   // LDS per workgroup for padded scenario sizes up to ni_max (nzk >= 0: SPREAD, the zone-key count | kLds* bits)
size_t table_ws_bytes(int K, int ni, bool nzeq, bool coarse, int Cn, int M, int NZ, int TH = 0, int TZ = 0);  // HBM workspace of ONE scenario with ni padded positions
// launches n_blocks scenarios (one workgroup of 64 * max(team, 1) threads each), scenario of block b = a.perm[b], on the translation unit that
// serves the launch (simon_table.hip: table_route)
hipError_t launch_table(const TableLaunch& a, int n_blocks, size_t lds_bytes, hipStream_t st);
const char* table_unit_name(const TableLaunch& a);   // the unit launch_table sends `a` to, by file name (SIMON_DEBUG_ROUTE)
int table_entries_per_lane(const TableLaunch& a);    // summary entries per lane of the kernel launch_table picks (NBQ), from the batch's largest scenario
// The smaller entries-per-lane the same kernel also serves, each scenario by its own padded size (table_kernel: LO); 0: none.  A scenario takes it iff
// its padded size is at most 64 x 16 x that many positions, unless TableScalars::static_tables holds kStOneSize.
int table_entries_own_size(const TableLaunch& a);
// Does the kernel re-base a summary row's class terms at the event -- in the cycle that empties a node class for the row's signature -- (true) or at the
// row's next use (false: the two-level layout -- so the REST, SPREAD and team units and more than 128 signatures --, more than 128 node classes)?
bool table_rebase_at_event(const TableLaunch& a);
// Can the launch take its initial table from the shared image (a.cold's pro_image)?  The one-level instantiations of simon_table.hip on prefix scenarios in
// canonical order: neither ranked nor segmented.  launch_table_image fills the image (the batch's largest scenario, `nb` blocks) on `st`, ahead of launch_table.
bool table_shared_prologue(const TableLaunch& a);
hipError_t launch_table_image(const TableLaunch& a, int nb, hipStream_t st);
inline size_t table_ldsx_bytes(int ni_max, int M) {   // rows [M][ni_max / 16] u16, row totals [M] u32, canonical indices [ni_max] u16 (each rounded up to 128 bytes)
    return ((((size_t)(ni_max >> 4) * M * 2) + 127) & ~(size_t)127) + (((size_t)M * 4 + 127) & ~(size_t)127) + (((size_t)ni_max * 2 + 127) & ~(size_t)127);
}
// placement[s][pod] = place_step[s][inverse order of s][pod]: the kernel records placements by scheduling STEP (coalesced)
hipError_t launch_unpermute(const int32_t* place_step, const int32_t* inv_orders, const ScenarioDesc* scen, int S, int P,
                            int32_t* placement, hipStream_t st);

}  // namespace simon

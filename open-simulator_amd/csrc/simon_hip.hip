// simon_hip.hip -- C-ABI of libsimon_hip.so (include/simon_hip.h): context, input staging into
// HBM (SoA), kernel-variant selection, launches, result fetch, min-plan reduction.
//
// Data layout in HBM (one copy per context, shared by every scenario of a batch):
//   nodes   NARROW: a_cpu/a_mem u32 (gcd-normalised), a_pods/ncls i32, initial state u32/i32
//           WIDE:   the int64 arrays of simon_nodes_soa as they come
//   pods    PodRowN[P] (32 B rows, read through scalar loads) / WidePod[P]
//   orders  int32 [n_orders][P];  scenarios {n_nodes, order_id}[S];  perm[S] (LPT launch order)
//   tables  simon_raw as i32/i64 [Cp][Cn]; static_mask u64 [Cp][ceil(N/64)]
//   out     unscheduled i32[S], used_cpu/used_mem i64[S], placement i32[S][P] (optional)
#include "../../include/simon_hip.h"
#include "simon_device.h"
#include "simon_wide.h"
#include "simon_table.h"
#include "simon_subset.h"
#include "simon_podsets.h"
#include "simon_orders.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <numeric>
#include <set>
#include <tuple>
#include <string>
#include <vector>

namespace simon {
struct PodRowF { double req_c, req_m, nz_c, nz_m; int32_t cls, preset, gate; uint32_t flags; };
struct FastScalars { int32_t mask_words, Cn, Cp, P, S; uint64_t g_cpu, g_mem; const uint32_t* pod_present; int32_t pp_words; };
struct FastLaunch {
    const uint32_t *a_cpu, *a_mem; const int32_t *a_pods, *ncls; const uint32_t *i_rq_cpu, *i_rq_mem, *i_nz_cpu, *i_nz_mem;
    const int32_t* i_npods; const PodRowF* pods; const int32_t* orders; const ScenarioDesc* scen; const int32_t* perm;
    const uint64_t* static_mask; const int32_t* simon_raw; int32_t* unscheduled; int64_t *used_cpu, *used_mem;
    int32_t* placement; FastScalars sc;
};
hipError_t launch_fast(const FastLaunch& a, int T, int slots, bool has_mask, bool nzeq, size_t lds_bytes, hipStream_t st);
hipError_t launch_narrow(const NarrowArgs& a, int T, int slots, bool has_mask, bool rcp_div, size_t lds_bytes,
                         hipStream_t st);
}  // namespace simon

using namespace simon;

namespace {

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = std::max<size_t>(count, 1);
        return e;
    }
    hipError_t upload(const std::vector<T>& h, hipStream_t st) {
        hipError_t e = ensure(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

struct PlanKernelOut {
    unsigned long long key;  // (n_nodes << 32) | scenario, min-reduced; ~0 = none
};

}  // namespace

constexpr int kPlanRecWords = 4;     // simon_ctx::d_plan: plan key, used cpu, used memory, used VG of the winner

struct simon_ctx : simon::HostInputs {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // host copies of the inputs live in the HostInputs base (caller buffers are never retained)
    bool have_nodes = false, have_pods = false, have_tables = false, staged = false, wide_staged = false;
    // ---- variant decision ----
    int variant = 0;
    uint64_t g_cpu = 1, g_mem = 1;
    bool rcp_div = true;
    int force_T = 0;  // env SIMON_WG
    bool force_v1 = false;  // env SIMON_NARROW_V1: use simon_narrow.hip even when simon_fast.hip applies
    bool force_wide = false;  // env SIMON_FORCE_WIDE
    int n_cus = 256;          // compute units of the device (simon_ctx_create)
    size_t lds_pad = 0;       // env SIMON_CACHE_LDS_PAD (bytes): occupancy experiment knob -- extra LDS per workgroup
    // ---- device buffers ----
    DevBuf<uint32_t> d_a_cpu, d_a_mem, d_i_rq_cpu, d_i_rq_mem, d_i_nz_cpu, d_i_nz_mem;
    DevBuf<int32_t> d_a_pods, d_ncls, d_i_npods, d_raw32;
    DevBuf<PodRowN> d_podsN;
    DevBuf<PodRowF> d_podsF;
    bool fast_ok = false, nzeq = false;  // simon_fast.hip eligibility
    // ---- simon_table.hip (score table, one wave per scenario) ----
    bool table_ok = false, table_perm_ok = false, no_cache = false;  // no_cache: env SIMON_NO_CACHE (run generation 2 instead)
    DevBuf<unsigned char> d_ws, d_table_cold;
    DevBuf<unsigned long long> d_table_prof, d_ws_off;
    int n_sigs = 0, Cn_t = 0;                    // request signatures; internal node classes = distinct (node_class, allocatable) pairs
    DevBuf<SigRow> d_sigs;
    DevBuf<ShapeRow> d_shapes;                   // [Cn_t]: capacity + reciprocals of an internal class
    DevBuf<PodRowC> d_podsC;
    DevBuf<int32_t> d_t_ncls, d_rank, d_clsprefix, d_inv_orders, d_place_step, d_cls_list, d_cls_off, d_t_raw;
    std::vector<int32_t> h_clsprefix, scen_ni;   // [(N+1)][Cn_t]; padded (class-major) size of every loaded scenario
    size_t ws_total = 0;
    // shared initial image of the score-table kernel (simon_table.h: TableImage): sized by table_layout next to ws_total, filled in every run
    DevBuf<unsigned char> d_pro_image;
    DevBuf<int32_t> d_pro_seg;
    size_t pro_bytes = 0;
    int pro_nb = 0;
    bool no_shared_prologue = false;              // env SIMON_NO_SHARED_PROLOGUE: every scenario evaluates its own initial table (A/B + tests)
    bool no_size_dispatch = false;                // env SIMON_NO_SIZE_DISPATCH: every scenario scans the launch's entries-per-lane, not its own size's (A/B + tests)
    // REST path of the score-table kernel (Open-Gpu-Share + node-level required anti-affinity): decided by choose_variant
    std::vector<int32_t> h_ncls_t, h_cls_off;    // internal node class of every node; class offsets into the per-class node lists
    DevBuf<int32_t> d_rk_ids, d_rk_pos;          // per-scenario node order for the score-table kernel (simon_set_node_ranks)
    bool table_ranks_ok = false;
    bool has_static = false;                     // static score tables present (score-table kernel: class term; else all-feature kernel)
    DevBuf<int32_t> d_t_na, d_t_tt, d_t_add;
    bool raw_fits_lds = true;                    // generations 1 / 2 can run (else: score table or the all-feature kernel)
    bool no_gpu_split = false, force_table = false, no_class_content = false, no_gpu_fold = false;
    bool debug_route = false;                     // env SIMON_DEBUG_ROUTE: one line per run on stderr with what decided the kernel
    bool gfold = false;                           // Open-Gpu-Share folded into the score table: the GPU request is part of the signature (gfold_supported)
    bool table_prof = false;                     // env SIMON_TABLE_PROF in -DSIMON_TABLE_PROFILE builds
    bool rest = false, no_rest = false;          // no_rest: env SIMON_NO_REST (such problems take the all-feature kernel)
    // fold: required anti-affinity / host ports on node-level topology keys as MONOTONE INFEASIBILITY of the score table -- a pod that
    // lands on a node zeroes the node's byte of every signature it excludes there, for good (fold_supported); env SIMON_NO_FOLD
    bool fold = false, no_fold = false;
    int fold_sigs = 0;                            // upper bound of the signatures the fold needs
    int gfold_sigs = 0, gfold_base_sigs = 0;      // ... and the GPU fold (request shape x table class x filter class x GPU request); the same without the GPU request
    std::vector<int32_t> fold_fc;                 // [Cp] filter class of a pod class
    std::vector<uint8_t> fold_x;                  // [FC][FC]: a pod of filter class L on a node excludes filter class S from it
    int fold_FC = 0;
    DevBuf<uint32_t> d_foldx;                     // [K][ceil(K / 32)]: bit S of row L = signature L landing excludes signature S
    uint64_t g_gpu = 1, g_eph = 1;               // gcd of every GPU memory / ephemeral-storage quantity
    uint64_t gfold_g = 1;                        // the GPU fold's own gcd: rest_supported() is also called as a PROBE and resets g_gpu
    std::vector<int> zone_keys;                  // topology keys of terms that are not node-level (REST: a domain = many positions)
    std::vector<int> key_zslot;                  // [Kt] index into zone_keys or -1 (node-level / unused)
    DevBuf<int32_t> d_zdom;
    bool xres = false;                           // some pod requests ephemeral storage or an extended resource
    int rest_M = 0, rest_G = 0, rest_X = 0;      // mask rows; GPU requests; extra-resource requests
    DevBuf<uint32_t> d_xsig, d_xalloc, d_i_xused;
    DevBuf<int32_t> d_xrows, d_gpu_cnt;
    DevBuf<uint32_t> d_gpu_devtot, d_i_gused;
    DevBuf<uint2> d_gsig;
    // SPREAD path of the score-table kernel (soft PodTopologySpread constraints, generation 7): decided by choose_variant
    bool sig_twins = false, no_sig_twins = false; // upper-half signatures sit 64 slots above a twin (same request, other table class); env SIMON_TABLE_NO_TWINS
    // InterPodAffinity preferred terms in self-referential form, scored in spread_select's table (spread_supported); env SIMON_NO_IPA_FOLD
    bool hard_fold = false, no_hard_fold = false; // hard spread constraints on zone-like keys as per-class verdicts of spread_select; env SIMON_NO_HARD_FOLD
    bool ipa_fold = false, no_ipa_fold = false;
    bool no_cn2 = false;                          // env SIMON_NO_CN2: generation 7 stays at 64 node classes (A/B + tests)
    // REST && SPREAD (round 6, simon_table_rs.hip): soft spread constraints next to GPU requests / required anti-affinity / ports / extra
    // resources that do not fold into the table -- generation 7's walks over generation 6's position-mask rows.  rs_probe: spread_supported
    // called to answer "would the walks take it if the rows carried the filters"; env SIMON_NO_RS: never (A/B + tests)
    bool rs = false, rs_probe = false, no_rs = false;
    DevBuf<int32_t> d_sp_word;                   // [P] SPREAD descriptor by pod id (TableCold::sp_word)
    std::vector<int32_t> ipa_h_term, ipa_h_w;     // [Cp] the hostname-like term of a class's raw score (-1: none) and its coefficient
    std::vector<std::vector<std::pair<int32_t, int32_t>>> ipa_z;   // [Cp] (zone-like term, coefficient)
    bool spread = false, no_spread = false;      // no_spread: env SIMON_NO_SPREAD (such problems take the all-feature kernel)
    // team mode of generation 7 (simon_table.hip: NW = kTeamWaves waves per scenario): env SIMON_TEAM = 0 never / 1 (or 4) always /
    // unset: batches of at most team_max_s scenarios (default 2 per CU: beyond that one wave per scenario fills the SIMDs by
    // itself -- measured crossover between 512 and 1 024 scenarios, profiles/r04; env SIMON_TEAM_MAX_S)
    int team_mode = -1, team_max_s = -1;
    int ldsws_mode = -1;                         // env SIMON_LDS_WS = 0 never / 1 whenever it fits / unset: batches of at most one scenario per CU (simon_table.hip: LDSWS)
    std::vector<int> sp_kind, sp_row, sp_zslot;  // per term: 0 unused / 1 hostname-like / 2 zone-like; its counter row; zone key slot
    std::vector<int> sp_set_eff;                  // per id: the node set its row is counted on (-1: every node)
    std::vector<int> sp_rep;                      // per term: the first term with the same key, node set and matching classes (they share a counter row)
    std::vector<int> sp_zkeys;                   // topology keys of the zone-like soft terms (<= kSpreadMaxZoneKeys): the class split
    int sp_TH = 0, sp_TZ = 0;
    DevBuf<int32_t> d_sp_ent;                    // (entry, term row) pairs: TableCold::sp_ent
    DevBuf<double> d_spread_log;
    DevBuf<uint64_t> d_node_sets;
    DevBuf<signed char> d_cls_zdom;
    bool table_coarse = false;                   // two-level summary (simon_table.hip: COARSE), decided per loaded batch
    int force_coarse = -1, table_ni_top = 16;    // env SIMON_TABLE_COARSE = 0 / 1 (A/B)
    std::vector<int32_t> h_perm;
    std::vector<int64_t> explain_detail;   // [failed][n][4] of the last explain (Open-Local error sizes), simon_explain_local_detail
    int explain_nodes = 0;
    bool explain_ran = false;
    DevBuf<uint64_t> d_mask, d_t_mask;           // static masks by pod class; by table class (simon_table.hip)
    DevBuf<int64_t> d_prefix_cpu, d_prefix_mem, d_prefix_vg;
    DevBuf<int32_t> d_node_rank, d_node_inv;      // [S][N] per-scenario nodeTree ranks (simon_set_node_ranks)
    bool has_ranks = false;
    // segmented batch (simon_set_scenario_segments): fixed nodes [0, seg_start[0]) + the first seg_count[s][g] nodes of every segment g.
    // Implies per-scenario ranks (absent nodes rank N) and per-scenario class lists; h_scls [S][Cn_t] = nodes of class d scenario s holds;
    // seg_tot [3][S] = its allocatable cpu / memory and VG capacity (satisfyResourceSetting over its own nodes)
    int seg_n = 0;
    std::vector<int32_t> seg_start, seg_count, seg_of, h_scls;
    std::vector<int64_t> seg_tot;
    DevBuf<int32_t> d_scls;
    DevBuf<int64_t> d_seg_tot;
    // node-subset batch (simon_set_scenario_nodes): scenario s holds exactly the pool nodes whose bit is set in sub_words[s][sub_W] (node j =
    // bit j & 31 of word j >> 5).  Rides on the segmented batch's kernel path (ranks, h_scls, seg_tot); a context holds one kind at a time.
    // sub_zone [N]: nodeTree zone ids (empty: one zone).  subset_host: env SIMON_SUBSET_STAGE=host -- the arrays from host loops (A/B + tests)
    bool sub_on = false, subset_host = false;
    // simon_set_own_nodes_all_feature: a segmented / node-subset batch that routes to the all-feature kernel runs there (its own-nodes run
    // forms, simon_wide_own.hip) instead of being refused.  A context option: off by default, survives every load.
    bool own_wide = false;
    int sub_W = 0;
    std::vector<uint32_t> sub_words;
    std::vector<int32_t> sub_zone;
    DevBuf<uint32_t> d_sub_words;
    DevBuf<int32_t> d_sub_zone;
    // simon_set_pod_eviction: p_evict [P] (empty: none) flags preset pods that a node-subset scenario without their node schedules like
    // any other pod.  evict_short: a flagged pod whose node the loaded PREFIX batch lacks (-1: none) -- such a batch waits for its node rows
    std::vector<uint8_t> p_evict;
    int evict_short = -1;
    // pod-subset batch (simon_set_scenario_pods): scenario s holds pod p iff bit p & 31 of pod_words[s][pod_W] word p >> 5 (by pod id); the
    // words go to the device as given.  Orthogonal to the node dimension: survives ranks, segments and node subsets; cleared by
    // simon_load_scenarios and simon_load_pods.  d_pod_group / d_grp_*: simon_fetch_group_counts' staging
    bool pods_on = false;
    int pod_W = 0;
    DevBuf<uint32_t> d_pod_words;
    DevBuf<int32_t> d_pod_group, d_grp_uns, d_grp_placed;
    // simon_load_scenarios_composed: the presence words of the live entries of every ORDER [n_orders][pod_W], which the pod rows expand by
    // scenario; order_rows_on while those rows are the installed ones (simon_fetch_orders reports them).  order_host: env
    // SIMON_ORDER_STAGE=host -- orders, inverse orders and words from host loops (A/B + tests)
    DevBuf<uint32_t> d_order_words;
    bool order_rows_on = false, order_host = false;
    // simon_fetch_node_usage / simon_fetch_headroom: compact int64 copies of the pod requests and the node rows ([kUsageRows][P] / [N]),
    // uploaded on the first call after simon_load_pods / simon_load_nodes; usage_rows: bit r = some pod requests resource row r (cpu and
    // memory always), the rows the kernels accumulate.  usage_tile: env SIMON_USAGE_TILE (nodes per LDS tile; 0 = from the LDS budget)
    bool usage_pods_staged = false, usage_nodes_staged = false;
    uint32_t usage_rows = 3;
    int usage_tile = 0;
    DevBuf<int64_t> d_u_pod_req, d_u_node_init, d_u_node_alloc, d_u_out64, d_u_fit;
    DevBuf<int32_t> d_u_init_npods, d_u_alloc_pods, d_u_ids, d_u_npods, d_u_fit_nodes;
    DevBuf<ProbeRow> d_u_probes;
    DevBuf<uint64_t> d_u_probe_mask;
    // simon_fetch_gpu_usage / simon_fetch_headroom_gpu: the GPU-share arrays the kernels read, staged likewise (gpu_mem [P]; devices per
    // node, bytes per device [N] and the state before the stream [N][8]); the probes' device requests per call
    bool usage_gpu_pods_staged = false, usage_gpu_nodes_staged = false;
    DevBuf<int64_t> d_g_pod_mem, d_g_per_dev, d_g_init_used, d_g_out_used, d_g_probe_mem;
    DevBuf<int32_t> d_g_node_cnt, d_g_out_pods, d_g_probe_cnt;
    // simon_fetch_local_usage / simon_fetch_headroom_local: the Open-Local arrays the storage kernels read, staged likewise -- the node
    // arrays after simon_load_nodes; the specs, every pod's spec (-1: none, or bound by Spec.NodeName) and, per loaded order, the pods with
    // a spec in that order's sequence (local_list / local_list_off, from h_orders) after simon_load_pods, simon_load_class_tables or
    // simon_load_scenarios; the probes' specs per call
    bool local_nodes_staged = false, local_pods_staged = false;
    std::vector<int32_t> h_orders;                // [n_orders][P] the loaded orders
    DevBuf<LocalSpec> d_l_specs;
    DevBuf<int32_t> d_l_pod_spec, d_l_list, d_l_list_off, d_l_flags, d_l_vg_cnt, d_l_vg_name, d_l_dev_cnt, d_l_dev_media, d_l_dev_init, d_l_probe_spec, d_l_out_dev;
    DevBuf<int64_t> d_l_vg_cap, d_l_vg_init, d_l_dev_cap, d_l_out_vg;
    bool orders_perm = false;                     // every loaded order is a permutation of [0, P) (the score-table kernel's placement gather)
    std::vector<int64_t> prefix_cpu, prefix_mem;   // [N+1] allocatable of the first n nodes
    std::vector<int64_t> prefix_vg;   // [N+1] Open-Local VG capacity of the first n nodes (0 without local storage)
    WideDevice wide;
    // scenarios
    int S = 0, n_orders = 0, max_n = 0;
    std::vector<ScenarioDesc> scen;
    DevBuf<ScenarioDesc> d_scen;
    DevBuf<int32_t> d_orders, d_perm;
    // outputs
    DevBuf<int32_t> d_unsched, d_place;
    DevBuf<int32_t> d_prio;                       // ABI v6: spec.priority per pod (simon_set_pod_priorities)
    DevBuf<unsigned char> d_risk;                 // [S] DefaultPreemption could have acted in the scenario (simon_fetch_preempt_risk)
    bool prio_staged = false, have_risk = false;
    DevBuf<int64_t> d_used_cpu, d_used_mem, d_used_vg;
    DevBuf<unsigned long long> d_plan;           // kPlanRecWords: plan key, then the winner's used cpu / memory / VG (plan_record_kernel)
    bool have_results = false, have_placement = false, have_slices = false;
    DevBuf<uint64_t> d_gpu_slices;      // [S][P] devices Reserve booked (simon_batch_out.gpu_slices), recorded on request
    // ABI v7 ImageLocality: the caller's node classes and (pod class, node class) tables before the image split (img_refine)
    bool img_refined = false;
    int img_base_Cn = 0;
    std::vector<int32_t> img_base_ncls;
    std::vector<int64_t> img_base_raw, img_base_na, img_base_tt, img_base_add;
    DevBuf<unsigned char> d_t_img, d_img_explain;   // score table: [slot][table class][internal node class]; explain: [1][img_R][Cn]
    DevBuf<int32_t> d_img_slot;                     // [S] size slot of every loaded scenario
    int img_stride_t = 0;                           // table classes x internal node classes (TableCold::img_stride)
    std::vector<int32_t> h_img_slot;                // host sources of d_img_slot / d_img_explain: they outlive the asynchronous uploads
    std::vector<unsigned char> h_img_explain;
    // own-nodes image states (HostInputs::img_own_*): the table comes from image_states_kernel (simon_subset.hip), or, image_host (env
    // SIMON_IMAGE_STAGE=host), from a host loop.  img_state_cap: bytes of [T][img_R][Cn] a batch may ask for (env SIMON_IMAGE_STATE_MB).
    // img_orders: the loaded orders, kept for every image problem (the re-staging derives the inverse orders again).  h_tc_of / t_img_staged:
    // table class of every pod class while d_t_img is current (simon_fetch_image_scores)
    bool image_host = false, t_img_staged = false;
    size_t img_state_cap = (size_t)256 << 20;
    std::vector<int32_t> img_orders, h_tc_of;
    DevBuf<uint32_t> d_is_words;
    DevBuf<int32_t> d_is_i32, d_is_scratch;
    DevBuf<int64_t> d_is_size;
    DevBuf<unsigned char> d_is_out;
    simon_stats stats{};
};

namespace {

int fail(simon_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(c, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), e_ == hipErrorOutOfMemory ? SIMON_ENOMEM : SIMON_ENODEV, "%s: %s", \
                        #call, hipGetErrorString(e_));                                           \
    } while (0)

template <class T>
void copy_opt(std::vector<T>& dst, const T* src, size_t n, T fill = T()) {
    if (src) dst.assign(src, src + n);
    else dst.assign(n, fill);
}

uint64_t gcd_u64(uint64_t a, uint64_t b) { while (b) { uint64_t t = a % b; a = b; b = t; } return a; }

uint64_t gcd_of(std::initializer_list<const std::vector<int64_t>*> vs) {
    uint64_t g = 0;
    for (auto* v : vs) for (int64_t x : *v) { if (x < 0) return 0; g = gcd_u64(g, (uint64_t)x); if (g == 1) return 1; }
    return g ? g : 1;
}

// ---- ImageLocality (ABI v7: simon_set_image_locality) -----------------------------------------------------------------------------------
// ImageLocality.Score of pod class cp on pool node j in a cluster of n nodes (imagelocality/image_locality.go:53-125): plain IEEE fp64
// as Go evaluates it (-ffp-contract=off), int64 arithmetic for the rest
int img_score(const simon_ctx* c, int cp, int j, int n) {
    const int e0 = c->img_class_off[cp], e1 = c->img_class_off[cp + 1];
    if (e1 == e0 || n <= 0 || j < 0) return 0;
    const int64_t mb = 1024 * 1024, lo = 23 * mb, hi = 1000 * mb * (int64_t)(e1 - e0);
    int64_t sum = 0;
    for (int e = e0; e < e1; ++e) {
        const int im = c->img_class_image[e];
        if (im < 0) continue;
        for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q)
            if (c->img_node_image[q] == im) {
                sum += (int64_t)((double)c->img_size[im] * ((double)c->img_node_count[q] / (double)n));
                break;
            }
        if (sum > hi) sum = hi + 1;                  // (saturates: the clamp below takes it to hi whatever follows)
    }
    if (sum < lo) sum = lo; else if (sum > hi) sum = hi;
    return (int)(100 * (sum - lo) / (hi - lo));
}

// the caller's node classes and tables back (before a reload or a new image input)
void img_unrefine(simon_ctx* c) {
    if (!c->img_refined) return;
    c->Cn = c->img_base_Cn; c->node_class.swap(c->img_base_ncls);
    c->simon_raw.swap(c->img_base_raw); c->na_raw.swap(c->img_base_na); c->tt_raw.swap(c->img_base_tt); c->static_add.swap(c->img_base_add);
    c->img_base_ncls.clear(); c->img_base_raw.clear(); c->img_base_na.clear(); c->img_base_tt.clear(); c->img_base_add.clear();
    c->img_refined = false;
}

// One slot's scores: out[row][Cn] for a cluster of n nodes, from a node of every class (every node of a class scores alike)
void img_slot_scores(const simon_ctx* c, int n, uint8_t* out) {
    for (int cp = 0; cp < c->Cp; ++cp) {
        const int r = c->img_row_of[cp];
        if (r < 0) continue;
        for (int k = 0; k < c->Cn; ++k) out[(size_t)r * c->Cn + k] = (uint8_t)img_score(c, cp, c->img_rep[k], n);
    }
}

// The image-state table of an own-nodes batch in a host loop (SIMON_IMAGE_STAGE=host; image_states_kernel's A/B and fallback):
// addNodeImageStates over the slot's nodes in pool order, then img_score's arithmetic on the slot's own counts and sizes.
void img_own_scores_host(simon_ctx* c) {
    const int N = c->N, I = (int)c->img_size.size(), W = (N + 31) / 32;
    const size_t slot = (size_t)c->img_R * c->Cn;
    std::vector<int32_t> cnt(c->img_node_image.size()), run(I), first(I);
    for (int t = 0; t < c->img_own_T; ++t) {
        const uint32_t* row = c->img_own_words.data() + (size_t)t * W;
        auto in = [&](int j) { return (row[j >> 5] >> (j & 31)) & 1u; };
        std::fill(run.begin(), run.end(), 0); std::fill(first.begin(), first.end(), -1);
        for (int j = 0; j < N; ++j)
            for (int q = c->img_node_off[j]; in(j) && q < c->img_node_off[j + 1]; ++q) {
                const int im = c->img_node_image[q];
                cnt[q] = ++run[im];
                if (first[im] < 0) first[im] = q;
            }
        const int n = c->img_own_n[t];
        for (int cp = 0; cp < c->Cp; ++cp) {
            const int r = c->img_row_of[cp], e0 = c->img_class_off[cp], e1 = c->img_class_off[cp + 1];
            if (r < 0) continue;
            const int64_t mb = 1024 * 1024, lo = 23 * mb, hi = 1000 * mb * (int64_t)(e1 - e0);
            for (int k = 0; k < c->Cn; ++k) {
                const int j = c->img_rep[k];
                if (j < 0 || !in(j)) continue;                       // (an absent representative scores 0)
                int64_t sum = 0;
                for (int e = e0; e < e1; ++e) {
                    const int im = c->img_class_image[e];
                    if (im < 0) continue;
                    for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q)
                        if (c->img_node_image[q] == im) {
                            sum += (int64_t)((double)c->img_node_size[first[im]] * ((double)cnt[q] / (double)n));
                            break;
                        }
                    if (sum > hi) sum = hi + 1;
                }
                if (sum < lo) sum = lo; else if (sum > hi) sum = hi;
                c->img_cls[t * slot + (size_t)r * c->Cn + k] = (uint8_t)(100 * (sum - lo) / (hi - lo));
            }
        }
    }
}

// ... and on the device: the lister lists (a CSR by image, pool order) and the flat inputs go up in one int32 buffer, the table comes
// back into img_cls (stage_narrow / wide_stage lay it out for their kernels)
int img_own_scores_device(simon_ctx* c) {
    const int N = c->N, I = (int)c->img_size.size(), W = (N + 31) / 32, T = c->img_own_T, Cp = c->Cp;
    const size_t nnz = c->img_node_image.size();
    std::vector<int32_t> lis_off(I + 1, 0), lis_node(nnz), lis_ent(nnz), row_class(c->img_R);
    for (size_t q = 0; q < nnz; ++q) ++lis_off[c->img_node_image[q] + 1];
    for (int i = 0; i < I; ++i) lis_off[i + 1] += lis_off[i];
    {
        std::vector<int32_t> at(lis_off.begin(), lis_off.end() - 1);
        for (int j = 0; j < N; ++j)
            for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q) {
                const int k = at[c->img_node_image[q]]++;
                lis_node[k] = j; lis_ent[k] = q;
            }
    }
    for (int cp = 0; cp < Cp; ++cp) if (c->img_row_of[cp] >= 0) row_class[c->img_row_of[cp]] = cp;
    std::vector<int32_t> flat;
    size_t off[10];
    const std::vector<int32_t>* parts[10] = {&lis_off, &lis_node, &lis_ent, &c->img_node_off, &c->img_node_image, &c->img_class_off, &c->img_class_image, &row_class, &c->img_rep, &c->img_own_n};
    for (int k = 0; k < 10; ++k) { off[k] = flat.size(); flat.insert(flat.end(), parts[k]->begin(), parts[k]->end()); }
    const size_t out_bytes = (size_t)T * c->img_R * c->Cn;
    HIP_TRY(c, c->d_is_i32.upload(flat, c->stream));
    HIP_TRY(c, c->d_is_words.upload(c->img_own_words, c->stream));
    HIP_TRY(c, c->d_is_size.upload(c->img_node_size, c->stream));
    HIP_TRY(c, c->d_is_out.ensure(out_bytes));
    ImageStates a{};
    const int32_t* const b = c->d_is_i32.p;
    a.present = c->d_is_words.p; a.slot_n = b + off[9];
    a.lis_off = b + off[0]; a.lis_node = b + off[1]; a.lis_ent = b + off[2];
    a.node_size = c->d_is_size.p; a.node_off = b + off[3]; a.node_image = b + off[4];
    a.class_off = b + off[5]; a.class_image = b + off[6]; a.row_class = b + off[7]; a.rep = b + off[8];
    a.T = T; a.W = W; a.I = I; a.nnz = (int32_t)nnz; a.R = c->img_R; a.Cn = c->Cn;
    if ((nnz + I) * sizeof(int32_t) > kImageLdsBudget) {              // (decided by size, here: the counts of a slot in a global row)
        HIP_TRY(c, c->d_is_scratch.ensure((size_t)T * (nnz + I)));
        a.scratch = c->d_is_scratch.p;
    }
    a.out = c->d_is_out.p;
    HIP_TRY(c, launch_image_states(a, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->img_cls.data(), c->d_is_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

// Split the caller's node classes by image CONTENT -- (image, NumNodes) of every entry of the node -- so that the nodes of a class score
// alike for EVERY cluster size (simon_explain of a size outside the batch included), and derive the per-slot tables of the batch
// (img_sizes).  Classes of nodes without entries keep their ids: a problem whose nodes list nothing stages exactly as without images.
// Own-nodes form (img_own_T > 0): a node's NumNodes depends on which listers the scenario holds, so every node with an entry is a class
// of its own and the slots are the batch's image states; the score-table staging interns equal score columns again.
int img_refine(simon_ctx* c) {
    img_unrefine(c);
    c->img_row_of.assign(c->Cp, -1);
    c->img_R = 0; c->img_cls.clear(); c->img_rep.clear();
    if (!c->has_img) return SIMON_OK;
    for (int cp = 0; cp < c->Cp; ++cp)
        for (int e = c->img_class_off[cp]; e < c->img_class_off[cp + 1]; ++e)
            if (c->img_class_image[e] >= 0) { c->img_row_of[cp] = c->img_R++; break; }
    if (c->img_R == 0) return SIMON_OK;
    const int N = c->N, Cn0 = c->Cn;
    const bool own = c->img_own_T > 0;
    std::map<std::vector<int32_t>, int> ids;
    for (int k = 0; k < Cn0; ++k) ids.emplace(std::vector<int32_t>{k}, k);
    std::vector<int32_t> ncls(N), rep(Cn0, -1);
    for (int j = 0; j < N; ++j) {
        std::vector<std::pair<int32_t, int32_t>> ent;
        for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q) ent.emplace_back(c->img_node_image[q], c->img_node_count[q]);
        std::sort(ent.begin(), ent.end());
        std::vector<int32_t> key{c->node_class[j]};
        if (own && !ent.empty()) { key = {-1, j}; ent.clear(); }      // (its own pre-class)
        for (auto& e : ent) { key.push_back(e.first); key.push_back(e.second); }
        auto it = ids.emplace(std::move(key), (int)ids.size());
        if (it.second) rep.push_back(-1);
        ncls[j] = it.first->second;
        if (rep[ncls[j]] < 0) rep[ncls[j]] = j;
    }
    const int Cn1 = (int)ids.size();
    if (Cn1 != Cn0) {
        c->img_base_Cn = Cn0;
        c->img_base_ncls = c->node_class; c->img_base_raw = c->simon_raw; c->img_base_na = c->na_raw; c->img_base_tt = c->tt_raw; c->img_base_add = c->static_add;
        std::vector<int32_t> orig(Cn1);
        for (int k = 0; k < Cn1; ++k) orig[k] = k < Cn0 ? k : c->img_base_ncls[rep[k]];
        for (std::vector<int64_t>* tab : {&c->simon_raw, &c->na_raw, &c->tt_raw, &c->static_add}) {
            if (tab->empty()) continue;
            std::vector<int64_t> t((size_t)c->Cp * Cn1);
            for (int cp = 0; cp < c->Cp; ++cp)
                for (int k = 0; k < Cn1; ++k) t[(size_t)cp * Cn1 + k] = (*tab)[(size_t)cp * Cn0 + orig[k]];
            tab->swap(t);
        }
        c->node_class = ncls;
        c->Cn = Cn1;
        c->img_refined = true;
    }
    c->img_rep = rep;
    const size_t slot = (size_t)c->img_R * c->Cn;
    c->img_cls.assign(c->img_slots() * slot, 0);
    if (own) {
        if (!c->image_host) return img_own_scores_device(c);
        img_own_scores_host(c);
        return SIMON_OK;
    }
    for (size_t t = 0; t < c->img_sizes.size(); ++t) img_slot_scores(c, c->img_sizes[t], c->img_cls.data() + t * slot);
    return SIMON_OK;
}

// every slot's image scores of pod class cp, appended to a content key (nothing for a class that scores 0 everywhere)
template <class T>
void img_row_append(const simon_ctx* c, int cp, std::vector<T>& key) {
    if (c->img_R == 0 || c->img_row_of[cp] < 0) return;
    const size_t slot = (size_t)c->img_R * c->Cn, off = (size_t)c->img_row_of[cp] * c->Cn;
    key.push_back((T)-1);                            // (a separator: rows of different lengths never alias)
    for (size_t t = 0; t < c->img_slots(); ++t)
        for (int k = 0; k < c->Cn; ++k) key.push_back((T)c->img_cls[t * slot + off + k]);
}

// Can the score-table kernel's REST path take this problem's GPU-share / topology-term features?  Terms: only required
// anti-affinity (match + anti lists; everything else is excluded by v2_features) on topology keys that give every node its own
// domain (kubernetes.io/hostname), counted on every node.  GPU: every quantity a multiple of a gcd with quotients < 2^31, at
// most kTableMaxGpuSigs distinct (gpu-mem, gpu-count) requests.  Fills g_gpu.
bool rest_supported(simon_ctx* c) {
    if (c->no_rest) return false;
    if (c->has_gpu_index) return false;   // pods that arrive with a gpu-index annotation (their own filter and Reserve rule): all-feature kernel
    if (c->Tm > kTableMaxTerms && !c->rs) return false;
    // a term's topology key is node-level (every node its own domain: kubernetes.io/hostname) or zone-like (a domain = several
    // nodes, some nodes without the label): at most 6 of the latter, domain ids below 65 535
    std::vector<int> key_kind(std::max(c->Kt, 1), -1);   // 1 node-level, 0 zone-like
    c->zone_keys.clear();
    c->key_zslot.assign(std::max(c->Kt, 1), -1);
    // (REST && SPREAD: the rows of a term nobody holds against others are never read -- stage_narrow drops them -- so the terms the spread
    // constraints alone count may carry node sets and any key)
    std::vector<char> row_read(std::max(c->Tm, 1), c->rs ? 0 : 1);
    if (c->rs)
        for (int cp = 0; cp < c->Cp; ++cp) {
            for (int e = c->anti_off.empty() ? 0 : c->anti_off[cp]; !c->anti_off.empty() && e < c->anti_off[cp + 1]; ++e) if (c->anti_idx[e] >= 0 && c->anti_idx[e] < c->Tm) row_read[c->anti_idx[e]] = 1;
            for (int e = c->port_off.empty() ? 0 : c->port_off[cp]; !c->port_off.empty() && e < c->port_off[cp + 1]; ++e) if (c->port_idx[e] >= 0 && c->port_idx[e] < c->Tm) row_read[c->port_idx[e]] = 1;
            for (int e = c->aff_off.empty() ? 0 : c->aff_off[cp]; !c->aff_off.empty() && e < c->aff_off[cp + 1]; ++e) if (c->aff_idx[e] >= 0 && c->aff_idx[e] < c->Tm) row_read[c->aff_idx[e]] = 1;
        }
    if (c->rs) {                                                          // (... and only those get rows: stage_narrow)
        int n_read = 0;
        for (int t = 0; t < c->Tm; ++t) n_read += row_read[t];
        if (n_read > kTableMaxTerms) return false;
    }
    for (int t = 0; t < c->Tm; ++t) {
        if (!row_read[t]) continue;
        if (!c->term_set.empty() && c->term_set[t] >= 0) return false;
        const int k = c->term_key[t];
        if (key_kind[k] < 0) {
            std::vector<char> seen(c->N, 0);
            key_kind[k] = 1;
            for (int j = 0; j < c->N; ++j) {
                const int d = c->topo_dom[(size_t)k * c->N + j];
                if (d < -1 || d >= 65535) return false;
                if (d < 0 || d >= c->N || seen[d]) key_kind[k] = 0; else seen[d] = 1;
            }
            if (!key_kind[k]) {
                if (c->zone_keys.size() == 6) return false;
                c->key_zslot[k] = (int)c->zone_keys.size();
                c->zone_keys.push_back(k);
            }
        }
    }
    c->g_eph = 1;
    static_assert(SIMON_MAX_SCALAR == 4, "simon_table.hip keeps ephemeral storage + 4 extended resources in 5 components");
    if (c->xres) {
        // Extra resources as mask rows: the rows stand for `Allocatable < request + Requested`, which is also what fitsRequest asks of
        // pods that request NONE of them (ephemeral storage is compared whatever the request) -- exact as long as Requested never
        // exceeds Allocatable: nothing over-committed at the start, and no pod bound by Spec.NodeName (no filter) requests any.
        uint64_t g = 0;
        const uint64_t lim31 = 1ull << 31;
        for (int j = 0; j < c->N; ++j) {
            if (c->i_req_eph[j] < 0 || c->i_req_eph[j] > c->alloc_eph[j]) return false;
            g = gcd_u64(gcd_u64(g, (uint64_t)c->alloc_eph[j]), (uint64_t)c->i_req_eph[j]);
            for (int k = 0; k < c->K; ++k) {
                const int64_t a = c->scalar_alloc[(size_t)k * c->N + j], u = c->i_scalar_req[(size_t)k * c->N + j];
                if (a < 0 || u < 0 || u > a || (uint64_t)a >= lim31) return false;
            }
        }
        std::set<std::vector<int64_t>> sigs;
        for (int p = 0; p < c->P; ++p) {
            std::vector<int64_t> key{c->p_req_eph[p]};
            bool any = c->p_req_eph[p] != 0;
            if (c->p_req_eph[p] < 0) return false;
            for (int k = 0; k < c->K; ++k) {
                const int64_t q = c->p_scalar[(size_t)k * c->P + p];
                if (q < 0 || (uint64_t)q >= lim31) return false;
                key.push_back(q); any = any || q != 0;
            }
            if (!any) continue;
            if (c->p_preset[p] >= 0) return false;                // (flagged for eviction or not: where its node is present the pod is bound there)
            g = gcd_u64(g, (uint64_t)c->p_req_eph[p]);
            sigs.insert(key);
            if ((int)sigs.size() > kTableMaxXres) return false;
        }
        if (!g) g = 1;
        for (int j = 0; j < c->N; ++j) if ((uint64_t)c->alloc_eph[j] / g >= lim31) return false;
        for (int p = 0; p < c->P; ++p) if ((uint64_t)c->p_req_eph[p] / g >= lim31) return false;
        c->g_eph = g;
    }
    c->g_gpu = 1;
    if (c->has_gpu) {
        uint64_t g = 0;
        auto take = [&](int64_t x) { if (x < 0) return false; g = gcd_u64(g, (uint64_t)x); return true; };
        for (int j = 0; j < c->N; ++j) {
            if (c->gpu_mem_total[j] < 0) return false;
            if (c->gpu_cnt[j] > 0 && !take(c->gpu_mem_total[j] / c->gpu_cnt[j])) return false;
            for (int d = 0; d < SIMON_MAX_GPU_DEV; ++d) if (!take(c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d])) return false;
        }
        for (int p = 0; p < c->P; ++p) if (c->p_gpu_mem[p] > 0) take(c->p_gpu_mem[p]);
        if (!g) g = 1;
        const uint64_t lim31 = 1ull << 31;
        for (int j = 0; j < c->N; ++j) {
            if (c->gpu_cnt[j] > 0 && (uint64_t)(c->gpu_mem_total[j] / c->gpu_cnt[j]) / g >= lim31) return false;
            for (int d = 0; d < SIMON_MAX_GPU_DEV; ++d) if ((uint64_t)c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d] / g >= lim31) return false;
        }
        std::set<std::pair<uint64_t, int>> sigs;
        for (int p = 0; p < c->P; ++p) {
            if (c->p_gpu_mem[p] <= 0) continue;
            if ((uint64_t)c->p_gpu_mem[p] / g >= lim31) return false;
            sigs.insert({(uint64_t)c->p_gpu_mem[p] / g, std::min(c->p_gpu_cnt[p], 64)});
            if ((int)sigs.size() > kTableMaxGpuSigs) return false;
        }
        c->g_gpu = g;
    }
    return true;
}

// Open-Gpu-Share FOLDED into the score table (round 4).  "GPU request g no longer fits node j" is monotone -- device memory is only ever
// booked -- which is what a 0 in the (signature, node) table already means.  With the GPU request made part of the request signature
// the assume of a GPU pod books the devices (Reserve) and zeroes the bytes of the signatures whose request stopped fitting; a GPU pod
// then needs NO select-time filter: it takes the summary scan, or generation 7's walk when a Service selects it.  Worth it when the
// signatures stay few (real gpushare workloads: a handful of Deployments) -- config 5's 42 shapes x 8 GPU requests keep the position
// masks of generation 6.  Needs: no arriving gpu-index lists, GPU quantities on a gcd with quotients < 2^31 (fills g_gpu), at most
// 1 023 signatures once the GPU request is part of them (beyond 128 only under generation 7's walks: choose_variant).
bool gfold_supported(simon_ctx* c) {
    if (c->no_gpu_fold || c->no_rest || !c->has_gpu || c->has_gpu_index || c->gpu_cnt.empty()) return false;   // (SIMON_NO_REST keeps meaning: GPU problems on the all-feature kernel)
    uint64_t g = 0;
    auto take = [&](int64_t x) { if (x < 0) return false; g = gcd_u64(g, (uint64_t)x); return true; };
    for (int j = 0; j < c->N; ++j) {
        if (c->gpu_mem_total[j] < 0) return false;
        if (c->gpu_cnt[j] > 0 && !take(c->gpu_mem_total[j] / c->gpu_cnt[j])) return false;
        for (int d = 0; d < SIMON_MAX_GPU_DEV; ++d) if (!take(c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d])) return false;
    }
    for (int p = 0; p < c->P; ++p) if (c->p_gpu_mem[p] > 0) take(c->p_gpu_mem[p]);
    if (!g) g = 1;
    const uint64_t lim31 = 1ull << 31;
    for (int j = 0; j < c->N; ++j) {
        if (c->gpu_cnt[j] > 0 && (uint64_t)(c->gpu_mem_total[j] / c->gpu_cnt[j]) / g >= lim31) return false;
        for (int d = 0; d < SIMON_MAX_GPU_DEV; ++d) if ((uint64_t)c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d] / g >= lim31) return false;
    }
    for (int p = 0; p < c->P; ++p) if (c->p_gpu_mem[p] > 0 && (uint64_t)c->p_gpu_mem[p] / g >= lim31) return false;
    // signatures the table would need: (request, content of the class's static rows as stage_narrow interns them, GPU request)
    const int Cp = c->Cp;
    std::vector<int32_t> content_of(Cp);
    {
        const size_t words = (size_t)(c->N + 63) / 64;
        std::map<std::pair<std::vector<uint64_t>, std::vector<int64_t>>, int> ids;
        for (int cp = 0; cp < Cp; ++cp) {
            std::vector<uint64_t> mrow;
            if (c->has_mask) mrow.assign(c->static_mask.begin() + (size_t)cp * words, c->static_mask.begin() + (size_t)(cp + 1) * words);
            std::vector<int64_t> rrow;
            for (const std::vector<int64_t>* tab : {&c->simon_raw, &c->na_raw, &c->tt_raw, &c->static_add})
                if (!tab->empty()) rrow.insert(rrow.end(), tab->begin() + (size_t)cp * c->Cn, tab->begin() + (size_t)(cp + 1) * c->Cn);
            img_row_append(c, cp, rrow);
            content_of[cp] = ids.emplace(std::make_pair(std::move(mrow), std::move(rrow)), (int)ids.size()).first->second;
        }
    }
    std::set<std::tuple<int64_t, int64_t, int64_t, int64_t, int32_t, int32_t, int64_t, int32_t>> sig;
    std::set<std::tuple<int64_t, int64_t, int64_t, int64_t, int32_t>> base;   // ... and without the GPU request / filter class: generation 6's signatures
    for (int p = 0; p < c->P; ++p) {
        const bool gp = c->p_gpu_mem[p] > 0;
        if ((int)base.size() <= 128) base.insert(std::make_tuple(c->p_req_cpu[p], c->p_req_mem[p], c->p_nz_cpu[p], c->p_nz_mem[p], content_of[c->p_cls[p]]));
        sig.insert(std::make_tuple(c->p_req_cpu[p], c->p_req_mem[p], c->p_nz_cpu[p], c->p_nz_mem[p], content_of[c->p_cls[p]],
                                   c->fold ? c->fold_fc[c->p_cls[p]] : 0, gp ? c->p_gpu_mem[p] : 0, gp ? std::min(c->p_gpu_cnt[p], 64) : 0));
        if ((int)sig.size() > kTableMaxSigs) return false;
    }
    c->gfold_sigs = (int)sig.size();
    c->gfold_base_sigs = (int)base.size();
    c->gfold_g = g;
    c->g_gpu = g;
    return true;
}

// Can the score-table kernel's SPREAD path (generation 7) take this problem?  Of the ABI v2 features: SOFT PodTopologySpread constraints
// (+ the static score tables the class term folds in), InterPodAffinity PREFERRED terms whose owners hold one weight per pod with at
// most one hostname-like counter per class, HARD spread constraints on zone-like keys whose eligible nodes are all the
// labelled ones (5.3f), required anti-affinity / host ports where they fold into the table (fold_supported, 5.3d).  Not: required
// affinity, Open-Gpu-Share / extra-resource rows (the REST path), Open-Local.  Every term with a counter sits on a hostname-like key
// (flagged topo_is_hostname, every node its own domain: one counter byte per position) or on a zone-like key (<= 16 domains; <= 3 such
// keys: the node classes are split by their domains).  Fills sp_kind / sp_row / sp_zslot / sp_zkeys / sp_rep / sp_set_eff and the
// per-class entries of the preferred score.
bool spread_supported(simon_ctx* c) {
    c->ipa_fold = false;
    c->ipa_h_term.clear(); c->ipa_h_w.clear(); c->ipa_z.clear();
    c->hard_fold = false;
    if (c->no_spread || (c->ss_idx.empty() && !c->has_ipa_score && c->sh_idx.empty())) return false;
    if (!c->sh_idx.empty() && c->no_hard_fold) return false;
    if (c->has_ipa_score && c->no_ipa_fold) return false;
    if (c->has_local || (!c->aff_idx.empty() && !c->rs_probe)) return false;   // (required affinity: rows that must be SET -- the mask rows, rs_probe)
    if ((!c->anti_idx.empty() || !c->port_idx.empty()) && !c->fold && !c->rs_probe) return false;   // required anti-affinity / ports: folded into the table, or (rs_probe) on the mask rows
    if (c->has_gpu_index || (c->has_gpu && !c->gfold && !c->rs_probe)) return false;      // (GPU share: folded into the table, gfold_supported -- or on the mask rows)
    if (c->topo_is_hostname.empty()) return false;
    if (!c->ss_idx.empty() && c->spread_log.size() < (size_t)c->N + 1) return false;
    int64_t max_pods = 0;
    // the per-position counters are bytes.  Pods that pass NodeResourcesFit number at most alloc_pods on a node; pods bound by
    // Spec.NodeName (presets) skip the filters (V/eventhandlers.go:223-236) and come on top.  (A pod flagged for eviction counts on its
    // preset node where it is bound and among the alloc_pods of the node it is scheduled to where it is not: the bound holds for both.)
    {
        std::vector<int32_t> preset_on(c->N, 0);
        for (int p = 0; p < c->P && !c->p_preset.empty(); ++p)
            if (c->p_preset[p] >= 0 && c->p_preset[p] < c->N) ++preset_on[c->p_preset[p]];
        for (int j = 0; j < c->N; ++j) {
            const int64_t x = (int64_t)c->alloc_pods[j] + preset_on[j];
            if (x > 255) return false;
            max_pods = std::max<int64_t>(max_pods, x);
        }
    }
    // ids: t < Tm = the pods MATCHING term t; Tm + t = the pods OWNING a scoring term t (one weight per pod: InterPodAffinity below)
    c->sp_kind.assign(2 * (size_t)c->Tm, 0); c->sp_row.assign(2 * (size_t)c->Tm, 0); c->sp_zslot.assign(2 * (size_t)c->Tm, 0);
    c->sp_zkeys.clear();
    c->sp_TH = c->sp_TZ = 0;
    std::vector<int> key_kind(std::max(c->Kt, 1), -1);                    // 1 hostname-like, 2 zone-like, 0 unusable
    // Terms on one key, counted on the same nodes, that the same pod classes match with the same multiplicities have the same
    // counters at all times (a Service's default constraint and the chart's anti-affinity term with the same selector): they share
    // ONE row, kept under the first of them (sp_rep).
    c->sp_rep.assign(2 * (size_t)c->Tm, 0);
    std::vector<long long> own_w_of(c->Tm, 0);                            // per-pod weight of the owners of term t (0: nobody owns it)
    bool own_uniform = true;
    {
        std::vector<std::vector<std::pair<int, int>>> who(2 * (size_t)c->Tm);
        for (int cp = 0; cp < c->Cp && !c->own_off.empty(); ++cp) {     // the owner classes of a scoring term, when they all hold one weight per pod
            std::map<int, long long> os;
            for (int e = c->own_off[cp]; e < c->own_off[cp + 1]; ++e) { const int t = c->own_idx[e]; if (t < 0 || t >= c->Tm) return false; os[t] += c->own_w[e]; }
            for (auto& kv : os) {
                if (kv.second == 0) continue;
                if (own_w_of[kv.first] == 0) own_w_of[kv.first] = kv.second;
                else if (own_w_of[kv.first] != kv.second) own_uniform = false;
                who[(size_t)c->Tm + kv.first].push_back(std::make_pair(cp, 1));
            }
        }
        for (int cp = 0; cp < c->Cp && !c->match_off.empty(); ++cp) {
            std::map<int, int> mult;
            for (int e = c->match_off[cp]; e < c->match_off[cp + 1]; ++e) { const int t = c->match_idx[e]; if (t < 0 || t >= c->Tm) return false; ++mult[t]; }
            for (auto& kv : mult) who[kv.first].push_back(std::make_pair(cp, kv.second));
        }
        const int words = (c->N + 63) / 64;                               // a node set that holds every node counts like no node set
        std::vector<char> full(std::max(c->R, 1), 0);
        for (int r = 0; r < c->R && (size_t)(r + 1) * words <= c->node_sets.size(); ++r) {
            long long n_in = 0;
            for (int wd = 0; wd < words; ++wd) n_in += __builtin_popcountll(c->node_sets[(size_t)r * words + wd] & (wd == words - 1 && (c->N & 63) ? (1ull << (c->N & 63)) - 1 : ~0ull));
            full[r] = n_in == c->N;
        }
        // A node set that leaves out only nodes WITHOUT the term's own label changes no counter (a zone-like key: such a node has no
        // domain); on a hostname-like key the set never matters to a reader at all -- a node outside it either fails the class's node
        // affinity (never feasible) or lacks a constraint key (IgnoredNodes: never scored).  Such terms join the unrestricted ones; a
        // group is kept under an unrestricted member when it has one (a reader of the preferred score wants the count everywhere).
        std::map<std::pair<int, int>, char> harmless;
        auto set_of = [&](int id) -> int {
            if (id >= c->Tm || c->term_set.empty()) return -1;            // (owners are counted wherever they land)
            const int set = c->term_set[id], k = c->term_key[id];
            if (set < 0 || set >= c->R || full[set]) return -1;
            if (c->topo_is_hostname[k]) return -1;
            auto it = harmless.find(std::make_pair(k, set));
            if (it == harmless.end()) {
                bool ok = true;
                for (int j = 0; j < c->N && ok; ++j)
                    if (!((c->node_sets[(size_t)set * words + (j >> 6)] >> (j & 63)) & 1ull)) ok = c->topo_dom[(size_t)k * c->N + j] < 0;
                it = harmless.emplace(std::make_pair(k, set), (char)ok).first;
            }
            return it->second ? -1 : set;
        };
        std::map<std::tuple<int, int, std::vector<std::pair<int, int>>>, int> first;
        for (int pass = 0; pass < 2; ++pass)
            for (int id = 0; id < 2 * c->Tm; ++id) {
                const int t = id < c->Tm ? id : id - c->Tm;
                const bool unrestricted = id >= c->Tm || c->term_set.empty() || c->term_set[id] < 0;
                if (unrestricted != (pass == 0)) continue;
                c->sp_rep[id] = first.emplace(std::make_tuple(c->term_key[t], set_of(id), who[id]), id).first->second;
            }
        // the set a row is COUNTED on: none where it does not matter -- members of one group may carry different (harmless) sets, and each
        // reads inside its own only, where counting everywhere and counting on the set agree
        c->sp_set_eff.assign(2 * (size_t)c->Tm, -1);
        for (int id = 0; id < c->Tm; ++id) c->sp_set_eff[id] = set_of(id);
    }
    // a term gets a counter row: a byte per position (hostname-like key) or a word per domain (zone-like key)
    auto classify = [&](int t) -> int {
        if (t < 0 || t >= 2 * c->Tm) return 0;
        const int r = c->sp_rep[t];
        const int k = c->term_key[r < c->Tm ? r : r - c->Tm];
        if (key_kind[k] < 0) {
            key_kind[k] = 0;
            if (c->topo_is_hostname[k]) {                                 // size = scored nodes (scoring.go:100-104): needs one domain per node
                std::vector<char> seen(c->N, 0);
                bool ok = true;
                for (int j = 0; j < c->N && ok; ++j) {
                    const int d = c->topo_dom[(size_t)k * c->N + j];
                    ok = d >= 0 && d < c->N && !seen[d];
                    if (ok) seen[d] = 1;
                }
                key_kind[k] = ok ? 1 : 0;
            } else {
                bool ok = c->topo_n_dom[k] <= kSpreadMaxZoneDom;
                for (int j = 0; j < c->N && ok; ++j) { const int d = c->topo_dom[(size_t)k * c->N + j]; ok = d >= -1 && d < kSpreadMaxZoneDom; }
                if (ok && (int)c->sp_zkeys.size() < kSpreadMaxZoneKeys) { key_kind[k] = 2; c->sp_zkeys.push_back(k); }
            }
        }
        if (key_kind[k] == 0) return 0;
        if (c->sp_kind[r] == 0) {
            c->sp_kind[r] = key_kind[k];
            if (key_kind[k] == 1) c->sp_row[r] = c->sp_TH++;
            else {
                c->sp_row[r] = c->sp_TZ++;
                c->sp_zslot[r] = (int)(std::find(c->sp_zkeys.begin(), c->sp_zkeys.end(), k) - c->sp_zkeys.begin());
            }
        }
        if (t != r) { c->sp_kind[t] = c->sp_kind[r]; c->sp_row[t] = c->sp_row[r]; c->sp_zslot[t] = c->sp_zslot[r]; }
        return key_kind[k];
    };
    for (int cp = 0; cp < c->Cp && !c->ss_idx.empty(); ++cp) {
        for (int e = c->ss_off[cp]; e < c->ss_off[cp + 1]; ++e) {
            const int maxskew = c->ss_skew[e] & ~SIMON_SPREAD_DUP_KEY;
            if (maxskew < 1 || maxskew >= (1 << 14)) return false;
            if (!classify(c->ss_idx[e])) return false;
        }
    }
    // Hard (DoNotSchedule) constraints on ZONE-like keys: a per-class verdict in spread_select (the classes are split by zone).  The
    // eligibility set of an entry (filtering.go:236-251: which nodes register a zone) may leave out unlabelled nodes only.
    if (!c->sh_idx.empty()) {
        const int words = (c->N + 63) / 64;
        for (int cp = 0; cp < c->Cp; ++cp) {
            if (c->sh_off[cp + 1] - c->sh_off[cp] > 3) return false;
            for (int e = c->sh_off[cp]; e < c->sh_off[cp + 1]; ++e) {
                const int t = c->sh_idx[e];
                if (t < 0 || t >= c->Tm || c->sh_skew[e] < 1 || c->sh_skew[e] >= (1 << 14)) return false;
                if (classify(t) != 2) return false;                       // hostname-like hard constraints: the all-feature kernel
                const int set = c->sh_set.empty() ? -1 : c->sh_set[e], k = c->term_key[t];
                if (set >= 0) {
                    if (set >= c->R) return false;
                    for (int j = 0; j < c->N; ++j)
                        if (!((c->node_sets[(size_t)set * words + (j >> 6)] >> (j & 63)) & 1ull) && c->topo_dom[(size_t)k * c->N + j] >= 0) return false;
                }
            }
        }
        // a pinned pod (one admissible node) is decided from the table byte of that node alone: it must not carry a hard constraint
        for (int p = 0; p < c->P && !c->p_pin.empty(); ++p)
            if (c->p_pin[p] >= 0 && c->sh_off[c->p_cls[p] + 1] > c->sh_off[c->p_cls[p]]) return false;
        c->hard_fold = true;
    }
    // InterPodAffinity preferred terms (scoring.go:87-271) in their usual, SELF-REFERENTIAL form: the raw score of pod class cp on a node is
    //   sum_e pref_w[e] * cnt_match[t_e][dom] + sum_{t in match(cp)} w_owner[t][dom],
    // and w_owner[t] = w_t * cnt_match[t] whenever every class owns t with w_t times the multiplicity it matches t with (the pods a
    // workload's (anti-)affinity term selects are the workload's own).  Then raw = sum_t coef(cp, t) * cnt_match[t][dom]: with at most ONE
    // hostname-like term per class -- the one its soft spread constraint counts, if it has one -- the raw score is a function of (class,
    // count) like the spread score and joins it in spread_select's table; zone-like terms add a per-class constant.
    if (c->has_ipa_score) {
        if (c->match_off.empty()) return false;
        const int Cp = c->Cp, T = c->Tm;
        std::vector<std::map<int, long long>> prefsum(Cp), mult(Cp);
        for (int cp = 0; cp < Cp; ++cp) {
            if (!c->pref_off.empty()) for (int e = c->pref_off[cp]; e < c->pref_off[cp + 1]; ++e) prefsum[cp][c->pref_idx[e]] += c->pref_w[e];
            for (int e = c->match_off[cp]; e < c->match_off[cp + 1]; ++e) mult[cp][c->match_idx[e]] += 1;
        }
        // w_owner[t] = (the owners' weight per pod) x (owner pods in the domain): a counter row of its own (id Tm + t) -- the SAME row as
        // cnt_match[t]'s when the owners are the matchers (sp_rep), the self-referential case
        if (!own_uniform) return false;
        c->ipa_h_term.assign(Cp, -1); c->ipa_h_w.assign(Cp, 0); c->ipa_z.assign(Cp, {});
        for (int cp = 0; cp < Cp; ++cp) {
            std::map<int, long long> coef;
            for (auto& kv : prefsum[cp]) { if (kv.first < 0 || kv.first >= T) return false; coef[c->sp_rep[kv.first]] += kv.second; }   // (per counter row)
            for (auto& kv : mult[cp]) if (own_w_of[kv.first] != 0) coef[c->sp_rep[(size_t)T + kv.first]] += kv.second * own_w_of[kv.first];
            int spread_host = -1;                                         // the class's own hostname-like soft constraint, if any
            for (int e = c->ss_idx.empty() ? 0 : c->ss_off[cp]; !c->ss_idx.empty() && e < c->ss_off[cp + 1]; ++e)
                if (c->sp_kind[c->ss_idx[e]] == 1) { const int r = c->sp_rep[c->ss_idx[e]]; if (spread_host >= 0 && spread_host != r) return false; spread_host = r; }
            for (auto& kv : coef) {
                if (kv.second == 0) continue;
                if (std::llabs(kv.second) >= (1ll << 20)) return false;
                if (kv.first < T && !c->term_set.empty() && c->term_set[kv.first] >= 0) return false;
                const int kind = classify(kv.first);
                if (kind == 0) return false;
                if (kind == 1) {
                    if (c->ipa_h_term[cp] >= 0) return false;             // two per-node counters: not a function of one count
                    if (spread_host >= 0 && spread_host != kv.first) return false;
                    c->ipa_h_term[cp] = kv.first; c->ipa_h_w[cp] = (int32_t)kv.second;
                } else {
                    if (c->ipa_z[cp].size() == 3) return false;
                    c->ipa_z[cp].push_back(std::make_pair(kv.first, (int32_t)kv.second));
                }
            }
            // a class whose spread constraints take the general walk of spread_select (several hostname-like constraints, or one behind a
            // zone-like one) keeps the all-feature kernel when it also has a preferred term
            if ((c->ipa_h_term[cp] >= 0 || !c->ipa_z[cp].empty()) && !c->ss_idx.empty()) {
                int nh = 0, first_kind = 0, ns = c->ss_off[cp + 1] - c->ss_off[cp];
                for (int e = c->ss_off[cp]; e < c->ss_off[cp + 1]; ++e) { nh += c->sp_kind[c->ss_idx[e]] == 1; if (e == c->ss_off[cp]) first_kind = c->sp_kind[c->ss_idx[e]]; }
                if (!(nh == 0 || (nh == 1 && first_kind == 1 && ns <= 2))) return false;
            }
        }
        c->ipa_fold = true;
    }
    if (c->sp_TH > kSpreadMaxHostTerms || c->sp_TZ > kSpreadMaxZoneTerms || c->R > 4094) return false;
    // counted terms of a class: the terms with a counter row among its match list, with multiplicity; one lane per distinct term
    for (int cp = 0; cp < c->Cp && !c->match_off.empty(); ++cp) {
        std::map<int, int> mult;                                           // per counter ROW (terms that share one count once)
        {
            std::map<int, int> per_term;
            for (int e = c->match_off[cp]; e < c->match_off[cp + 1]; ++e) if (c->sp_kind[c->match_idx[e]]) ++per_term[c->match_idx[e]];
            for (auto& kv : per_term) mult[c->sp_rep[kv.first]] = kv.second;
            for (int e = c->own_off.empty() ? 0 : c->own_off[cp]; !c->own_off.empty() && e < c->own_off[cp + 1]; ++e)      // rows that count this class as an owner
                if (c->sp_kind[(size_t)c->Tm + c->own_idx[e]] && own_w_of[c->own_idx[e]] != 0) mult[c->sp_rep[(size_t)c->Tm + c->own_idx[e]]] = 1;
        }
        const int ns = c->ss_idx.empty() ? 0 : c->ss_off[cp + 1] - c->ss_off[cp];
        const int ni = (c->ipa_fold ? (c->ipa_h_term[cp] >= 0 ? 1 : 0) + (int)c->ipa_z[cp].size() : 0) + (c->hard_fold ? c->sh_off[cp + 1] - c->sh_off[cp] : 0);
        if ((int)mult.size() + ns + ni > 64) return false;
        for (auto& kv : mult) if ((int64_t)kv.second * max_pods > 255) return false;   // a byte counter: pods on a node x multiplicity
    }
    return true;
}

// Required anti-affinity (both directions, filtering.go:319-346) and NodePorts conflicts (node_ports.go:104-127) on node-level topology
// keys never leave the node the pod lands on, and pods never leave: "signature S cannot use node j any more" is the monotone
// infeasibility the score table already knows (byte 0 stays 0).  The fold needs: only anti / match / port lists among the
// placement-dependent filters, every such term on a key that gives every node its own domain, counted on every node; the filter
// class (anti list, relevant match list, port list) becomes part of the request signature.
bool fold_supported(simon_ctx* c) {
    c->fold_fc.clear(); c->fold_x.clear(); c->fold_FC = 0; c->fold_sigs = 0;
    if (c->no_fold || c->Tm <= 0 || (c->anti_idx.empty() && c->port_idx.empty())) return false;
    // (GPU share next to the fold: only when it is folded too -- choose_variant drops the fold again when gfold_supported says no)
    if (!c->aff_idx.empty() || c->has_gpu_index || (c->has_gpu && (c->no_gpu_fold || c->no_rest)) || c->match_off.empty()) return false;
    const int Cp = c->Cp, N = c->N;
    std::vector<char> relevant(c->Tm, 0);
    auto list_of = [&](const std::vector<int32_t>& off, const std::vector<int32_t>& idx, int cp) {
        std::vector<int32_t> v;
        if (!off.empty()) v.assign(idx.begin() + off[cp], idx.begin() + off[cp + 1]);
        std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end());
        return v;
    };
    for (int cp = 0; cp < Cp; ++cp) {
        for (int t : list_of(c->anti_off, c->anti_idx, cp)) { if (t < 0 || t >= c->Tm) return false; relevant[t] = 1; }
        for (int t : list_of(c->port_off, c->port_idx, cp)) { if (t < 0 || t >= c->Tm) return false; relevant[t] = 1; }
    }
    std::vector<int> key_ok(std::max(c->Kt, 1), -1);
    for (int t = 0; t < c->Tm; ++t) {
        if (!relevant[t]) continue;
        if (!c->term_set.empty() && c->term_set[t] >= 0) return false;
        const int k = c->term_key[t];
        if (key_ok[k] < 0) {
            std::vector<char> seen(N, 0);
            key_ok[k] = 1;
            for (int j = 0; j < N && key_ok[k]; ++j) {
                const int d = c->topo_dom[(size_t)k * N + j];
                if (d < 0 || d >= N || seen[d]) key_ok[k] = 0; else seen[d] = 1;
            }
        }
        if (!key_ok[k]) return false;
    }
    // filter classes by content
    std::map<std::tuple<std::vector<int32_t>, std::vector<int32_t>, std::vector<int32_t>>, int> fc_id;
    std::vector<std::tuple<std::vector<int32_t>, std::vector<int32_t>, std::vector<int32_t>>> fcs;
    c->fold_fc.assign(Cp, 0);
    for (int cp = 0; cp < Cp; ++cp) {
        std::vector<int32_t> anti = list_of(c->anti_off, c->anti_idx, cp), port = list_of(c->port_off, c->port_idx, cp), match;
        for (int t : list_of(c->match_off, c->match_idx, cp)) { if (t < 0 || t >= c->Tm) return false; if (relevant[t]) match.push_back(t); }
        auto key = std::make_tuple(anti, match, port);
        auto it = fc_id.emplace(key, (int)fcs.size());
        if (it.second) fcs.push_back(key);
        c->fold_fc[cp] = it.first->second;
    }
    const int FC = (int)fcs.size();
    if (FC > 4096) return false;
    auto meets = [](const std::vector<int32_t>& a, const std::vector<int32_t>& b) {       // sorted lists share an element
        size_t i = 0, j = 0;
        while (i < a.size() && j < b.size()) { if (a[i] == b[j]) return true; if (a[i] < b[j]) ++i; else ++j; }
        return false;
    };
    c->fold_x.assign((size_t)FC * FC, 0);
    for (int L = 0; L < FC; ++L)
        for (int S = 0; S < FC; ++S)       // L has landed: S meets a pod matching one of its anti terms / ports, or a pod requiring a term S matches
            c->fold_x[(size_t)L * FC + S] = meets(std::get<0>(fcs[S]), std::get<1>(fcs[L])) || meets(std::get<1>(fcs[S]), std::get<0>(fcs[L])) ||
                                            meets(std::get<2>(fcs[S]), std::get<1>(fcs[L]));
    c->fold_FC = FC;
    // signatures the table would need: (request, content of the class's static rows as stage_narrow interns them, filter class)
    std::vector<int32_t> content_of(Cp);
    {
        const size_t words = (size_t)(N + 63) / 64;
        std::map<std::pair<std::vector<uint64_t>, std::vector<int64_t>>, int> ids;
        for (int cp = 0; cp < Cp; ++cp) {
            std::vector<uint64_t> mrow;
            if (c->has_mask) mrow.assign(c->static_mask.begin() + (size_t)cp * words, c->static_mask.begin() + (size_t)(cp + 1) * words);
            std::vector<int64_t> rrow;
            for (const std::vector<int64_t>* tab : {&c->simon_raw, &c->na_raw, &c->tt_raw, &c->static_add})
                if (!tab->empty()) rrow.insert(rrow.end(), tab->begin() + (size_t)cp * c->Cn, tab->begin() + (size_t)(cp + 1) * c->Cn);
            img_row_append(c, cp, rrow);
            content_of[cp] = ids.emplace(std::make_pair(std::move(mrow), std::move(rrow)), (int)ids.size()).first->second;
        }
    }
    std::set<std::tuple<int64_t, int64_t, int64_t, int64_t, int32_t, int32_t>> sig;
    for (int p = 0; p < c->P; ++p) {
        sig.insert(std::make_tuple(c->p_req_cpu[p], c->p_req_mem[p], c->p_nz_cpu[p], c->p_nz_mem[p], content_of[c->p_cls[p]], c->fold_fc[c->p_cls[p]]));
        if ((int)sig.size() > kTableMaxSigs) return false;
    }
    c->fold_sigs = (int)sig.size();
    return true;
}

// LDS of ONE workgroup of the two-level score-table instantiations: a gfx950 workgroup may hold all 160 KB of its CU (the launch sets
// hipFuncAttributeMaxDynamicSharedMemorySize).  Past 64 KB a CU holds two, then one scenario -- still far ahead of the all-feature kernel
// for the problems that need it (hundreds of signatures x thousands of nodes under generation 7's walks); the one-level layout, which
// exists for occupancy, keeps its 64 KB bound.
static constexpr size_t kTableLdsMaxWG = 159 * 1024;

// Decide NARROW vs WIDE and compute the gcd normalisation.
// NARROW needs: cpu+mem+pods only; every quantity non-negative; after dividing by the gcd all
// node totals and the worst-case accumulated NonZeroRequested stay < 2^31; simon raw scores fit
// 30 bits; original quantities < 2^53 (exact in fp64, so BalancedAllocation is scale-invariant).
void choose_variant(simon_ctx* c) {
    c->variant = SIMON_KERNEL_WIDE;
    c->g_cpu = c->g_mem = 1;
    if (c->force_wide) return;
    c->rest = false;
    c->spread = false;
    c->has_static = c->has_na || c->has_tt || c->has_add || c->img_R > 0;
    c->fold = fold_supported(c);
    c->gfold = gfold_supported(c);
    if (c->fold && c->has_gpu && !c->gfold) c->fold = false;        // GPU share on position masks (generation 6) takes the terms along
    c->rs = false;
    if (c->v2_features_but_ports_and_static()) {
        if (!spread_supported(c)) {                               // only soft spread constraints: generation 7 of the score-table kernel
            // ... or its walks over the position-mask rows, when GPU share / required anti-affinity / ports are what keeps it out and the
            // walk scores soft constraints only
            if (c->no_rs || c->no_rest) return;
            c->rs_probe = true;
            const bool ok = spread_supported(c);
            c->rs_probe = false;
            if (c->debug_route) fprintf(stderr, "[route] walks over the mask rows: probe %d ipa %d hard %d soft %d\n", (int)ok, (int)c->ipa_fold, (int)c->hard_fold, (int)!c->ss_idx.empty());
            if (!ok) return;
            c->rs = true;
            c->fold = false; c->gfold = false;
        }
        c->spread = true;
    }
    if (c->has_static) {
        // The class term of the score-table kernel takes them if byte (<= 201) + 2 x Simon (<= 200) + NodeAffinity (<= 100) +
        // TaintToleration (<= 100) + the largest addition stays within the 10 bits the two-level summary gives a total.
        int64_t add_max = 0;
        for (int64_t x : c->na_raw) if (x < 0 || x >= (1ll << 30)) return;
        for (int64_t x : c->tt_raw) if (x < 0 || x >= (1ll << 30)) return;
        for (int64_t x : c->static_add) { if (x < 0) return; add_max = std::max(add_max, x); }
        if (201 + 200 + (c->has_na ? 100 : 0) + (c->has_tt ? 100 : 0) + add_max + (c->img_R > 0 ? 100 : 0) > 1023) return;   // (+ ImageLocality <= 100)
    }
    // Ephemeral storage and extended resources take part only when somebody requests them: with no request and nothing requested at
    // the start, fitsRequest's `Allocatable < request + Requested` (fit.go:264-299) is 0-false on every node whatever the allocatable.
    for (int64_t x : c->alloc_eph) if (x < 0) return;
    c->xres = false;
    for (int64_t x : c->i_req_eph) if (x) c->xres = true;
    for (int64_t x : c->p_req_eph) if (x) c->xres = true;
    for (int64_t x : c->i_scalar_req) if (x) c->xres = true;
    for (int64_t x : c->p_scalar) if (x) c->xres = true;
    if (c->fold && c->xres) c->fold = false;                        // (extra-resource rows live on the REST path)
    // anti-affinity / ports without soft spread constraints: the fold while two signatures per lane hold them, else the position masks
    if (c->fold && !c->spread && c->fold_sigs > 128 && rest_supported(c)) c->fold = false;
    // ... and GPU share alike: with more than 128 signatures the device rows of generation 6 beat the signature groups read from memory
    // (generation 6 itself holds <= 128 signatures: where the requests alone are more, the fold with its signature groups is what is left)
    if (c->gfold && !c->spread && c->gfold_sigs > 128 && c->gfold_base_sigs <= 128 && rest_supported(c)) { c->gfold = false; c->fold = false; }
    // the GPU fold serves problems that need no other per-node filter row: plain cpu+memory+GPU, and generation 7's (Services next to GPU pods)
    if (c->gfold && ((!c->spread && !c->fold && c->Tm > 0) || c->xres)) { c->gfold = false; if (c->has_gpu) c->fold = false; }
    if (c->spread && !c->rs && !c->no_rs && !c->no_rest && c->xres && c->aff_idx.empty()) {
        c->rs = true; c->fold = false; c->gfold = false;            // extra-resource rows under the walks: the same instantiation
    }
    const bool wants_rest = (!c->spread || c->rs) && !c->fold && ((c->has_gpu && !c->gfold) || c->Tm > 0 || c->xres);
    // rest_supported() above ran as a probe and leaves g_gpu = 1 when it says no (e.g. more than kTableMaxGpuSigs GPU requests): a fold
    // that survives the probes stages its quantities on ITS gcd -- the 31-bit bounds were checked against that one, not against 1
    if (c->gfold) c->g_gpu = c->gfold_g;
    if (c->spread && !c->rs && c->xres) { c->spread = false; return; }       // extra-resource rows live on the REST path: all-feature kernel
    if (c->spread && !c->rs && !c->fold && (!c->anti_idx.empty() || !c->port_idx.empty())) { c->spread = false; return; }
    if (c->rs && !wants_rest) c->rs = false;
    if (wants_rest && !rest_supported(c)) { if (c->debug_route) fprintf(stderr, "[route] mask rows refused (rs %d)\n", (int)c->rs); return; }
    if (c->N >= (1 << 20) - 1) return;
    const uint64_t gc = gcd_of({&c->alloc_cpu, &c->i_req_cpu, &c->i_nz_cpu, &c->p_req_cpu, &c->p_nz_cpu});
    const uint64_t gm = gcd_of({&c->alloc_mem, &c->i_req_mem, &c->i_nz_mem, &c->p_req_mem, &c->p_nz_mem});
    if (!gc || !gm) return;  // negative quantity somewhere
    const uint64_t lim53 = 1ull << 53, lim31 = 1ull << 31;
    auto bounded = [&](const std::vector<int64_t>& alloc, const std::vector<int64_t>& irq, const std::vector<int64_t>& inz,
                       const std::vector<int64_t>& prq, const std::vector<int64_t>& pnz, uint64_t g) {
        uint64_t max_node = 0, sum_p = 0;
        for (size_t j = 0; j < alloc.size(); ++j)
            max_node = std::max({max_node, (uint64_t)alloc[j], (uint64_t)irq[j], (uint64_t)inz[j]});
        for (size_t p = 0; p < prq.size(); ++p) {
            sum_p += std::max((uint64_t)prq[p], (uint64_t)pnz[p]);
            if (sum_p >= lim53) return false;
        }
        if (max_node + sum_p >= lim53) return false;
        return (max_node + sum_p) / g < lim31;
    };
    if (!bounded(c->alloc_cpu, c->i_req_cpu, c->i_nz_cpu, c->p_req_cpu, c->p_nz_cpu, gc)) return;
    if (!bounded(c->alloc_mem, c->i_req_mem, c->i_nz_mem, c->p_req_mem, c->p_nz_mem, gm)) return;
    for (int64_t r : c->simon_raw) if (r < 0 || r >= (1ll << 30)) return;
    // generations 1 and 2 keep simon_raw [Cp][Cn] in LDS; the score-table kernel reads it by table class from global memory
    c->raw_fits_lds = (size_t)c->Cp * c->Cn * sizeof(int32_t) <= 60 * 1024;
    c->variant = SIMON_KERNEL_NARROW;
    c->g_cpu = gc;
    c->g_mem = gm;
    c->rest = wants_rest;
}

int stage_narrow(simon_ctx* c) {
    const int N = c->N, P = c->P;
    std::vector<uint32_t> a_cpu(N), a_mem(N), rqc(N), rqm(N), nzc(N), nzm(N);
    for (int j = 0; j < N; ++j) {
        a_cpu[j] = (uint32_t)(c->alloc_cpu[j] / c->g_cpu);
        a_mem[j] = (uint32_t)(c->alloc_mem[j] / c->g_mem);
        rqc[j] = (uint32_t)(c->i_req_cpu[j] / c->g_cpu);
        rqm[j] = (uint32_t)(c->i_req_mem[j] / c->g_mem);
        nzc[j] = (uint32_t)(c->i_nz_cpu[j] / c->g_cpu);
        nzm[j] = (uint32_t)(c->i_nz_mem[j] / c->g_mem);
    }
    std::vector<PodRowN> rows(P);
    for (int p = 0; p < P; ++p) {
        PodRowN& r = rows[p];
        r.req_cpu = (uint32_t)(c->p_req_cpu[p] / c->g_cpu);
        r.req_mem = (uint32_t)(c->p_req_mem[p] / c->g_mem);
        r.nz_cpu = (uint32_t)(c->p_nz_cpu[p] / c->g_cpu);
        r.nz_mem = (uint32_t)(c->p_nz_mem[p] / c->g_mem);
        r.cls = c->p_cls[p];
        r.preset = c->p_preset[p];
        r.gate = c->p_gate[p];
        bool no_xres = c->p_req_eph[p] == 0;                     // fit.go:244-249: the early return needs EVERY request to be zero
        for (int k = 0; k < c->K && no_xres; ++k) no_xres = c->p_scalar[(size_t)k * c->P + p] == 0;
        if (!c->p_entries.empty() && c->p_entries[p]) no_xres = false;   // ... and to hold no ScalarResources ENTRY, not even one of quantity 0 (simon_set_scalar_entries)
        r.flags = (c->p_req_cpu[p] == 0 && c->p_req_mem[p] == 0 && no_xres) ? 1u : 0u;
    }
    std::vector<int32_t> raw32(c->simon_raw.begin(), c->simon_raw.end());
    hipStream_t st = c->stream;
    // simon_fast.hip: <= 32 node classes, no zero-capacity node; NZEQ when NonZeroRequested == Requested everywhere
    c->fast_ok = c->Cn <= 32 && (size_t)c->Cp * c->Cn * 8 <= 48 * 1024;
    c->nzeq = true;
    for (int j = 0; j < N; ++j) {
        if (a_cpu[j] == 0 || a_mem[j] == 0) c->fast_ok = false;
        if (rqc[j] != nzc[j] || rqm[j] != nzm[j]) c->nzeq = false;
    }
    std::vector<PodRowF> rowsF(P);
    for (int p = 0; p < P; ++p) {
        const PodRowN& r = rows[p];
        rowsF[p] = PodRowF{(double)r.req_cpu, (double)r.req_mem, (double)r.nz_cpu, (double)r.nz_mem, r.cls, r.preset, r.gate, r.flags};
        if (r.req_cpu != r.nz_cpu || r.req_mem != r.nz_mem) c->nzeq = false;
    }
    // simon_table.hip: intern pod request signatures and internal node classes
    bool nozero = true;
    for (int j = 0; j < N; ++j) if (a_cpu[j] == 0 || a_mem[j] == 0) nozero = false;
    c->table_ok = nozero && N <= kTableMaxNodesCoarse;
    if (c->table_ok) {
        // Table class of a pod class = its CONTENT: (static-mask row, Simon raw row).  Workload expansion hands over one pod class
        // per template (thousands with anti-affinity groups or DaemonSets) of which few differ in what this kernel reads, and a
        // request signature is (requests, table class).
        const size_t words = (size_t)(N + 63) / 64;
        std::map<std::pair<std::vector<uint64_t>, std::vector<int32_t>>, int> tc_id;
        std::vector<int32_t> tc_of(c->Cp), tc_rep;
        for (int cp = 0; cp < c->Cp; ++cp) {
            std::vector<uint64_t> mrow;
            if (c->has_mask) mrow.assign(c->static_mask.begin() + (size_t)cp * words, c->static_mask.begin() + (size_t)(cp + 1) * words);
            std::vector<int32_t> rrow(raw32.begin() + (size_t)cp * c->Cn, raw32.begin() + (size_t)(cp + 1) * c->Cn);
            for (const std::vector<int64_t>* tab : {&c->na_raw, &c->tt_raw, &c->static_add})       // static score rows are content too
                if (!tab->empty()) rrow.insert(rrow.end(), tab->begin() + (size_t)cp * c->Cn, tab->begin() + (size_t)(cp + 1) * c->Cn);
            img_row_append(c, cp, rrow);                               // ... and so are the image score rows of every size of the batch
            auto it = tc_id.emplace(std::make_pair(std::move(mrow), std::move(rrow)), (int)tc_rep.size());
            if (it.second) tc_rep.push_back(cp);
            tc_of[cp] = it.first->second;
        }
        const int Ctc = (int)tc_rep.size();
        std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, int32_t, uint32_t, int32_t, uint32_t, int32_t>, int> sig_id;
        std::vector<SigRow> sigs;
        std::vector<int32_t> sig_fc;          // fold: filter class of a signature
        std::vector<PodRowC> rowsC(P);
        for (int p = 0; p < P && c->table_ok; ++p) {
            const PodRowN& r = rows[p];
            const int32_t tc = tc_of[r.cls];
            const int32_t fc = c->fold ? c->fold_fc[r.cls] : 0;
            // GPU fold: the (gpu-mem per device in gcd units, device count) request is part of the signature
            const bool gp = c->gfold && c->p_gpu_mem[p] > 0;
            const uint32_t gq = gp ? (uint32_t)((uint64_t)c->p_gpu_mem[p] / c->g_gpu) : 0u;
            const int32_t gn = gp ? std::min(c->p_gpu_cnt[p], 64) : 0;
            auto key = std::make_tuple(r.req_cpu, r.req_mem, r.nz_cpu, r.nz_mem, tc, r.flags, fc, gq, gn);
            auto it = sig_id.find(key);
            if (it == sig_id.end()) {
                if ((int)sigs.size() == kTableMaxSigs) { c->table_ok = false; break; }
                it = sig_id.emplace(key, (int)sigs.size()).first;
                SigRow sr{};
                sr.req_c = r.req_cpu; sr.req_m = r.req_mem; sr.nz_c = r.nz_cpu; sr.nz_m = r.nz_mem; sr.cls = tc; sr.flags = r.flags;
                sr.pad[0] = (int32_t)gq; sr.pad[1] = gp ? (gn > 0 ? gn : -1) : 0;      // (pad[1] != 0 marks a GPU signature; a request without devices fits nowhere)
                sigs.push_back(sr);
                sig_fc.push_back(fc);
            }
            rowsC[p] = PodRowC{it->second | (tc << 10), (!c->p_pin.empty() && c->p_pin[p] >= 0) ? -2 - c->p_pin[p] : r.preset, r.gate, 0};
        }
        // 65 .. 128 signatures: the kernel keeps two per lane (k and k + 64).  When every signature of the upper half can sit 64 slots
        // above a TWIN -- the same request under another table class -- the kernel evaluates a lane's node byte once for both
        // (TableScalars::static_tables & kStTwins; config 5: 42 request shapes x 2 table classes).  A permutation of the ids, nothing else.
        c->sig_twins = false;
        if (c->gfold && (int)sigs.size() > kTableMaxSigs) c->table_ok = false;      // (gfold_supported counted them: cannot happen)
        if (c->table_ok && !c->no_sig_twins && !c->gfold && sigs.size() > 64 && sigs.size() <= 128) {
            const int K = (int)sigs.size(), n_hi = K - 64;
            std::map<std::tuple<double, double, double, double, uint32_t>, std::vector<int>> by_shape;
            for (int k = 0; k < K; ++k) by_shape[std::make_tuple(sigs[k].req_c, sigs[k].req_m, sigs[k].nz_c, sigs[k].nz_m, sigs[k].flags)].push_back(k);
            std::vector<int> slot_of(K, -1), lo_rest;
            int paired = 0;
            for (auto& kv : by_shape) {
                std::vector<int>& v = kv.second;
                size_t i = 0;
                for (; i + 1 < v.size() && paired < n_hi; i += 2, ++paired) { slot_of[v[i]] = paired; slot_of[v[i + 1]] = 64 + paired; }
                for (; i < v.size(); ++i) lo_rest.push_back(v[i]);
            }
            if (paired == n_hi) {
                int next = n_hi;
                for (int k : lo_rest) slot_of[k] = next++;
                std::vector<SigRow> moved(K);
                std::vector<int32_t> moved_fc(K);
                for (int k = 0; k < K; ++k) { moved[slot_of[k]] = sigs[k]; moved_fc[slot_of[k]] = sig_fc[k]; }
                sigs.swap(moved); sig_fc.swap(moved_fc);
                for (int p = 0; p < P; ++p) rowsC[p].sigcls = (rowsC[p].sigcls & ~0x3FF) | slot_of[rowsC[p].sigcls & 0x3FF];
                c->sig_twins = true;
            }
        }
        // REST descriptors: term class (which mask rows a pod must find clear / sets) and GPU signature of every pod
        std::vector<int32_t> xrows;           // entries of every term class: filter row | set row << 16
        std::vector<uint2> gsigs;
        std::vector<uint32_t> xsigs;          // [X][8]
        c->rest_M = c->rest_G = c->rest_X = 0;
        if (c->rest && c->table_ok) {
            std::map<std::pair<uint32_t, int32_t>, int> gs_id;
            std::vector<int> gs_of(P, -1);
            for (int p = 0; p < P; ++p) {
                if (!c->has_gpu || c->p_gpu_mem[p] <= 0) continue;
                const auto key = std::make_pair((uint32_t)((uint64_t)c->p_gpu_mem[p] / c->g_gpu), (int32_t)std::min(c->p_gpu_cnt[p], 64));
                auto it = gs_id.emplace(key, (int)gsigs.size());
                if (it.second) gsigs.push_back(make_uint2(key.first, (unsigned)key.second));
                gs_of[p] = it.first->second;
            }
            std::map<std::vector<uint32_t>, int> xs_id;
            std::vector<int> xs_of(P, -1);
            for (int p = 0; p < P && c->xres; ++p) {
                std::vector<uint32_t> key(8, 0);
                key[0] = (uint32_t)((uint64_t)c->p_req_eph[p] / c->g_eph);
                bool any = key[0] != 0;
                for (int k = 0; k < c->K; ++k) { key[1 + k] = (uint32_t)c->p_scalar[(size_t)k * P + p]; any = any || key[1 + k] != 0; }
                if (!any) continue;
                auto it = xs_id.emplace(key, (int)xs_id.size());
                if (it.second) xsigs.insert(xsigs.end(), key.begin(), key.end());
                xs_of[p] = it.first->second;
            }
            const int Xn = (int)xs_id.size();
            // REST && SPREAD: the match lists also name the terms the spread constraints count -- rows nobody ever tests (and on a zone-like
            // key a set-row costs a pass over the scenario's blocks per landing pod): only the terms some class holds AGAINST others get
            // rows there (tm: term -> its row pair), so a cluster of hundreds of Services next to a few anti-affinity terms fits
            std::vector<char> row_read(std::max(c->Tm, 1), c->rs ? 0 : 1);
            if (c->rs)
                for (int cp = 0; cp < c->Cp; ++cp) {
                    for (int e = c->anti_off.empty() ? 0 : c->anti_off[cp]; !c->anti_off.empty() && e < c->anti_off[cp + 1]; ++e) row_read[c->anti_idx[e]] = 1;
                    for (int e = c->port_off.empty() ? 0 : c->port_off[cp]; !c->port_off.empty() && e < c->port_off[cp + 1]; ++e) row_read[c->port_idx[e]] = 1;
                    for (int e = c->aff_off.empty() ? 0 : c->aff_off[cp]; !c->aff_off.empty() && e < c->aff_off[cp + 1]; ++e) row_read[c->aff_idx[e]] = 1;
                }
            std::vector<int> tm(std::max(c->Tm, 1), 0);
            int n_rows_t = 0;
            for (int t = 0; t < c->Tm; ++t) if (row_read[t]) tm[t] = n_rows_t++;
            const int G = (int)gsigs.size(), T = n_rows_t, B = G + Xn;       // term rows start behind the request rows
            const int NZk = (int)c->zone_keys.size(), SCR = B + 2 * T, LBL = SCR + 1;
            // rows: requests | "a pod MATCHING t is here" | "a pod REQUIRING t is here" | scratch (set by entries that set nothing,
            // never read) | per zone-like key "the node lacks the label"
            c->rest_G = G; c->rest_X = Xn; c->rest_M = LBL + NZk;
            std::map<std::pair<std::vector<int32_t>, std::vector<int32_t>>, int> xc_id;   // -> n | offset << 6
            std::vector<int> xc_of(c->Cp, 0);

            for (int cp = 0; cp < c->Cp && T > 0; ++cp) {
                std::vector<int32_t> anti(c->anti_idx.begin() + c->anti_off[cp], c->anti_idx.begin() + c->anti_off[cp + 1]);
                std::vector<int32_t> match(c->match_idx.begin() + c->match_off[cp], c->match_idx.begin() + c->match_off[cp + 1]);
                std::vector<int32_t> aff;      // required affinity (filtering.go:348-377): DERIVED terms, in the class's order
                if (!c->aff_off.empty()) aff.assign(c->aff_idx.begin() + c->aff_off[cp], c->aff_idx.begin() + c->aff_off[cp + 1]);
                std::sort(aff.begin(), aff.end()); aff.erase(std::unique(aff.begin(), aff.end()), aff.end());
                const bool aff_self = !aff.empty() && !c->class_flags.empty() && (c->class_flags[cp] & SIMON_CLASS_AFF_SELF);
                std::vector<int32_t> port;     // NodePorts (node_ports.go:104-127): port terms this class CONFLICTS with
                if (!c->port_off.empty()) port.assign(c->port_idx.begin() + c->port_off[cp], c->port_idx.begin() + c->port_off[cp + 1]);
                std::sort(anti.begin(), anti.end()); anti.erase(std::unique(anti.begin(), anti.end()), anti.end());
                std::sort(match.begin(), match.end()); match.erase(std::unique(match.begin(), match.end()), match.end());
                match.erase(std::remove_if(match.begin(), match.end(), [&](int32_t t) { return !row_read[t]; }), match.end());
                std::sort(port.begin(), port.end()); port.erase(std::unique(port.begin(), port.end()), port.end());
                if (anti.empty() && match.empty() && port.empty() && aff.empty()) continue;
                size_t n_lbl = 0;              // one label entry per zone-like key among the affinity terms
                { std::set<int> zk; for (int t : aff) if (c->key_zslot[c->term_key[t]] >= 0) zk.insert(c->key_zslot[c->term_key[t]]); n_lbl = zk.size(); }
                const size_t n = anti.size() + match.size() + port.size() + aff.size() + n_lbl, off = xrows.size();
                if (n > 63 || off + n >= (1u << 14)) { c->table_ok = false; break; }   // one lane per entry; 14-bit offsets
                std::vector<int32_t> anti_key = anti;       // key: (anti list, -1, port list), match list
                anti_key.push_back(-1); anti_key.insert(anti_key.end(), port.begin(), port.end());
                anti_key.push_back(aff_self ? -3 : -2); anti_key.insert(anti_key.end(), aff.begin(), aff.end());
                auto it = xc_id.emplace(std::make_pair(anti_key, match), (int)(n | (off << 6)));
                if (it.second) {
                    // filter (filtering.go:319-346): a placed pod MATCHES one of my anti terms (row B + t), or a placed pod
                    // REQUIRES a term that matches me (row B + T + t); AddPod sets the mirror rows (oracle/simon_oracle.c: add_pod)
                    // bits 28..30: zone key + 1 of the term (the set-row then covers every position of the pod's domain)
                    auto zs = [&](int t) { return (unsigned)(c->key_zslot[c->term_key[t]] + 1) << 28; };
                    for (int t : anti) xrows.push_back((int)((unsigned)(B + tm[t]) | ((unsigned)(B + T + tm[t]) << 16) | zs(t)));
                    for (int t : match) xrows.push_back((int)((unsigned)(B + T + tm[t]) | ((unsigned)(B + tm[t]) << 16) | zs(t)));
                    // a conflicting port is in use on the node: a placed pod MATCHES (binds) port term t; nothing to set -- the
                    // entry's set-row repeats a row the class sets anyway, or a scratch row behind the last term row
                    for (int t : port) xrows.push_back((B + tm[t]) | (SCR << 16));
                    // required affinity: row B + t must be SET (bit 31; bit 27: the class matches its own terms -- the first-pod
                    // escape); on a zone-like key the node must carry the label whatever the escape says (label row, plain entry)
                    std::set<int> zk;
                    for (int t : aff) {
                        xrows.push_back((int)((unsigned)(B + tm[t]) | ((unsigned)SCR << 16) | (aff_self ? 1u << 27 : 0u) | (1u << 31)));
                        const int z = c->key_zslot[c->term_key[t]];
                        if (z >= 0 && zk.insert(z).second) xrows.push_back((LBL + z) | (SCR << 16));
                    }
                }
                xc_of[cp] = it.first->second;
            }
            bool any_rest = false;
            for (int p = 0; p < P; ++p) {
                rowsC[p].rest = (gs_of[p] + 1) | ((xs_of[p] + 1) << 6) | (int)((unsigned)xc_of[c->p_cls[p]] << 12);
                any_rest = any_rest || rowsC[p].rest != 0;
            }
            // GPU nodes without a GPU pod, terms no pod of the stream carries: nothing for the REST path to do -- generations 4 / 5
            // run the batch (their cycle is 17 % shorter than the REST instantiation's, profiles/README.md)
            if (!any_rest && c->table_ok) { c->rest = false; c->rs = false; c->rest_M = c->rest_G = c->rest_X = 0; }
        }
        // SPREAD descriptors: per pod class its soft constraints (term | maxSkew << 16 | dup << 30), the terms with a counter row its pods
        // are COUNTED on (term | multiplicity << 16) and the entries of its InterPodAffinity raw score (coefficient; the hostname-like term
        // first), interned by content; every entry travels with its term; PodRowC::rest = soft | counted << 3 | preferred << 10 | offset << 13
        std::vector<int32_t> sp_ent, sp_ent_term;
        if (c->spread && c->table_ok) {
            std::map<std::vector<int32_t>, int> sc_id;
            std::vector<int> desc_of(c->Cp, 0);
            for (int cp = 0; cp < c->Cp; ++cp) {
                std::vector<int32_t> ent, ent_term;
                const int ns = c->ss_idx.empty() ? 0 : c->ss_off[cp + 1] - c->ss_off[cp];
                for (int e = c->ss_idx.empty() ? 0 : c->ss_off[cp]; !c->ss_idx.empty() && e < c->ss_off[cp + 1]; ++e) {
                    ent.push_back(c->ss_idx[e] | ((c->ss_skew[e] & 0x3FFF) << 16) | ((c->ss_skew[e] & SIMON_SPREAD_DUP_KEY) ? 1 << 30 : 0));
                    ent_term.push_back(c->ss_idx[e]);
                }
                std::map<int, int> mult;                                   // per counter ROW (terms that share one count once)
                if (!c->match_off.empty()) {
                    std::map<int, int> per_term;
                    for (int e = c->match_off[cp]; e < c->match_off[cp + 1]; ++e) if (c->sp_kind[c->match_idx[e]]) ++per_term[c->match_idx[e]];
                    for (auto& kv : per_term) mult[c->sp_rep[kv.first]] = kv.second;
                }
                if (c->ipa_fold && !c->own_off.empty()) {                 // rows that count the class's pods as OWNERS of a scoring term (one per pod)
                    std::map<int, long long> os;
                    for (int e = c->own_off[cp]; e < c->own_off[cp + 1]; ++e) os[c->own_idx[e]] += c->own_w[e];
                    for (auto& kv : os) if (kv.second != 0 && c->sp_kind[(size_t)c->Tm + kv.first]) mult[c->sp_rep[(size_t)c->Tm + kv.first]] = 1;
                }
                for (auto& kv : mult) { ent.push_back((kv.first & 0xFFFF) | (kv.second << 16)); ent_term.push_back(kv.first); }
                int n_ipa = 0;
                if (c->ipa_fold) {
                    if (c->ipa_h_term[cp] >= 0) { ent.push_back(c->ipa_h_w[cp]); ent_term.push_back(c->ipa_h_term[cp]); ++n_ipa; }
                    for (auto& zt : c->ipa_z[cp]) { ent.push_back(zt.second); ent_term.push_back(zt.first); ++n_ipa; }
                }
                int n_hard = 0;
                if (c->hard_fold)
                    for (int e = c->sh_off[cp]; e < c->sh_off[cp + 1]; ++e, ++n_hard) {
                        ent.push_back((c->sh_skew[e] & 0x3FFF) | ((!c->sh_self.empty() && c->sh_self[e]) ? 1 << 14 : 0));
                        ent_term.push_back(c->sh_idx[e]);
                    }
                if (ent.empty()) continue;
                std::vector<int32_t> key = ent;                            // (entries of different kinds can spell the same word)
                key.insert(key.end(), ent_term.begin(), ent_term.end());
                key.push_back(ns); key.push_back(n_ipa); key.push_back(n_hard);
                auto it = sc_id.find(key);
                if (it == sc_id.end()) {
                    if (sp_ent.size() + ent.size() >= (1u << 16)) { c->table_ok = false; break; }
                    it = sc_id.emplace(key, ns | ((int)mult.size() << 3) | (n_ipa << 10) | (n_hard << 13) | ((int)sp_ent.size() << 15)).first;
                    sp_ent.insert(sp_ent.end(), ent.begin(), ent.end());
                    sp_ent_term.insert(sp_ent_term.end(), ent_term.begin(), ent_term.end());
                }
                desc_of[cp] = it->second;
            }
            if (c->rs) {                                                   // PodRowC::rest keeps the REST descriptor: the SPREAD word travels by pod id
                std::vector<int32_t> spw(std::max(P, 1), 0);
                for (int p = 0; p < P; ++p) spw[p] = desc_of[c->p_cls[p]];
                HIP_TRY(c, c->d_sp_word.upload(spw, st));
            } else {
                for (int p = 0; p < P && c->table_ok; ++p) rowsC[p].rest = desc_of[c->p_cls[p]];
            }
            if (c->Tm >= (1 << 16)) c->table_ok = false;
        }
        // Internal node class = (caller's node class, allocatable cpu, allocatable memory).  The caller's classes share their
        // allocatable by contract (include/simon_hip.h), so normally this IS the caller's partition; splitting a class that
        // does not keeps the kernel's "shape follows from class" exact for any input.
        // With GPU requests in the stream (REST) a class is also split into its nodes with and without devices when that fits: a GPU
        // request then excludes the units of a device-less class as a whole (one compare per 64 positions in rest_select) and a
        // class with devices holds candidates only.
        // SPREAD: a class is also split by the domains of the zone-like keys of the soft spread terms (sub = the domains, 5 bits each, 0 =
        // the label is missing): a summary unit then has ONE zone term and "which zones hold a scored node" follows from the feasible-node
        // counters per (signature, class).
        // The caller's node classes are interned by CONTENT first -- the class's column of every (pod class, node class) table the kernel
        // reads (Simon raw score, NodeAffinity preferred, TaintToleration PreferNoSchedule, weighted additions), over the table classes in
        // use.  A host that derives node classes from label / taint sets hands over hundreds (464 in profiles/e2e_sweep.py's mix of 3
        // capacities) of which few differ in those columns; the static filters are per node (static_mask), not per class.
        // (SIMON_TABLE_NO_CLASS_CONTENT=1: the caller's ids as they come -- A/B and tests.)
        std::vector<int32_t> content_of(std::max(c->Cn, 1));
        {
            std::map<std::vector<int32_t>, int> col_id;
            for (int nc = 0; nc < c->Cn; ++nc) {
                if (c->no_class_content) { content_of[nc] = nc; continue; }
                std::vector<int32_t> col;
                col.reserve((size_t)Ctc * 4);
                for (int tc = 0; tc < Ctc; ++tc) {
                    col.push_back(raw32[(size_t)tc_rep[tc] * c->Cn + nc]);
                    for (const std::vector<int64_t>* tab : {&c->na_raw, &c->tt_raw, &c->static_add})
                        if (!tab->empty()) col.push_back((int32_t)(*tab)[(size_t)tc_rep[tc] * c->Cn + nc]);
                    const int ir = c->img_R ? c->img_row_of[tc_rep[tc]] : -1;   // ImageLocality: the class's score column for every size of the batch
                    for (size_t t = 0; ir >= 0 && t < c->img_slots(); ++t)
                        col.push_back(c->img_cls[(t * c->img_R + ir) * c->Cn + nc]);
                }
                content_of[nc] = col_id.emplace(std::move(col), (int)col_id.size()).first->second;
            }
        }
        std::map<std::tuple<int32_t, uint32_t, uint32_t, int>, int> cls_id;
        std::vector<ShapeRow> shapes;
        std::vector<int32_t> orig_of, ncls_t(N), sub_of_class;
        bool split_gpu = c->rest && !c->spread && c->has_gpu && c->rest_G > 0 && !c->gpu_cnt.empty() && !c->no_gpu_split;
        if (split_gpu) {
            std::set<std::tuple<int32_t, uint32_t, uint32_t, int>> keys;
            for (int j = 0; j < N; ++j) keys.insert(std::make_tuple(content_of[c->node_class[j]], a_cpu[j], a_mem[j], c->gpu_cnt[j] > 0 ? 1 : 0));
            split_gpu = (int)keys.size() <= kTableMaxClasses;        // (the split is an optimisation: never at the price of the second class per lane)
        }
        auto zone_sub = [&](int j) -> int {
            int sub = 0;
            for (size_t z = 0; z < c->sp_zkeys.size(); ++z) sub |= (c->topo_dom[(size_t)c->sp_zkeys[z] * N + j] + 1) << (5 * z);
            return sub;
        };
        for (int j = 0; j < N && c->table_ok; ++j) {
            auto key = std::make_tuple(content_of[c->node_class[j]], a_cpu[j], a_mem[j], c->spread ? zone_sub(j) : (split_gpu && c->gpu_cnt[j] > 0) ? 1 : 0);
            auto it = cls_id.find(key);
            if (it == cls_id.end()) {
                // two classes per lane in the REST select and in the SPREAD walks beyond 64 (round 6, simon_table.hip: CN2), as in the
                // instantiations without rows and walks
                const int cls_max = (c->rest || c->spread) ? ((c->no_cn2 || c->rs) ? kTableMaxClasses : kTableMaxClassesSpread) : kTableMaxClassesPlain;
                if ((int)shapes.size() == cls_max) { c->table_ok = false; break; }
                it = cls_id.emplace(key, (int)shapes.size()).first;
                ShapeRow sh{};
                sh.cap_c = (double)a_cpu[j]; sh.cap_m = (double)a_mem[j];
                sh.rc_c = 1.0 / sh.cap_c; sh.rc_m = 1.0 / sh.cap_m;           // IEEE, as the device's correctly rounded '/'
                sh.rc100_c = 100.0 * sh.rc_c; sh.rc100_m = 100.0 * sh.rc_m;
                shapes.push_back(sh);
                orig_of.push_back(c->node_class[j]);
                sub_of_class.push_back(std::get<3>(key));
            }
            ncls_t[j] = it->second;
        }
        if (c->table_ok && c->spread && (int)shapes.size() > kTableMaxClasses && sigs.size() > 128) c->table_ok = false;   // (CN2 serves <= 128 signatures)
        if (c->table_ok && c->rest && (int)shapes.size() > kTableMaxClasses && sigs.size() > 128) c->table_ok = false;        // (... and so does the second class per lane of the REST select)
        if (c->table_ok) {
            const int Ct = (int)shapes.size();
            c->n_sigs = (int)sigs.size(); c->Cn_t = Ct;
            if (sigs.empty()) sigs.push_back(SigRow{});
            std::vector<int32_t> raw_t((size_t)Ctc * Ct);
            for (int tc = 0; tc < Ctc; ++tc)
                for (int d = 0; d < Ct; ++d) raw_t[(size_t)tc * Ct + d] = raw32[(size_t)tc_rep[tc] * c->Cn + orig_of[d]];
            for (auto [tab, buf] : {std::make_pair(&c->na_raw, &c->d_t_na), std::make_pair(&c->tt_raw, &c->d_t_tt), std::make_pair(&c->static_add, &c->d_t_add)}) {
                if (tab->empty()) continue;
                std::vector<int32_t> t((size_t)Ctc * Ct);
                for (int tc = 0; tc < Ctc; ++tc)
                    for (int d = 0; d < Ct; ++d) t[(size_t)tc * Ct + d] = (int32_t)(*tab)[(size_t)tc_rep[tc] * c->Cn + orig_of[d]];
                HIP_TRY(c, buf->upload(t, st));
            }
            if (c->img_R > 0) {                                       // ImageLocality: [slot][table class][internal node class]
                const size_t nslot = std::max<size_t>(c->img_slots(), 1);
                std::vector<unsigned char> img_t(nslot * Ctc * Ct, 0);
                for (size_t t = 0; t < c->img_slots(); ++t)
                    for (int tc = 0; tc < Ctc; ++tc) {
                        const int ir = c->img_row_of[tc_rep[tc]];
                        if (ir < 0) continue;
                        for (int d = 0; d < Ct; ++d) img_t[(t * Ctc + tc) * Ct + d] = c->img_cls[(t * c->img_R + ir) * c->Cn + orig_of[d]];
                    }
                HIP_TRY(c, c->d_t_img.upload(img_t, st));
                HIP_TRY(c, hipStreamSynchronize(st));                  // (img_t dies at the end of this block)
                c->img_stride_t = Ctc * Ct;
                c->h_tc_of = tc_of; c->t_img_staged = true;
            }
            if (c->has_mask) {
                std::vector<uint64_t> mask_t((size_t)Ctc * words);
                for (int tc = 0; tc < Ctc; ++tc)
                    std::copy(c->static_mask.begin() + (size_t)tc_rep[tc] * words, c->static_mask.begin() + (size_t)(tc_rep[tc] + 1) * words, mask_t.begin() + (size_t)tc * words);
                HIP_TRY(c, c->d_t_mask.upload(mask_t, st));
            }
            // class-major layout: rank of a node among its class, per-class node lists in canonical order, class counts of
            // every prefix of the pool (a scenario = a prefix)
            std::vector<int32_t> rank(N), prefix((size_t)(N + 1) * Ct, 0), cls_off(Ct + 1, 0), cls_list((size_t)N + 64, 0);   // (+ 64: generation 7 reads a whole unit of the last, padded class)
            for (int j = 0; j < N; ++j) {
                const int d = ncls_t[j];
                rank[j] = prefix[(size_t)j * Ct + d];
                for (int e = 0; e < Ct; ++e) prefix[(size_t)(j + 1) * Ct + e] = prefix[(size_t)j * Ct + e] + (e == d);
            }
            for (int d = 0; d < Ct; ++d) cls_off[d + 1] = cls_off[d] + prefix[(size_t)N * Ct + d];
            for (int j = 0; j < N; ++j) cls_list[cls_off[ncls_t[j]] + rank[j]] = j;
            c->h_clsprefix = prefix;
            c->h_ncls_t = ncls_t; c->h_cls_off = cls_off;
            HIP_TRY(c, c->d_sigs.upload(sigs, st));
            if (c->fold) {                                            // which signatures a landing signature excludes from its node
                const int K = (int)sigs.size(), KW = (K + 31) / 32;
                std::vector<uint32_t> fx((size_t)K * KW, 0u);
                for (int L = 0; L < K; ++L)
                    for (int S = 0; S < K; ++S)
                        if (c->fold_x[(size_t)sig_fc[L] * c->fold_FC + sig_fc[S]]) fx[(size_t)L * KW + (S >> 5)] |= 1u << (S & 31);
                HIP_TRY(c, c->d_foldx.upload(fx, st));
            }
            HIP_TRY(c, c->d_shapes.upload(shapes, st));
            HIP_TRY(c, c->d_podsC.upload(rowsC, st));
            HIP_TRY(c, c->d_t_ncls.upload(ncls_t, st));
            HIP_TRY(c, c->d_t_raw.upload(raw_t, st));
            HIP_TRY(c, c->d_rank.upload(rank, st));
            HIP_TRY(c, c->d_clsprefix.upload(prefix, st));
            HIP_TRY(c, c->d_cls_list.upload(cls_list, st));
            HIP_TRY(c, c->d_cls_off.upload(cls_off, st));
            if (c->rest) {
                std::vector<uint32_t> devtot(N, 0), gused((size_t)N * 8, 0);
                for (int j = 0; j < N && c->has_gpu; ++j) {
                    if (c->gpu_cnt[j] > 0) devtot[j] = (uint32_t)((uint64_t)(c->gpu_mem_total[j] / c->gpu_cnt[j]) / c->g_gpu);
                    for (int d = 0; d < 8; ++d) gused[(size_t)j * 8 + d] = (uint32_t)((uint64_t)c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d] / c->g_gpu);
                }
                if (gsigs.empty()) gsigs.push_back(make_uint2(0, 0));
                if (xrows.empty()) xrows.push_back(0);
                std::vector<int32_t> gcnt(N, 0);
                if (c->has_gpu) gcnt = c->gpu_cnt;
                HIP_TRY(c, c->d_xrows.upload(xrows, st));
                std::vector<int32_t> zdom(std::max<size_t>(c->zone_keys.size(), 1) * N, -1);
                for (size_t z = 0; z < c->zone_keys.size(); ++z)
                    std::copy(c->topo_dom.begin() + (size_t)c->zone_keys[z] * N, c->topo_dom.begin() + (size_t)(c->zone_keys[z] + 1) * N, zdom.begin() + z * N);
                HIP_TRY(c, c->d_zdom.upload(zdom, st));
                std::vector<uint32_t> xalloc((size_t)N * 8, 0), xused((size_t)N * 8, 0);
                for (int j = 0; j < N && c->xres; ++j) {
                    xalloc[(size_t)j * 8] = (uint32_t)((uint64_t)c->alloc_eph[j] / c->g_eph);
                    xused[(size_t)j * 8] = (uint32_t)((uint64_t)c->i_req_eph[j] / c->g_eph);
                    for (int k = 0; k < c->K; ++k) {
                        xalloc[(size_t)j * 8 + 1 + k] = (uint32_t)c->scalar_alloc[(size_t)k * N + j];
                        xused[(size_t)j * 8 + 1 + k] = (uint32_t)c->i_scalar_req[(size_t)k * N + j];
                    }
                }
                if (xsigs.empty()) xsigs.assign(8, 0);
                HIP_TRY(c, c->d_xsig.upload(xsigs, st)); HIP_TRY(c, c->d_xalloc.upload(xalloc, st)); HIP_TRY(c, c->d_i_xused.upload(xused, st));
                HIP_TRY(c, c->d_gsig.upload(gsigs, st)); HIP_TRY(c, c->d_gpu_cnt.upload(gcnt, st));
                HIP_TRY(c, c->d_gpu_devtot.upload(devtot, st)); HIP_TRY(c, c->d_i_gused.upload(gused, st));
            }
            if (c->gfold && !c->rest) {                              // GPU fold: the pool's devices (the kernel keeps them per position)
                std::vector<uint32_t> devtot(N, 0), gused((size_t)N * 8, 0);
                for (int j = 0; j < N; ++j) {
                    if (c->gpu_cnt[j] > 0) devtot[j] = (uint32_t)((uint64_t)(c->gpu_mem_total[j] / c->gpu_cnt[j]) / c->g_gpu);
                    for (int d = 0; d < 8; ++d) gused[(size_t)j * 8 + d] = (uint32_t)((uint64_t)c->i_gpu_used[(size_t)j * SIMON_MAX_GPU_DEV + d] / c->g_gpu);
                }
                HIP_TRY(c, c->d_gpu_cnt.upload(c->gpu_cnt, st));
                HIP_TRY(c, c->d_gpu_devtot.upload(devtot, st)); HIP_TRY(c, c->d_i_gused.upload(gused, st));
            }
            if (c->spread) {
                std::vector<int32_t> sp_term(std::max(2 * c->Tm, 1), 0);      // ids Tm + t: rows that count the OWNERS of scoring term t (no node set)
                for (int id = 0; id < 2 * c->Tm; ++id)
                    sp_term[id] = c->sp_kind[id] | (c->sp_row[id] << 2) | (c->sp_zslot[id] << 16) | ((c->sp_set_eff[id] + 1) << 19);
                const int nzk = (int)c->sp_zkeys.size();
                std::vector<signed char> zdom((size_t)std::max(nzk, 1) * Ct, 0);
                for (int z = 0; z < nzk; ++z)
                    for (int d = 0; d < Ct; ++d) zdom[(size_t)z * Ct + d] = (signed char)(((sub_of_class[d] >> (5 * z)) & 31) - 1);
                if (sp_ent.empty()) { sp_ent.push_back(0); sp_ent_term.push_back(0); }
                std::vector<int32_t> sp_pairs(sp_ent.size() * 2);            // the term's row travels with the entry (one load in the kernel)
                for (size_t i = 0; i < sp_ent.size(); ++i) { sp_pairs[2 * i] = sp_ent[i]; sp_pairs[2 * i + 1] = sp_term[sp_ent_term[i]]; }
                std::vector<uint64_t> sets = c->node_sets;
                if (sets.empty()) sets.push_back(0);
                HIP_TRY(c, c->d_sp_ent.upload(sp_pairs, st));
                HIP_TRY(c, c->d_cls_zdom.upload(zdom, st));
                { std::vector<double> lg = c->spread_log; if (lg.empty()) lg.push_back(0.0); HIP_TRY(c, c->d_spread_log.upload(lg, st)); }
                HIP_TRY(c, c->d_node_sets.upload(sets, st));
            }
            HIP_TRY(c, hipStreamSynchronize(st));
        }
    }
    HIP_TRY(c, c->d_podsF.upload(rowsF, st));
    HIP_TRY(c, c->d_a_cpu.upload(a_cpu, st));
    HIP_TRY(c, c->d_a_mem.upload(a_mem, st));
    HIP_TRY(c, c->d_i_rq_cpu.upload(rqc, st));
    HIP_TRY(c, c->d_i_rq_mem.upload(rqm, st));
    HIP_TRY(c, c->d_i_nz_cpu.upload(nzc, st));
    HIP_TRY(c, c->d_i_nz_mem.upload(nzm, st));
    HIP_TRY(c, c->d_a_pods.upload(c->alloc_pods, st));
    HIP_TRY(c, c->d_ncls.upload(c->node_class, st));
    HIP_TRY(c, c->d_i_npods.upload(c->i_npods, st));
    HIP_TRY(c, c->d_podsN.upload(rows, st));
    HIP_TRY(c, c->d_raw32.upload(raw32, st));
    if (c->has_mask) HIP_TRY(c, c->d_mask.upload(c->static_mask, st));
    HIP_TRY(c, hipStreamSynchronize(st));  // staging vectors die at scope exit
    return SIMON_OK;
}

int stage(simon_ctx* c) {
    if (!(c->have_nodes && c->have_pods && c->have_tables))
        return fail(c, SIMON_ESTATE, "load nodes, pods and class tables before scenarios");
    if (c->staged) return SIMON_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // cross-validation of the three inputs
    for (int p = 0; p < c->P; ++p) {
        if (c->p_cls[p] < 0 || c->p_cls[p] >= c->Cp) return fail(c, SIMON_EINVAL, "pod %d: class %d out of range", p, c->p_cls[p]);
        if (c->p_preset[p] >= c->N) return fail(c, SIMON_EINVAL, "pod %d: preset node %d out of range", p, c->p_preset[p]);
    }
    for (int j = 0; j < c->N; ++j)
        if (c->node_class[j] < 0 || c->node_class[j] >= c->Cn) return fail(c, SIMON_EINVAL, "node %d: class out of range", j);
    if (c->has_mask && c->static_mask.size() != (size_t)c->Cp * ((c->N + 63) / 64))
        return fail(c, SIMON_EINVAL, "static_mask size mismatch");
    // derived per staging, never carried over from an earlier pod set: the pool's own GPU arrays, or a pod that asks for GPU memory
    // in a pool without them (every node then fails Open-Gpu-Share, :64-67)
    c->has_gpu = c->has_gpu_nodes;
    if (!c->has_gpu)
        for (int p = 0; p < c->P; ++p) if (c->p_gpu_mem[p] > 0) { c->has_gpu = true; break; }
    c->t_img_staged = false;
    if (const int rc = img_refine(c)) return rc;                    // (ABI v7: node classes split by image content, the batch's size slots or image states)
    if (c->debug_route && c->img_R > 0)
        fprintf(stderr, "[route] image split: %d node classes (caller %d), %d image-scoring pod classes, %zu %s\n", c->Cn,
                c->img_refined ? c->img_base_Cn : c->Cn, c->img_R, c->img_slots(), c->img_own_T > 0 ? "image states" : "sizes");
    choose_variant(c);
    if (c->variant != SIMON_KERNEL_NARROW) c->spread = false;         // (a later precondition sent the problem to the all-feature kernel)
    // prefix sums of allocatable for the occupancy caps (satisfyResourceSetting, apply.go:737-760)
    std::vector<int64_t> pc(c->N + 1, 0), pm(c->N + 1, 0);
    for (int j = 0; j < c->N; ++j) { pc[j + 1] = pc[j] + c->alloc_cpu[j]; pm[j + 1] = pm[j] + c->alloc_mem[j]; }
    c->prefix_vg.assign(c->N + 1, 0);
    for (int j = 0; j < c->N; ++j) {
        int64_t cap = 0;
        if (c->has_local && (c->l_flags[j] & 1))
            for (int q = 0; q < c->l_vg_cnt[j]; ++q) cap += c->l_vg_cap[(size_t)j * SIMON_MAX_VG + q];
        c->prefix_vg[j + 1] = c->prefix_vg[j] + cap;
    }
    c->prefix_cpu = pc; c->prefix_mem = pm;
    HIP_TRY(c, c->d_prefix_cpu.upload(pc, c->stream));
    HIP_TRY(c, c->d_prefix_mem.upload(pm, c->stream));
    HIP_TRY(c, c->d_prefix_vg.upload(c->prefix_vg, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->wide_staged = false;
    int rc = c->variant == SIMON_KERNEL_NARROW ? stage_narrow(c) : wide_stage(c->wide, *c, c->stream, c->err);
    if (rc) return rc;
    c->wide_staged = c->variant != SIMON_KERNEL_NARROW;
    c->staged = true;
    return SIMON_OK;
}

// ---- DefaultPreemption could have acted (ABI v6: simon_set_pod_priorities / simon_fetch_preempt_risk) ----------------------------------
// One wave per scenario walks the pods in scheduling order, 64 steps at a time: risk = some pod failed (SIMON_UNSCHEDULED) while a pod of
// LOWER priority was placed before it -- by the scheduler, by Spec.NodeName, or before the stream (init_min).  PostFilter runs only for a
// failed pod (V/scheduler.go:479) and selectVictimsOnNode only considers pods of lower priority (default_preemption.go:578-592): without
// such a pair no eviction can have happened in the reference and the scenario's result is exact.  HBM-bound: 12 B per pod-step.
__global__ __launch_bounds__(64) void preempt_risk_kernel_impl(const int32_t* __restrict__ place, const int32_t* __restrict__ orders,
                                                               const ScenarioDesc* __restrict__ scen, const int32_t* __restrict__ prio, int P,
                                                               int init_min, unsigned char* __restrict__ risk) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int32_t* __restrict__ order = orders + (size_t)scen[s].order_id * P;
    const int32_t* __restrict__ pl = place + (size_t)s * P;
    int runmin = init_min;
    bool bad = false;
    for (int i0 = 0; i0 < P; i0 += 64) {
        const int idx = i0 + lane;
        int placed_prio = 0x7fffffff, mine = 0;
        bool failed = false;
        if (idx < P) {
            const int pod = order[idx];
            const int v = pl[pod];
            mine = prio[pod];
            if (v >= 0) placed_prio = mine;
            failed = v == SIMON_UNSCHEDULED;
        }
        int inc = placed_prio;                                            // inclusive prefix minimum over the 64 steps
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off, 64);
            if (lane >= off) inc = t < inc ? t : inc;
        }
        int exc = __shfl_up(inc, 1, 64);
        if (lane == 0) exc = 0x7fffffff;
        exc = exc < runmin ? exc : runmin;                                // lowest priority among everything placed before this step
        bad = bad || (failed && mine > exc);
        const int last = __shfl(inc, 63, 64);
        runmin = last < runmin ? last : runmin;
    }
    const bool any = __ballot(bad) != 0ull;
    if (lane == 0) risk[s] = any ? 1 : 0;
}

// ---- min-plan reduction (pkg/apply/apply.go:203-259 + satisfyResourceSetting :689-775) --------
__global__ void plan_kernel(const ScenarioDesc* __restrict__ scen, int S, const int32_t* __restrict__ unsched,
                            const int64_t* __restrict__ used_cpu, const int64_t* __restrict__ used_mem,
                            const int64_t* __restrict__ prefix_cpu, const int64_t* __restrict__ prefix_mem, int max_cpu,
                            int max_mem, const int64_t* __restrict__ used_vg, const int64_t* __restrict__ prefix_vg, int max_vg,
                            const int64_t* __restrict__ seg_tot, unsigned long long* __restrict__ out) {
    unsigned long long best = ~0ull;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < S; s += gridDim.x * blockDim.x) {
        if (unsched[s] != 0) continue;
        const int n = scen[s].n_nodes;
        // int(float64(used.MilliValue()) / float64(alloc.MilliValue()) * 100), apply.go:759-760
        // segmented batch (seg_tot = [3][S]): the totals of the scenario's own nodes
        const int64_t ac = seg_tot ? seg_tot[s] : prefix_cpu[n], am = seg_tot ? seg_tot[S + s] : prefix_mem[n], av = seg_tot ? seg_tot[2 * S + s] : prefix_vg[n];
        const int cpu = (int)((double)used_cpu[s] / (double)ac * 100.0);
        const int mem = (int)((double)(used_mem[s] * 1000) / (double)(am * 1000) * 100.0);
        if (cpu > max_cpu || mem > max_mem) continue;
        if (used_vg && av != 0 &&                                // MaxVG, apply.go:767-771
            (int)((double)used_vg[s] / (double)av * 100.0) > max_vg) continue;
        const unsigned long long key = ((unsigned long long)(unsigned)n << 32) | (unsigned)s;
        best = key < best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(out, best);
}

// One thread behind plan_kernel: the winner's sums next to its key, so that simon_min_plan_vg reads ONE record back.
// rec = {key, used_cpu[s], used_mem[s], used_vg[s] (0 without local storage)}; without a plan only the key (~0) is meaningful.
__global__ void plan_record_kernel(const int64_t* __restrict__ used_cpu, const int64_t* __restrict__ used_mem,
                                   const int64_t* __restrict__ used_vg, unsigned long long* __restrict__ rec) {
    const unsigned long long key = rec[0];
    if (key == ~0ull) return;
    const unsigned s = (unsigned)(key & 0xFFFFFFFFu);
    rec[1] = (unsigned long long)used_cpu[s];
    rec[2] = (unsigned long long)used_mem[s];
    rec[3] = used_vg ? (unsigned long long)used_vg[s] : 0ull;
}

// simon_batch_out as the caller filled it, widened to the current layout: a v3 struct (no gpu_slices member) reads as gpu_slices = NULL
bool batch_out_view(const simon_batch_out* out, simon_batch_out* v) {
    if (out->struct_size == sizeof(simon_batch_out)) { *v = *out; return true; }
    if (out->struct_size != SIMON_BATCH_OUT_SIZE_V3) return false;
    std::memset(v, 0, sizeof *v);
    std::memcpy(v, out, SIMON_BATCH_OUT_SIZE_V3);
    v->struct_size = sizeof *v;
    return true;
}

// the kernel launches of a run between the context's event pair (simon_stats.kernel_ms); launch() returns a SIMON_* code
template <class F>
int timed_launch(simon_ctx* c, F&& launch) {
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if (int rc = launch()) return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    return SIMON_OK;
}

// the pool, state, stream and result pointers FastLaunch and NarrowArgs share (generations 2 and 1; a.pods is each kernel's own row format)
template <class Args>
void fill_register_args(const simon_ctx* c, bool want_placement, Args& a) {
    a.a_cpu = c->d_a_cpu.p; a.a_mem = c->d_a_mem.p; a.a_pods = c->d_a_pods.p; a.ncls = c->d_ncls.p;
    a.i_rq_cpu = c->d_i_rq_cpu.p; a.i_rq_mem = c->d_i_rq_mem.p; a.i_nz_cpu = c->d_i_nz_cpu.p; a.i_nz_mem = c->d_i_nz_mem.p;
    a.i_npods = c->d_i_npods.p; a.orders = c->d_orders.p; a.scen = c->d_scen.p; a.perm = c->d_perm.p;
    a.static_mask = c->has_mask ? c->d_mask.p : nullptr; a.simon_raw = c->d_raw32.p;
    a.unscheduled = c->d_unsched.p; a.used_cpu = c->d_used_cpu.p; a.used_mem = c->d_used_mem.p;
    a.placement = want_placement ? c->d_place.p : nullptr;
}

// the presence rows of a pod-subset batch (simon_set_scenario_pods), or null
inline const uint32_t* pod_rows(const simon_ctx* c) { return c->pods_on ? c->d_pod_words.p : nullptr; }

}  // namespace

// ============================================================================================
extern "C" {

int simon_hip_version(void) { return SIMON_HIP_ABI_VERSION; }

int simon_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

simon_ctx* simon_ctx_create(int device_id) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) return nullptr;
    if (hipSetDevice(device_id) != hipSuccess) return nullptr;
    simon_ctx* c = new (std::nothrow) simon_ctx();
    if (!c) return nullptr;
    c->device = device_id;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        delete c;
        return nullptr;
    }
    { int n_cu = 0; if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && n_cu > 0) c->n_cus = n_cu; }
    // Tuning / experiment knobs: every environment variable is read HERE, once per context; none changes a result.
    if (const char* e = getenv("SIMON_WG")) c->force_T = atoi(e);
    if (const char* e = getenv("SIMON_RCP_DIV")) c->rcp_div = atoi(e) != 0;
    if (const char* e = getenv("SIMON_NARROW_V1")) c->force_v1 = atoi(e) != 0;
    if (const char* e = getenv("SIMON_NO_CACHE")) c->no_cache = atoi(e) != 0;
    if (const char* e = getenv("SIMON_FORCE_WIDE")) c->force_wide = e[0] == '1';
    if (const char* e = getenv("SIMON_TABLE_COARSE")) c->force_coarse = atoi(e) != 0;
    c->no_rest = getenv("SIMON_NO_REST") != nullptr;
    c->no_fold = getenv("SIMON_NO_FOLD") != nullptr;                  // A/B + tests: anti-affinity / ports through the position masks (or the all-feature kernel)
    c->no_sig_twins = getenv("SIMON_TABLE_NO_TWINS") != nullptr;      // A/B: signature ids in order of appearance
    c->no_hard_fold = getenv("SIMON_NO_HARD_FOLD") != nullptr;        // A/B + tests: hard spread constraints always on the all-feature kernel
    c->no_cn2 = getenv("SIMON_NO_CN2") != nullptr;
    c->no_rs = getenv("SIMON_NO_RS") != nullptr;
    c->no_ipa_fold = getenv("SIMON_NO_IPA_FOLD") != nullptr;          // A/B + tests: preferred pod (anti-)affinity always on the all-feature kernel
    c->no_spread = getenv("SIMON_NO_SPREAD") != nullptr;              // A/B + tests: soft spread constraints on the all-feature kernel
    if (const char* e = getenv("SIMON_TEAM")) { const int v = atoi(e); c->team_mode = v == 0 ? 0 : (v == 1 || v == kTeamWaves) ? 1 : -1; }
    if (const char* e = getenv("SIMON_TEAM_MAX_S")) c->team_max_s = atoi(e);
    if (const char* e = getenv("SIMON_LDS_WS")) c->ldsws_mode = atoi(e) ? 1 : 0;
    c->no_gpu_split = getenv("SIMON_TABLE_NO_GPU_SPLIT") != nullptr;
    c->no_class_content = getenv("SIMON_TABLE_NO_CLASS_CONTENT") != nullptr;
    c->no_gpu_fold = getenv("SIMON_NO_GPU_FOLD") != nullptr;
    c->no_shared_prologue = getenv("SIMON_NO_SHARED_PROLOGUE") != nullptr;
    c->no_size_dispatch = getenv("SIMON_NO_SIZE_DISPATCH") != nullptr;
    if (const char* e = getenv("SIMON_SUBSET_STAGE")) c->subset_host = strcmp(e, "host") == 0;   // A/B + tests: node-subset staging in host loops
    if (const char* e = getenv("SIMON_ORDER_STAGE")) c->order_host = strcmp(e, "host") == 0;     // A/B + tests: composed order rows in host loops
    if (const char* e = getenv("SIMON_IMAGE_STAGE")) c->image_host = strcmp(e, "host") == 0;     // A/B + tests: image states of an own-nodes batch in a host loop
    if (const char* e = getenv("SIMON_IMAGE_STATE_MB")) c->img_state_cap = (size_t)std::max(atoll(e), 0ll) << 20;
    if (const char* e = getenv("SIMON_USAGE_TILE")) c->usage_tile = std::max(atoi(e), 0);        // tests: node tiles of simon_fetch_node_usage / _headroom
    c->debug_route = getenv("SIMON_DEBUG_ROUTE") != nullptr;
    c->force_table = getenv("SIMON_FORCE_TABLE") != nullptr;         // A/B + tests: keep 257 .. 384 signatures on the score-table kernel   // A/B: node classes not split into with / without devices
#ifdef SIMON_TABLE_PROFILE
    c->table_prof = getenv("SIMON_TABLE_PROF") != nullptr;   // phase profile of simon_table.hip: profiling builds only
#endif
    if (const char* e = getenv("SIMON_CACHE_LDS_PAD")) c->lds_pad = (size_t)atol(e);
    c->wide.knobs.no_lean = getenv("SIMON_WIDE_NO_LEAN") != nullptr;
    c->wide.knobs.no_table = getenv("SIMON_WIDE_NO_TABLE") != nullptr;
    c->wide.knobs.prof = getenv("SIMON_WIDE_PROF") != nullptr;
    c->wide.knobs.no_zmask = getenv("SIMON_WIDE_NO_ZMASK") != nullptr;
    c->wide.knobs.no_ident = getenv("SIMON_WIDE_NO_IDENT") != nullptr;
    c->wide.knobs.no_rows_lds = getenv("SIMON_WIDE_NO_ROWS_LDS") != nullptr;
    if (const char* e = getenv("SIMON_WIDE_NO_CACHE_B")) c->wide.knobs.no_cache_b = *e ? atoi(e) : 3;
    if (const char* e = getenv("SIMON_STATE_BUDGET_MB")) c->wide.knobs.state_budget = (size_t)atoll(e) << 20;
    return c;
}

void simon_ctx_destroy(simon_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    c->wide.release();
    // DevBuf destructors free device memory
    hipStream_t st = c->stream;
    delete c;
    if (st) (void)hipStreamDestroy(st);
}

const char* simon_last_error(simon_ctx* c) { return c ? c->err.c_str() : "null context"; }

int simon_load_nodes(simon_ctx* c, const simon_nodes_soa* nd) {
    if (!c || !nd) return SIMON_EINVAL;
    if (nd->struct_size != sizeof(simon_nodes_soa)) return fail(c, SIMON_EINVAL, "simon_nodes_soa size mismatch");
    const int N = nd->n_nodes;
    if (N <= 0 || !nd->alloc_cpu || !nd->alloc_mem || !nd->alloc_pods) return fail(c, SIMON_EINVAL, "nodes: missing required arrays");
    if (nd->n_scalar < 0 || nd->n_scalar > SIMON_MAX_SCALAR) return fail(c, SIMON_EINVAL, "n_scalar out of range");
    if (nd->n_scalar > 0 && !nd->scalar_alloc) return fail(c, SIMON_EINVAL, "scalar_alloc missing");
    if (nd->n_topo_keys < 0 || (nd->n_topo_keys > 0 && (!nd->topo_dom || !nd->topo_n_dom))) return fail(c, SIMON_EINVAL, "topology arrays missing");
    img_unrefine(c);                     // (a new pool: the image input no longer describes it)
    c->has_img = false; c->img_sizes.clear(); c->img_node_size.clear(); c->img_own_T = 0;
    c->N = N; c->K = nd->n_scalar; c->Kt = nd->n_topo_keys;
    copy_opt(c->alloc_cpu, nd->alloc_cpu, N); copy_opt(c->alloc_mem, nd->alloc_mem, N);
    copy_opt(c->alloc_eph, nd->alloc_eph, N); copy_opt(c->alloc_pods, nd->alloc_pods, N);
    copy_opt(c->i_req_cpu, nd->init_req_cpu, N); copy_opt(c->i_req_mem, nd->init_req_mem, N);
    copy_opt(c->i_req_eph, nd->init_req_eph, N); copy_opt(c->i_nz_cpu, nd->init_nz_cpu, N);
    copy_opt(c->i_nz_mem, nd->init_nz_mem, N); copy_opt(c->i_npods, nd->init_npods, N);
    copy_opt(c->node_class, nd->node_class, N);
    copy_opt(c->scalar_alloc, nd->scalar_alloc, (size_t)c->K * N);
    copy_opt(c->i_scalar_req, nd->init_scalar_req, (size_t)c->K * N);
    c->has_gpu_nodes = c->has_gpu = nd->gpu_cnt != nullptr;
    if (c->has_gpu && !nd->gpu_mem_total) return fail(c, SIMON_EINVAL, "gpu_mem_total missing");
    copy_opt(c->gpu_cnt, nd->gpu_cnt, N); copy_opt(c->gpu_mem_total, nd->gpu_mem_total, N);
    copy_opt(c->i_gpu_used, nd->init_gpu_used, (size_t)N * SIMON_MAX_GPU_DEV);
    for (int j = 0; j < N; ++j)
        if (c->gpu_cnt[j] < 0 || c->gpu_cnt[j] > SIMON_MAX_GPU_DEV) return fail(c, SIMON_ERANGE, "node %d: gpu_cnt %d > %d", j, c->gpu_cnt[j], SIMON_MAX_GPU_DEV);
    c->has_local = nd->local_flags != nullptr;
    if (c->has_local) {
        if (!nd->local_vg_cnt || !nd->local_vg_cap || !nd->local_vg_name || !nd->local_dev_cnt || !nd->local_dev_cap || !nd->local_dev_media)
            return fail(c, SIMON_EINVAL, "Open-Local node arrays missing");
        copy_opt(c->l_flags, nd->local_flags, N); copy_opt(c->l_vg_cnt, nd->local_vg_cnt, N);
        copy_opt(c->l_vg_cap, nd->local_vg_cap, (size_t)N * SIMON_MAX_VG); copy_opt(c->l_vg_req, nd->init_vg_req, (size_t)N * SIMON_MAX_VG);
        copy_opt(c->l_vg_name, nd->local_vg_name, (size_t)N * SIMON_MAX_VG); copy_opt(c->l_dev_cnt, nd->local_dev_cnt, N);
        copy_opt(c->l_dev_cap, nd->local_dev_cap, (size_t)N * SIMON_MAX_LDEV); copy_opt(c->l_dev_media, nd->local_dev_media, N);
        copy_opt(c->l_dev_alloc, nd->init_dev_alloc, N);
        for (int j = 0; j < N; ++j) {
            if (c->l_vg_cnt[j] < 0 || c->l_vg_cnt[j] > SIMON_MAX_VG || c->l_dev_cnt[j] < 0 || c->l_dev_cnt[j] > SIMON_MAX_LDEV)
                return fail(c, SIMON_ERANGE, "node %d: more than %d volume groups or %d devices", j, SIMON_MAX_VG, SIMON_MAX_LDEV);
            for (int v = 0; v < c->l_vg_cnt[j]; ++v)
                if (c->l_vg_cap[(size_t)j * SIMON_MAX_VG + v] <= 0) return fail(c, SIMON_EINVAL, "node %d: volume group %d without capacity", j, v);
            for (int d = 0; d < c->l_dev_cnt[j]; ++d)
                if (c->l_dev_cap[(size_t)j * SIMON_MAX_LDEV + d] <= 0) return fail(c, SIMON_EINVAL, "node %d: device %d without capacity", j, d);
        }
    }
    copy_opt(c->topo_dom, nd->topo_dom, (size_t)c->Kt * N); copy_opt(c->topo_n_dom, nd->topo_n_dom, (size_t)c->Kt);
    for (int k = 0; k < c->Kt; ++k)
        for (int j = 0; j < N; ++j) {
            const int d = c->topo_dom[(size_t)k * N + j];
            if (d < -1 || d >= c->topo_n_dom[k]) return fail(c, SIMON_EINVAL, "topo_dom[%d][%d] out of range", k, j);
        }
    c->have_nodes = true; c->staged = false; c->have_results = false;
    c->usage_nodes_staged = false; c->usage_gpu_nodes_staged = false; c->local_nodes_staged = false;
    return SIMON_OK;
}

int simon_load_pods(simon_ctx* c, const simon_pods_soa* pd) {
    if (!c || !pd) return SIMON_EINVAL;
    if (pd->struct_size != sizeof(simon_pods_soa)) return fail(c, SIMON_EINVAL, "simon_pods_soa size mismatch");
    if (!c->have_nodes) return fail(c, SIMON_ESTATE, "load nodes before pods");
    const int P = pd->n_pods;
    if (P < 0 || (P > 0 && (!pd->req_cpu || !pd->req_mem))) return fail(c, SIMON_EINVAL, "pods: missing required arrays");
    c->P = P;
    copy_opt(c->p_req_cpu, pd->req_cpu, P); copy_opt(c->p_req_mem, pd->req_mem, P); copy_opt(c->p_req_eph, pd->req_eph, P);
    if (pd->nz_cpu) copy_opt(c->p_nz_cpu, pd->nz_cpu, P); else c->p_nz_cpu = c->p_req_cpu;
    if (pd->nz_mem) copy_opt(c->p_nz_mem, pd->nz_mem, P); else c->p_nz_mem = c->p_req_mem;
    copy_opt(c->p_scalar, pd->scalar_req, (size_t)c->K * P);
    copy_opt(c->p_cls, pd->pod_class, P);
    copy_opt(c->p_preset, pd->preset_node, P, (int32_t)-1);
    copy_opt(c->p_gate, pd->gate_node, P, (int32_t)-1);
    copy_opt(c->p_gpu_mem, pd->gpu_mem, P); copy_opt(c->p_gpu_cnt, pd->gpu_cnt, P);
    copy_opt(c->p_pin, pd->pin_node, P, (int32_t)-1);
    copy_opt(c->p_gpu_index, pd->gpu_index, P);
    c->has_gpu_index = false;
    for (int p = 0; p < P; ++p) {
        const uint32_t w = c->p_gpu_index[p];
        if (!w) continue;
        c->has_gpu_index = true;
        bool ended = false;                            // nibbles: 1 + device id, 0 ends the list; ids 0 .. SIMON_MAX_GPU_DEV - 1
        for (int i = 0; i < 8; ++i) {
            const uint32_t nib = (w >> (4 * i)) & 15u;
            if (!nib) ended = true;
            else if (ended || nib > SIMON_MAX_GPU_DEV) return fail(c, SIMON_EINVAL, "pod %d: gpu_index 0x%x is not a packed device-id list", p, w);
        }
    }
    c->has_pin = false;
    for (int p = 0; p < P; ++p) {
        if (c->p_pin[p] >= c->N) return fail(c, SIMON_EINVAL, "pod %d: pin_node %d out of range", p, c->p_pin[p]);
        if (c->p_pin[p] >= 0 && c->p_preset[p] >= 0) return fail(c, SIMON_EINVAL, "pod %d: both preset_node and pin_node", p);
        c->has_pin = c->has_pin || c->p_pin[p] >= 0;
    }
    c->p_entries.clear(); c->p_priority.clear(); c->init_min_priority = 0x7fffffff;   // (ABI v6 additions: set after the pods)
    c->p_evict.clear(); c->evict_short = -1;
    c->pods_on = false;
    c->have_pods = true; c->staged = false; c->have_results = false;
    c->usage_pods_staged = false; c->usage_gpu_pods_staged = false; c->local_pods_staged = false;
    return SIMON_OK;
}

int simon_set_scalar_entries(simon_ctx* c, const uint8_t* entries) {
    if (!c) return SIMON_EINVAL;
    if (!c->have_pods) return fail(c, SIMON_ESTATE, "set_scalar_entries: load pods first");
    if (entries) {
        c->p_entries.assign(entries, entries + c->P);
        for (int p = 0; p < c->P; ++p) {
            if (c->p_entries[p] & 0x70u & ~((1u << SIMON_MAX_SCALAR) - 1u)) return fail(c, SIMON_EINVAL, "pod %d: scalar_entries 0x%x names a resource beyond SIMON_MAX_SCALAR", p, c->p_entries[p]);
            for (int k = 0; k < c->K; ++k)                    // a non-zero quantity IS an entry
                if (c->p_scalar[(size_t)k * c->P + p] != 0) c->p_entries[p] |= (uint8_t)(1u << k);
        }
    } else c->p_entries.clear();
    c->staged = false; c->wide_staged = false; c->have_results = false;
    return SIMON_OK;
}

static inline bool evicted_pod(const simon_ctx* c, int p) { return !c->p_evict.empty() && c->p_evict[p] != 0; }

int simon_set_pod_eviction(simon_ctx* c, const uint8_t* evict) {
    if (!c) return SIMON_EINVAL;
    if (!c->have_pods) return fail(c, SIMON_ESTATE, "set_pod_eviction: load pods first");
    if (c->seg_n > 0 || c->sub_on) return fail(c, SIMON_ESTATE, "set_pod_eviction: a %s batch is in effect; set the flags before simon_set_scenario_nodes", c->sub_on ? "node-subset" : "segmented");
    if (!evict) { c->p_evict.clear(); return SIMON_OK; }
    for (int p = 0; p < c->P; ++p) {
        if (!evict[p]) continue;
        if (c->p_preset[p] < 0) return fail(c, SIMON_EINVAL, "set_pod_eviction: pod %d is flagged but not preset to a node", p);
        if (c->p_gate[p] != -1) return fail(c, SIMON_EINVAL, "set_pod_eviction: pod %d is flagged and gated on node %d (a gated pod vanishes with its node)", p, c->p_gate[p]);
    }
    c->p_evict.assign(evict, evict + c->P);
    return SIMON_OK;
}

int simon_set_own_nodes_all_feature(simon_ctx* c, int32_t on) {
    if (!c) return SIMON_EINVAL;
    c->own_wide = on != 0;           // (read by the next simon_run_loaded / simon_explain_own_batch: nothing staged depends on it)
    return SIMON_OK;
}

int simon_set_pod_priorities(simon_ctx* c, const int32_t* priority, int32_t init_min_priority) {
    if (!c) return SIMON_EINVAL;
    if (!c->have_pods) return fail(c, SIMON_ESTATE, "set_pod_priorities: load pods first");
    if (priority) c->p_priority.assign(priority, priority + c->P); else c->p_priority.clear();
    c->init_min_priority = priority ? init_min_priority : 0x7fffffff;
    c->prio_staged = false; c->have_risk = false;
    return SIMON_OK;
}

int simon_set_image_locality(simon_ctx* c, const simon_image_locality* im) {
    if (!c) return SIMON_EINVAL;
    if (!c->have_nodes || !c->have_tables) return fail(c, SIMON_ESTATE, "set_image_locality: load nodes and class tables first");
    img_unrefine(c);
    c->staged = false; c->wide_staged = false; c->have_results = false;
    c->has_img = false; c->img_sizes.clear(); c->img_node_size.clear(); c->img_own_T = 0;
    c->img_size.clear(); c->img_node_off.clear(); c->img_node_image.clear(); c->img_node_count.clear(); c->img_class_off.clear(); c->img_class_image.clear();
    if (!im) return SIMON_OK;
    const int N = c->N, Cp = c->Cp, I = im->n_images;
    if (I < 0) return fail(c, SIMON_EINVAL, "image locality: n_images %d < 0", I);
    if (!im->node_off || !im->class_off || (I > 0 && !im->size)) return fail(c, SIMON_EINVAL, "image locality: size / node_off / class_off missing");
    if (im->node_off[0] != 0) return fail(c, SIMON_EINVAL, "image locality: node_off[0] != 0");
    for (int j = 0; j < N; ++j)
        if (im->node_off[j + 1] < im->node_off[j] || im->node_off[j + 1] - im->node_off[j] > I)
            return fail(c, SIMON_EINVAL, "image locality: node %d: node_off not ascending or more entries than images", j);
    if (im->class_off[0] != 0) return fail(c, SIMON_EINVAL, "image locality: class_off[0] != 0");
    for (int k = 0; k < Cp; ++k)
        if (im->class_off[k + 1] < im->class_off[k] || im->class_off[k + 1] - im->class_off[k] > (1 << 20))
            return fail(c, SIMON_EINVAL, "image locality: pod class %d: class_off not ascending or more than 2^20 containers", k);
    const size_t nnz = (size_t)im->node_off[N], ncont = (size_t)im->class_off[Cp];
    if ((nnz > 0 && (!im->node_image || !im->node_count)) || (ncont > 0 && !im->class_image))
        return fail(c, SIMON_EINVAL, "image locality: node_image / node_count / class_image missing");
    copy_opt(c->img_size, im->size, (size_t)I);
    copy_opt(c->img_node_off, im->node_off, (size_t)N + 1);
    copy_opt(c->img_node_image, im->node_image, nnz);
    copy_opt(c->img_node_count, im->node_count, nnz);
    copy_opt(c->img_class_off, im->class_off, (size_t)Cp + 1);
    copy_opt(c->img_class_image, im->class_image, ncont);
    for (int i = 0; i < I; ++i)
        if (c->img_size[i] < 0 || c->img_size[i] >= (1ll << 53)) return fail(c, SIMON_ERANGE, "image locality: image %d: size %lld outside [0, 2^53)", i, (long long)c->img_size[i]);
    std::vector<int32_t> seen(std::max(I, 1), -1);
    for (int j = 0; j < N; ++j)
        for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q) {
            const int32_t i = c->img_node_image[q];
            if (i < 0 || i >= I) return fail(c, SIMON_EINVAL, "image locality: node %d lists image id %d outside [0,%d)", j, i, I);
            if (seen[i] == j) return fail(c, SIMON_EINVAL, "image locality: node %d lists image %d twice", j, i);
            seen[i] = j;
            if (c->img_node_count[q] < 1 || c->img_node_count[q] > N)
                return fail(c, SIMON_ERANGE, "image locality: node %d: NumNodes %d of image %d outside [1,%d]", j, c->img_node_count[q], i, N);
        }
    for (size_t e = 0; e < ncont; ++e)
        if (c->img_class_image[e] < -1 || c->img_class_image[e] >= I) return fail(c, SIMON_EINVAL, "image locality: class_image[%zu] = %d outside [-1,%d)", e, c->img_class_image[e], I);
    c->has_img = true;
    return SIMON_OK;
}

int simon_set_image_node_sizes(simon_ctx* c, const int64_t* node_size) {
    if (!c) return SIMON_EINVAL;
    if (!c->has_img) return fail(c, SIMON_ESTATE, "set_image_node_sizes: load image locality first");
    if (c->img_own_T > 0) { c->img_own_T = 0; c->staged = false; c->wide_staged = false; c->have_results = false; }   // (an own-nodes image batch is loaded again)
    c->img_node_size.clear();
    if (!node_size) return SIMON_OK;
    const size_t nnz = c->img_node_image.size();
    for (size_t q = 0; q < nnz; ++q)
        if (node_size[q] < 0 || node_size[q] >= (1ll << 53)) return fail(c, SIMON_ERANGE, "set_image_node_sizes: entry %zu: size %lld outside [0, 2^53)", q, (long long)node_size[q]);
    c->img_node_size.assign(node_size, node_size + nnz);
    if (nnz == 0) c->img_node_size.assign(1, 0);                  // (attached, though no node lists anything: "empty" means detached)
    return SIMON_OK;
}

int simon_load_class_tables(simon_ctx* c, const simon_class_tables* tb) {
    if (!c || !tb) return SIMON_EINVAL;
    if (tb->struct_size != sizeof(simon_class_tables)) return fail(c, SIMON_EINVAL, "simon_class_tables size mismatch");
    if (!c->have_nodes) return fail(c, SIMON_ESTATE, "load nodes before class tables");
    if (tb->n_pod_classes <= 0 || tb->n_node_classes <= 0 || !tb->simon_raw) return fail(c, SIMON_EINVAL, "class tables: bad sizes");
    img_unrefine(c);                     // (new class tables: the image input no longer describes them)
    c->has_img = false; c->img_sizes.clear(); c->img_node_size.clear(); c->img_own_T = 0;
    c->Cp = tb->n_pod_classes; c->Cn = tb->n_node_classes;
    const size_t words = (size_t)(c->N + 63) / 64;
    c->has_mask = tb->static_mask != nullptr;
    copy_opt(c->static_mask, tb->static_mask, c->has_mask ? (size_t)c->Cp * words : 0);
    copy_opt(c->static_reason, tb->static_reason, tb->static_reason ? (size_t)c->Cp * c->N : 0);
    copy_opt(c->simon_raw, tb->simon_raw, (size_t)c->Cp * c->Cn);
    copy_opt(c->const_score, tb->const_score, (size_t)c->Cp);
    const size_t cells = (size_t)c->Cp * c->Cn;
    c->has_na = tb->node_affinity_raw != nullptr; c->has_tt = tb->taint_prefer_raw != nullptr; c->has_add = tb->static_add != nullptr;
    copy_opt(c->na_raw, tb->node_affinity_raw, c->has_na ? cells : 0);
    copy_opt(c->tt_raw, tb->taint_prefer_raw, c->has_tt ? cells : 0);
    copy_opt(c->static_add, tb->static_add, c->has_add ? cells : 0);
    for (int64_t x : c->na_raw) if (x < 0 || x >= (1ll << 40)) return fail(c, SIMON_ERANGE, "node_affinity_raw outside [0, 2^40)");
    for (int64_t x : c->tt_raw) if (x < 0 || x >= (1ll << 40)) return fail(c, SIMON_ERANGE, "taint_prefer_raw outside [0, 2^40)");
    for (int64_t x : c->static_add) if (x < 0 || x >= (1ll << 30)) return fail(c, SIMON_ERANGE, "static_add outside [0, 2^30)");
    c->l_spec_of.clear(); c->l_specs.clear();
    if (tb->local_spec_of) {
        if (!c->has_local) return fail(c, SIMON_ESTATE, "local_spec_of given but the nodes carry no Open-Local arrays");
        if (tb->n_local_specs < 0 || (tb->n_local_specs > 0 && !tb->local_specs)) return fail(c, SIMON_EINVAL, "local_specs missing");
        copy_opt(c->l_spec_of, tb->local_spec_of, (size_t)c->Cp);
        c->l_specs.assign(tb->local_specs, tb->local_specs + tb->n_local_specs);
        for (int32_t x : c->l_spec_of) if (x < -1 || x >= tb->n_local_specs) return fail(c, SIMON_EINVAL, "local_spec_of out of range");
        for (const simon_local_spec& sp : c->l_specs) {
            if (sp.n_lvm < 0 || sp.n_lvm > SIMON_MAX_LVOL || sp.n_ssd < 0 || sp.n_ssd > SIMON_MAX_LVOL || sp.n_hdd < 0 || sp.n_hdd > SIMON_MAX_LVOL)
                return fail(c, SIMON_ERANGE, "more than %d Open-Local volumes of one kind", SIMON_MAX_LVOL);
            for (int k = 0; k < sp.n_lvm; ++k) if (sp.lvm_size[k] <= 0) return fail(c, SIMON_EINVAL, "Open-Local volume size <= 0");
            for (int k = 0; k < sp.n_ssd; ++k) if (sp.ssd_size[k] <= 0 || (k && sp.ssd_size[k] < sp.ssd_size[k - 1])) return fail(c, SIMON_EINVAL, "ssd_size must be positive and ascending");
            for (int k = 0; k < sp.n_hdd; ++k) if (sp.hdd_size[k] <= 0 || (k && sp.hdd_size[k] < sp.hdd_size[k - 1])) return fail(c, SIMON_EINVAL, "hdd_size must be positive and ascending");
        }
    }
    c->Tm = tb->n_terms;
    if (c->Tm < 0) return fail(c, SIMON_EINVAL, "n_terms < 0");
    c->term_key.clear(); c->term_set.clear(); c->node_sets.clear(); c->R = 0;
    c->match_off.clear(); c->match_idx.clear(); c->anti_off.clear(); c->anti_idx.clear(); c->aff_off.clear(); c->aff_idx.clear(); c->port_off.clear(); c->port_idx.clear();
    c->class_flags.clear(); c->pref_off.clear(); c->pref_idx.clear(); c->pref_w.clear(); c->own_off.clear(); c->own_idx.clear();
    c->own_w.clear(); c->sh_off.clear(); c->sh_idx.clear(); c->sh_skew.clear(); c->sh_self.clear(); c->sh_set.clear();
    c->ss_off.clear(); c->ss_idx.clear(); c->ss_skew.clear(); c->topo_is_hostname.clear(); c->spread_log.clear();
    c->has_ipa_score = false;
    if (c->Tm > 0) {
        if (!tb->term_topo_key) return fail(c, SIMON_EINVAL, "term_topo_key missing");
        copy_opt(c->term_key, tb->term_topo_key, (size_t)c->Tm);
        for (int t = 0; t < c->Tm; ++t)
            if (c->term_key[t] < 0 || c->term_key[t] >= c->Kt) return fail(c, SIMON_EINVAL, "term %d: topology key out of range", t);
        c->R = tb->n_node_sets;
        if (c->R < 0 || (c->R > 0 && !tb->node_sets)) return fail(c, SIMON_EINVAL, "node_sets missing");
        copy_opt(c->node_sets, tb->node_sets, (size_t)c->R * words);
        copy_opt(c->term_set, tb->term_node_set, (size_t)c->Tm, (int32_t)-1);
        for (int32_t r : c->term_set) if (r < -1 || r >= c->R) return fail(c, SIMON_EINVAL, "term_node_set out of range");
        // one CSR list per role; idx entries are term ids
        struct Csr { const char* name; const int32_t* off; const int32_t* idx; std::vector<int32_t>* h_off; std::vector<int32_t>* h_idx; int cap; };
        Csr lists[] = {
            {"match", tb->match_off, tb->match_idx, &c->match_off, &c->match_idx, 1 << 20},
            {"anti", tb->anti_off, tb->anti_idx, &c->anti_off, &c->anti_idx, SIMON_MAX_TERMS_PER_CLASS * 4},
            {"aff", tb->aff_off, tb->aff_idx, &c->aff_off, &c->aff_idx, SIMON_MAX_TERMS_PER_CLASS * 4},
            {"port", tb->port_off, tb->port_idx, &c->port_off, &c->port_idx, 1 << 16},
            {"pref", tb->pref_off, tb->pref_idx, &c->pref_off, &c->pref_idx, SIMON_MAX_TERMS_PER_CLASS * 4},
            {"own", tb->own_off, tb->own_idx, &c->own_off, &c->own_idx, SIMON_MAX_TERMS_PER_CLASS * 8},
            {"spread_hard", tb->spread_hard_off, tb->spread_hard_idx, &c->sh_off, &c->sh_idx, SIMON_MAX_SPREAD},
            {"spread_soft", tb->spread_soft_off, tb->spread_soft_idx, &c->ss_off, &c->ss_idx, SIMON_MAX_SPREAD},
        };
        for (Csr& l : lists) {
            if (!l.off) continue;
            copy_opt(*l.h_off, l.off, (size_t)c->Cp + 1);
            if ((*l.h_off)[0] != 0) return fail(c, SIMON_EINVAL, "%s_off[0] != 0", l.name);
            for (int k = 0; k < c->Cp; ++k) {
                const int len = (*l.h_off)[k + 1] - (*l.h_off)[k];
                if (len < 0 || len > l.cap) return fail(c, SIMON_EINVAL, "class %d: %s list has %d entries (limit %d)", k, l.name, len, l.cap);
            }
            const size_t cnt = (size_t)(*l.h_off)[c->Cp];
            if (cnt > 0 && !l.idx) return fail(c, SIMON_EINVAL, "%s_idx missing", l.name);
            copy_opt(*l.h_idx, l.idx, cnt);
            for (int32_t t : *l.h_idx) if (t < 0 || t >= c->Tm) return fail(c, SIMON_EINVAL, "%s_idx out of range", l.name);
        }
        if (c->match_off.empty()) c->match_off.assign(c->Cp + 1, 0);
        if (c->anti_off.empty()) c->anti_off.assign(c->Cp + 1, 0);
        copy_opt(c->class_flags, tb->class_flags, tb->class_flags ? (size_t)c->Cp : 0);
        if (!c->pref_idx.empty()) { if (!tb->pref_w) return fail(c, SIMON_EINVAL, "pref_w missing"); copy_opt(c->pref_w, tb->pref_w, c->pref_idx.size()); }
        if (!c->own_idx.empty()) { if (!tb->own_w) return fail(c, SIMON_EINVAL, "own_w missing"); copy_opt(c->own_w, tb->own_w, c->own_idx.size()); }
        c->has_ipa_score = !c->pref_idx.empty() || !c->own_idx.empty();
        // counters are int32 on the device: bound the weighted sums by P * sum |w|
        long long wsum = 0;
        for (int32_t x : c->pref_w) wsum = std::max<long long>(wsum, std::llabs((long long)x));
        long long osum = 0;
        for (int k = 0; k < c->Cp && !c->own_off.empty(); ++k) {
            long long sk = 0;
            for (int e = c->own_off[k]; e < c->own_off[k + 1]; ++e) sk += std::llabs((long long)c->own_w[e]);
            osum = std::max(osum, sk);
        }
        if (osum * std::max(c->P, 1) >= (1ll << 31)) return fail(c, SIMON_ERANGE, "own_w x pods overflows the int32 weight counters");
        (void)wsum;
        if (!c->sh_idx.empty()) {
            if (!tb->spread_hard_skew || !tb->spread_hard_self) return fail(c, SIMON_EINVAL, "spread_hard_skew/self missing");
            copy_opt(c->sh_skew, tb->spread_hard_skew, c->sh_idx.size());
            copy_opt(c->sh_self, tb->spread_hard_self, c->sh_idx.size());
            copy_opt(c->sh_set, tb->spread_hard_set, c->sh_idx.size(), (int32_t)-1);
            for (int32_t r : c->sh_set) if (r < -1 || r >= c->R) return fail(c, SIMON_EINVAL, "spread_hard_set out of range");
        }
        if (!c->ss_idx.empty()) {
            if (!tb->spread_soft_skew || !tb->spread_log) return fail(c, SIMON_EINVAL, "spread_soft_skew / spread_log missing");
            copy_opt(c->ss_skew, tb->spread_soft_skew, c->ss_idx.size());
            copy_opt(c->spread_log, tb->spread_log, (size_t)c->N + 1);
            if ((long long)c->P * SIMON_MAX_SPREAD >= (1ll << 31) - 2) return fail(c, SIMON_ERANGE, "too many pods for the spread stamps");
        }
        copy_opt(c->topo_is_hostname, tb->topo_is_hostname, tb->topo_is_hostname ? (size_t)c->Kt : 0);
    } else {
        c->anti_off.assign(c->Cp + 1, 0); c->match_off.assign(c->Cp + 1, 0);
    }
    c->have_tables = true; c->staged = false; c->have_results = false;
    c->local_pods_staged = false;
    return SIMON_OK;
}

// does every scenario of the loaded batch bring its own node set (segmented or node-subset batch) instead of a prefix of the pool?
static inline bool own_nodes(const simon_ctx* c) { return c->seg_n > 0 || c->sub_on; }
static inline const char* own_kind(const simon_ctx* c) { return c->sub_on ? "node-subset" : "segmented"; }

// table_lds_bytes' nzk of the staged problem with `team` waves per scenario: -1 without SPREAD, else the zone-key count | kLds* bits
static int spread_lds_word(const simon_ctx* c, int team) {
    if (!c->spread) return -1;
    return (int)c->sp_zkeys.size() | ((c->ipa_fold || c->hard_fold) ? kLdsSecondTable : 0) | (team > 1 ? kLdsTeam : 0) | (c->Cn_t > kTableMaxClasses ? kLdsCn2 : 0);
}

// padded sizes, summary layout and workspace slices of the loaded batch for the score-table kernel (simon_load_scenarios; again
// after simon_set_scenario_segments, whose scenarios have their own class counts)
static int table_layout(simon_ctx* c) {
    const int S = (int)c->scen.size(), max_n = c->max_n;
    const std::vector<int32_t>& perm = c->h_perm;
    {
        // padded class-major size of every scenario; workspace slice of every workgroup (launch order = perm)
        const int Ct = c->Cn_t;
        std::vector<int> ni16(S), ni64(S);
        int top16 = 16, top64 = 64;
        for (int s = 0; s < S; ++s) {
            int a = 0, b = 0;
            for (int d = 0; d < Ct; ++d) {
                const int cnt = own_nodes(c) ? c->h_scls[(size_t)s * Ct + d] : c->h_clsprefix[(size_t)c->scen[s].n_nodes * Ct + d];   // (segmented / node-subset: the scenario's own count)
                a += (cnt + 15) & ~15; b += (cnt + 63) & ~63;
            }
            ni16[s] = std::max(a, 16); ni64[s] = std::max(b, 64);
            top16 = std::max(top16, ni16[s]); top64 = std::max(top64, ni64[s]);
        }
        {
            // One-level or two-level summary (simon_table.hip: tcarve)?  The LDS of a workgroup decides how many scenario waves a CU
            // holds (allocation granularity 1 280 B, 160 KB, at most 32 single-wave workgroups: profiles/micro/occupancy_probe.hip),
            // and a batch that offers more runs in rounds.  The two-level form needs a quarter of the LDS but costs an 8-byte load and
            // ~15 VALU per signature and cycle more (+19 % per wave, measured).  Cost model fitted to profiles/README.md (config 3:
            // 256 scenarios 7.7 ms, 4 096 14.0 ms, 8 192 27.5 ms one-level / 32.3 ms two-level; 100 signatures 39.5 / 32.1 ms):
            // a round of w waves per CU takes 1 + 0.055 (w - 1) units up to 16 waves and 0.11 per wave beyond.
            auto fit = [](size_t lds) { const size_t g = (lds + 1279) / 1280 * 1280; return g ? (int)std::min<size_t>(32, kTableLdsPerCU / g) : 32; };
            const size_t lds16 = table_lds_bytes(c->n_sigs, top16, Ct, false, false) + c->lds_pad, lds64 = table_lds_bytes(c->n_sigs, top64, Ct, true, c->rest, spread_lds_word(c, 1)) + c->lds_pad;   // (the single-wave shape: teams are a matter of the launch)
            const bool fine_ok = max_n <= kTableMaxNodes && top16 <= kTableMaxPadded && lds16 <= 64 * 1024, coarse_ok = top64 <= kTableMaxPaddedCoarse && lds64 <= kTableLdsMaxWG && Ct <= 128;   // (129 .. 256 classes: one-level only, simon_table_cls4.hip)
            const int per_cu = (S + c->n_cus - 1) / std::max(c->n_cus, 1);
            auto cost = [&](int fits, double factor) {
                auto round_cost = [](int w) { return 1.0 + 0.055 * (std::min(w, 16) - 1) + 0.11 * std::max(w - 16, 0); };
                double t = 0;
                for (int left = per_cu; left > 0; left -= fits) t += round_cost(std::min(left, fits));
                return t * factor;
            };
            bool coarse = coarse_ok && (!fine_ok || cost(std::max(fit(lds64), 1), 1.2) < 0.95 * cost(std::max(fit(lds16), 1), 1.0));
            if (c->force_coarse >= 0) coarse = c->force_coarse ? coarse_ok : !fine_ok && coarse_ok;
            if (c->rest) coarse = coarse_ok;                        // the REST path is built on the two-level layout
            if (c->n_sigs > 128) coarse = coarse_ok;                // ... and so are the signature groups beyond 128 (simon_table.hip: MANY)
            if (c->spread) coarse = coarse_ok;                      // ... and the SPREAD path (generation 7)
            if (c->fold || c->gfold) coarse = coarse_ok;            // ... and the folded exclusions / GPU share (carried by the two-level instantiations)
            c->table_coarse = coarse;
            for (int s = 0; s < S; ++s) c->scen_ni[s] = coarse ? ni64[s] : ni16[s];
            const int ni_top = coarse ? top64 : top16;
            c->table_ni_top = ni_top;
            std::vector<unsigned long long> ws_off(S);
            size_t off = 0;
            for (int b = 0; b < S; ++b) { ws_off[b] = off; off += table_ws_bytes(c->n_sigs, c->scen_ni[perm[b]], c->nzeq, coarse, Ct, c->rest ? c->rest_M : 0, c->rest ? (int)c->zone_keys.size() : 0, c->spread ? c->sp_TH : 0, c->spread ? c->sp_TZ : 0)
                                                                    + (c->gfold ? (((size_t)c->scen_ni[perm[b]] * 40 + 127) & ~(size_t)127) : 0); }   // + GPU fold: devices by position
            c->ws_total = off;
            HIP_TRY(c, c->d_ws_off.upload(ws_off, c->stream));
            // the shared initial image: the batch's largest scenario in the one-level layout (a prefix scenario's class lists are prefixes of its lists)
            c->pro_nb = 0; c->pro_bytes = 0;
            std::vector<int32_t> seg(Ct + 1, 0);                    // (alive until the synchronise below)
            if (!coarse && !own_nodes(c)) {
                for (int d = 0; d < Ct; ++d) seg[d + 1] = seg[d] + ((c->h_clsprefix[(size_t)max_n * Ct + d] + 15) & ~15);
                c->pro_nb = seg[Ct] / 16;
                c->pro_bytes = table_image_of(c->n_sigs, c->pro_nb, c->nzeq).total;
                HIP_TRY(c, c->d_pro_seg.upload(seg, c->stream));
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            // more than 128 signatures: two-level layout without the REST path (simon_table.hip: MANY; since round 4 also under generation 7's
            // walks); else generation 2 / all-feature kernel
            c->table_perm_ok = (!c->rest || coarse) && (c->n_sigs <= 128 || coarse) && (!c->spread || coarse) && (!c->fold || coarse) && (!c->gfold || coarse);
        }
    }
    return SIMON_OK;
}

// What a loaded batch derives from the staged problem next to its scenarios (simon_load_scenarios; again after an own-nodes image batch
// has re-staged the tables): for the score-table kernel the inverse orders -- placements are recorded by scheduling step and gathered
// back to pod ids through them, which takes every order to be a permutation of [0, P) -- and the layout of the batch.
// orders == null: the rows were composed on the device (simon_load_scenarios_composed) -- permutations by construction, their inverse
// already in d_inv_orders.
static int batch_orders_stage(simon_ctx* c, const int32_t* orders, int n_orders, int S, int max_n) {
    const int P = c->P;
    c->scen_ni.assign(S, 0);
    c->orders_perm = false;
    c->table_perm_ok = false;
    if (c->variant == SIMON_KERNEL_NARROW && c->table_ok) {
        std::vector<int32_t> inv(orders ? (size_t)n_orders * P : 0, -1);
        bool is_perm = true;
        for (int o = 0; orders && o < n_orders && is_perm; ++o)
            for (int i = 0; i < P; ++i) {
                int32_t& slot = inv[(size_t)o * P + orders[(size_t)o * P + i]];
                if (slot >= 0) { is_perm = false; break; }
                slot = i;
            }
        c->orders_perm = is_perm;
        c->S = S; c->max_n = max_n;
        if (is_perm) {
            if (orders) HIP_TRY(c, c->d_inv_orders.upload(inv, c->stream));
            if (const int rc = table_layout(c)) return rc;           // (synchronises: inv may die)
        }
    }
    return SIMON_OK;
}

// Order rows that the device composes from a validated segment table (simon_load_scenarios_composed): `dev` points at the uploaded table.
struct ComposedOrders {
    OrderCompose dev;
    bool live;                                           // the call installs pod rows: the live entries of every scenario's order
};

// The body of simon_load_scenarios and simon_load_scenarios_composed: the order rows are the caller's (orders) or composed on the device
// (comp, orders == null); everything else is the same call.
static int load_scenarios_body(simon_ctx* c, const simon_scenario* scen, int32_t S, const int32_t* orders, int32_t n_orders, const ComposedOrders* comp) {
    c->seg_n = 0; c->sub_on = false;                     // (segments and node subsets belong to the batch they were set for)
    c->pods_on = false; c->order_rows_on = false;        // (and so do pod rows)
    if (c->img_own_T > 0) { c->img_own_T = 0; c->staged = false; }   // (image states belong to the own-nodes batch they were built for)
    if (c->has_img) {                    // ImageLocality: one slot per distinct cluster size; another set of sizes re-stages the tables
        std::vector<int32_t> sizes(S);
        for (int s = 0; s < S; ++s) sizes[s] = scen[s].n_nodes;
        std::sort(sizes.begin(), sizes.end());
        sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
        if (sizes != c->img_sizes) { c->img_sizes = sizes; c->staged = false; }
    }
    int rc = stage(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int P = c->P;
    c->scen.resize(S);
    int max_n = 0;
    for (int s = 0; s < S; ++s) {
        if (scen[s].n_nodes < 0 || scen[s].n_nodes > c->N) return fail(c, SIMON_EINVAL, "scenario %d: n_nodes %d outside [0,%d]", s, scen[s].n_nodes, c->N);
        if (scen[s].order_id < 0 || scen[s].order_id >= n_orders) return fail(c, SIMON_EINVAL, "scenario %d: order_id out of range", s);
        c->scen[s] = ScenarioDesc{scen[s].n_nodes, scen[s].order_id};
        max_n = std::max(max_n, scen[s].n_nodes);
    }
    // every order must be a sequence of valid pod ids; preset targets must exist in each scenario
    for (size_t i = 0; orders && i < (size_t)n_orders * P; ++i)
        if (orders[i] < 0 || orders[i] >= P) return fail(c, SIMON_EINVAL, "orders[%zu] = %d is not a pod id", i, orders[i]);
    int min_n = c->N;
    for (int s = 0; s < S; ++s) min_n = std::min(min_n, scen[s].n_nodes);
    // (a pod flagged for eviction may lack its node in a node-subset batch, whose rows arrive after this call: evict_short holds the batch
    // back until they have -- simon_run_loaded)
    c->evict_short = -1;
    for (int p = 0; p < P; ++p)
        if (c->p_preset[p] >= 0 && c->p_preset[p] >= min_n && c->p_gate[p] < c->p_preset[p]) {
            if (evicted_pod(c, p)) { if (c->evict_short < 0) c->evict_short = p; continue; }
            return fail(c, SIMON_EINVAL, "pod %d is preset to node %d which a %d-node scenario lacks (gate it)", p, c->p_preset[p], min_n);
        }
    // LPT launch order: biggest scenarios first (cost ~ ceil(n / T) per pod)
    std::vector<int32_t> perm(S);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return scen[a].n_nodes > scen[b].n_nodes; });
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    HIP_TRY(c, c->d_scen.upload(c->scen, c->stream));
    HIP_TRY(c, c->d_perm.upload(perm, c->stream));
    HIP_TRY(c, c->d_orders.ensure((size_t)n_orders * P));
    const size_t W = (size_t)pod_row_words(P);
    if (orders) HIP_TRY(c, hipMemcpyAsync(c->d_orders.p, orders, (size_t)n_orders * P * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    else {
        // composed rows: the orders by stream position; by pod id the inverse orders, where batch_orders_stage would derive them, and the
        // presence words of every order
        const bool inv = c->variant == SIMON_KERNEL_NARROW && c->table_ok;
        if (inv) HIP_TRY(c, c->d_inv_orders.ensure((size_t)n_orders * P));
        if (comp->live) HIP_TRY(c, c->d_order_words.ensure((size_t)n_orders * W));
        HIP_TRY(c, launch_order_compose(comp->dev, c->d_orders.p, c->stream));
        HIP_TRY(c, launch_order_by_pod(comp->dev, inv ? c->d_inv_orders.p : nullptr, comp->live ? c->d_order_words.p : nullptr, c->stream));
    }
    HIP_TRY(c, c->d_unsched.ensure(S));
    HIP_TRY(c, c->d_used_cpu.ensure(S));
    HIP_TRY(c, c->d_used_mem.ensure(S));
    HIP_TRY(c, c->d_used_vg.ensure(S));
    HIP_TRY(c, c->d_plan.ensure(kPlanRecWords));
    if (c->img_R > 0) {
        std::vector<int32_t>& slot = c->h_img_slot;
        slot.resize(S);
        for (int s = 0; s < S; ++s) slot[s] = (int32_t)(std::lower_bound(c->img_sizes.begin(), c->img_sizes.end(), scen[s].n_nodes) - c->img_sizes.begin());
        HIP_TRY(c, c->d_img_slot.upload(slot, c->stream));
    }
    c->wide.img_slot_ext = c->img_R > 0 ? c->d_img_slot.p : nullptr;
    c->h_perm = perm;
    rc = batch_orders_stage(c, orders, n_orders, S, max_n);
    if (rc) return rc;
    if (!c->has_img) c->img_orders.clear();
    else if (orders) c->img_orders.assign(orders, orders + (size_t)n_orders * P);   // (an own-nodes batch re-stages, whenever the sizes arrive: img_own_restage)
    else {                                               // (composed rows are read back once for the host-side readers)
        c->img_orders.resize((size_t)n_orders * P);
        HIP_TRY(c, hipMemcpyAsync(c->img_orders.data(), c->d_orders.p, (size_t)n_orders * P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (!orders && c->has_local) {
        c->h_orders.resize((size_t)n_orders * P);
        HIP_TRY(c, hipMemcpyAsync(c->h_orders.data(), c->d_orders.p, (size_t)n_orders * P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (comp && comp->live) {                            // the pod rows: scenario s holds the live entries of its order
        static_assert(sizeof(ScenarioDesc) == 8, "order_rows_expand_kernel reads ScenarioDesc as int32 pairs");
        HIP_TRY(c, c->d_pod_words.ensure((size_t)S * W));
        HIP_TRY(c, launch_order_rows_expand(c->d_order_words.p, reinterpret_cast<const int32_t*>(c->d_scen.p), S, (int)W, c->d_pod_words.p, c->stream));
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // caller buffers may die after return
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.h2d_ms = ms;
    c->S = S; c->n_orders = n_orders; c->max_n = max_n;
    if (!c->has_local) c->h_orders.clear();
    else if (orders) c->h_orders.assign(orders, orders + (size_t)n_orders * P);     // (only the storage calls read them: local_stage)
    if (comp && comp->live) { c->pod_W = (int)W; c->pods_on = true; c->order_rows_on = true; }
    c->local_pods_staged = false;
    c->has_ranks = false;
    c->have_results = false;
    return SIMON_OK;
}

int simon_load_scenarios(simon_ctx* c, const simon_scenario* scen, int32_t S, const int32_t* orders, int32_t n_orders) {
    if (!c || !scen || S <= 0 || !orders || n_orders <= 0) return c ? fail(c, SIMON_EINVAL, "load_scenarios: bad arguments") : SIMON_EINVAL;
    return load_scenarios_body(c, scen, S, orders, n_orders, nullptr);
}

// simon_load_scenarios with the order rows composed from segments: on the device (simon_orders.hip) from the uploaded table, or with
// SIMON_ORDER_STAGE=host in the loops of order_segments_compose_host, whose rows then take simon_load_scenarios' and
// simon_set_scenario_pods' own road.
static int load_composed(simon_ctx* c, const simon_scenario* scen, int32_t S, const simon_order_segments* seg, int32_t n_orders) {
    if (!scen || S <= 0 || !seg || n_orders <= 0) return fail(c, SIMON_EINVAL, "load_scenarios_composed: bad arguments");
    if (seg->struct_size != sizeof(simon_order_segments)) return fail(c, SIMON_EINVAL, "load_scenarios_composed: simon_order_segments size mismatch");
    if (!(c->have_nodes && c->have_pods && c->have_tables)) return fail(c, SIMON_ESTATE, "load nodes, pods and class tables before scenarios");
    const int P = c->P;
    OrderSegTable t;
    long long at = 0;
    const OrderSegView view{seg->n_seg, seg->seg_start, seg->n_variants, seg->variant_pods, seg->variant_live, seg->choice};
    if (const OrderSegError e = order_segments_check(view, P, n_orders, t, &at))
        return fail(c, SIMON_EINVAL, "load_scenarios_composed: %s (entry %lld)", order_segments_text(e), at);
    if (c->debug_route) fprintf(stderr, "[orders] stage %s n_orders %d segments %d table ids %zu\n", c->order_host ? "host" : "device", n_orders, t.G, t.n_ids());
    const size_t W = (size_t)pod_row_words(P);
    if (c->order_host) {
        std::vector<int32_t> orders((size_t)n_orders * P);
        std::vector<uint32_t> words(seg->variant_live ? (size_t)n_orders * W : 0);
        order_segments_compose_host(t, seg->variant_pods, seg->variant_live, seg->choice, n_orders, orders.data(), nullptr,
                                    seg->variant_live ? words.data() : nullptr);
        if (const int rc = load_scenarios_body(c, scen, S, orders.data(), n_orders, nullptr)) return rc;
        if (!seg->variant_live) return SIMON_OK;
        std::vector<uint32_t> rows((size_t)S * W);
        for (int s = 0; s < S; ++s) std::copy_n(words.begin() + (size_t)scen[s].order_id * W, W, rows.begin() + (size_t)s * W);
        if (const int rc = simon_set_scenario_pods(c, rows.data())) return rc;
        HIP_TRY(c, c->d_order_words.upload(words, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->order_rows_on = true;
        return SIMON_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the table on the device, for the length of this call: sum_g n_variants[g] x len_g ids twice, n_orders x G choices
    DevBuf<int32_t> d_start, d_live_off, d_pods, d_pos, d_owner, d_local, d_live, d_choice;
    DevBuf<int64_t> d_var_off;
    const std::vector<int32_t> pods(seg->variant_pods, seg->variant_pods + t.n_ids()), choice(seg->choice, seg->choice + (size_t)n_orders * t.G);
    std::vector<int32_t> live;
    if (seg->variant_live) live.assign(seg->variant_live, seg->variant_live + t.n_var());
    const auto staged = [&]() -> int {
        HIP_TRY(c, d_start.upload(t.seg_start, c->stream));
        HIP_TRY(c, d_var_off.upload(t.var_off, c->stream));
        HIP_TRY(c, d_live_off.upload(t.live_off, c->stream));
        HIP_TRY(c, d_pods.upload(pods, c->stream));
        HIP_TRY(c, d_pos.upload(t.pos, c->stream));
        HIP_TRY(c, d_owner.upload(t.owner, c->stream));
        HIP_TRY(c, d_local.upload(t.local, c->stream));
        HIP_TRY(c, d_choice.upload(choice, c->stream));
        if (seg->variant_live) HIP_TRY(c, d_live.upload(live, c->stream));
        ComposedOrders comp;
        comp.dev = OrderCompose{d_start.p, d_var_off.p, d_live_off.p, d_pods.p, d_pos.p, d_owner.p, d_local.p, seg->variant_live ? d_live.p : nullptr,
                                d_choice.p, t.G, P, n_orders};
        comp.live = seg->variant_live != nullptr;
        return load_scenarios_body(c, scen, S, nullptr, n_orders, &comp);
    };
    const int rc = staged();
    (void)hipStreamSynchronize(c->stream);                       // (the table's buffers die here: whichever step failed, nothing of it is in flight)
    return rc;
}

int simon_load_scenarios_composed(simon_ctx* c, const simon_scenario* scen, int32_t S, const simon_order_segments* seg, int32_t n_orders) {
    if (!c) return SIMON_EINVAL;
    int rc;
    try {
        rc = load_composed(c, scen, S, seg, n_orders);
    } catch (const std::exception&) {                    // (no exception crosses the C ABI: a table the host cannot hold)
        rc = fail(c, SIMON_ENOMEM, "load_scenarios_composed: out of host memory");
    }
    if (rc) { c->S = 0; c->pods_on = false; c->order_rows_on = false; }     // (a failing call leaves no batch loaded)
    return rc;
}

int simon_fetch_orders(simon_ctx* c, int32_t first, int32_t n, int32_t* orders, uint32_t* present) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "fetch_orders: load scenarios first");
    if (!orders || first < 0 || n < 1 || first > c->n_orders - n) return fail(c, SIMON_EINVAL, "fetch_orders: rows [%d, %d + %d) outside the %d loaded orders", first, first, n, c->n_orders);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t P = c->P, W = (size_t)pod_row_words(c->P);
    HIP_TRY(c, hipMemcpyAsync(orders, c->d_orders.p + (size_t)first * P, (size_t)n * P * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (present && c->order_rows_on)
        HIP_TRY(c, hipMemcpyAsync(present, c->d_order_words.p + (size_t)first * W, (size_t)n * W * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    else if (present)                                            // (no rows of a composed batch: every order holds every pod)
        for (size_t i = 0; i < (size_t)n * W; ++i) present[i] = (i % W == W - 1 && (P & 31)) ? ~(~0u << (P & 31)) : ~0u;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

// is pool node j part of loaded scenario s?  Node-subset batches: its presence bit; prefix batches: j < n_nodes; segmented ones: a
// fixed node or within its segment's count
static inline bool node_in(const simon_ctx* c, size_t s, int j) {
    if (c->sub_on) return (c->sub_words[s * (size_t)c->sub_W + (j >> 5)] >> (j & 31)) & 1u;
    if (!c->seg_n) return j < c->scen[s].n_nodes;
    const int g = c->seg_of[j];
    return g < 0 || j - c->seg_start[g] < c->seg_count[s * c->seg_n + g];
}

// rank rows of the loaded batch: the caller's (validated over each scenario's own nodes) or, rank == NULL on a segmented batch, pool
// order restricted to the scenario (own: the batch's scenarios bring their own node sets, own_nodes()).  Nodes outside a scenario get
// rank N (the score-table kernel tests presence by it).
static int load_ranks(simon_ctx* c, const int32_t* rank) {
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t S = c->S, N = c->N;
    const bool own = own_nodes(c);
    std::vector<int32_t> inv(S * N, 0);
    std::vector<int32_t> rk = own ? std::vector<int32_t>(S * N, (int32_t)N) : std::vector<int32_t>(rank, rank + S * N);
    std::vector<char> seen;
    for (size_t s = 0; s < S; ++s) {
        const int n = c->scen[s].n_nodes;
        seen.assign(n, 0);
        int next = 0;
        const int hi = own ? (int)N : n;
        for (int j = 0; j < hi; ++j) {
            if (own && !node_in(c, s, j)) continue;
            const int r = rank ? rank[s * N + j] : next++;
            if (r < 0 || r >= n || seen[r]) return fail(c, SIMON_EINVAL, "set_node_ranks: scenario %d: not a permutation of 0..%d over its nodes", (int)s, n - 1);
            seen[r] = 1;
            inv[s * N + r] = j;
            if (own) rk[s * N + j] = r;
        }
    }
    HIP_TRY(c, c->d_node_rank.upload(rk, c->stream));
    HIP_TRY(c, c->d_node_inv.upload(inv, c->stream));
    // the score-table kernel's view of a scenario's own node order: per-class node lists in rank order (class segments at the
    // pool's class offsets; a scenario fills the first clsprefix[n][d] entries of segment d -- segmented: h_scls[s][d]) and a node's
    // index inside its class
    c->table_ranks_ok = false;
    if (c->variant == SIMON_KERNEL_NARROW && c->table_ok && c->table_perm_ok) {
        const int Ct = c->Cn_t;
        std::vector<int32_t> ids(S * N, 0), pos(S * N, 0), fill(Ct);
        for (size_t s = 0; s < S; ++s) {
            const int n = c->scen[s].n_nodes;
            std::fill(fill.begin(), fill.end(), 0);
            for (int r = 0; r < n; ++r) {                       // nodes in rank order
                const int j = inv[s * N + r], d = c->h_ncls_t[j];
                pos[s * N + j] = fill[d];
                ids[s * N + c->h_cls_off[d] + fill[d]++] = j;
            }
        }
        HIP_TRY(c, c->d_rk_ids.upload(ids, c->stream));
        HIP_TRY(c, c->d_rk_pos.upload(pos, c->stream));
        c->table_ranks_ok = true;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->has_ranks = true;
    c->have_results = false;
    return SIMON_OK;
}

static int subset_stage(simon_ctx* c);

int simon_set_node_ranks(simon_ctx* c, const int32_t* rank) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "set_node_ranks: load scenarios first");
    if (!rank) {
        if (c->sub_on) return subset_stage(c);                // a node-subset batch keeps its own rows: nodeTree order of its nodes
        if (c->seg_n) return load_ranks(c, nullptr);          // a segmented batch keeps its own rows: pool order over its nodes
        c->has_ranks = false; return SIMON_OK;
    }
    return load_ranks(c, rank);
}

// the slot of every loaded scenario on the device
static int img_slots_upload(simon_ctx* c) {
    HIP_TRY(c, c->d_img_slot.upload(c->h_img_slot, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->wide.img_slot_ext = c->img_R > 0 ? c->d_img_slot.p : nullptr;
    return SIMON_OK;
}

// the tables staged again for another set of slots, the loaded scenarios, orders and pod rows kept
static int img_own_restage(simon_ctx* c) {
    c->seg_n = 0; c->sub_on = false;                              // (the layout of a prefix batch first: the class counts of an own-nodes one are the caller's next step)
    c->has_ranks = false; c->table_ranks_ok = false; c->have_results = false;
    c->staged = false;
    if (const int rc = stage(c)) return rc;
    return batch_orders_stage(c, c->img_orders.data(), c->n_orders, c->S, c->max_n);
}

// An own-nodes batch leaves its image states: the per-size slots of the prefix batch again.
static int img_own_leave(simon_ctx* c) {
    if (c->img_own_T == 0) return SIMON_OK;
    c->img_own_T = 0; c->img_own_n.clear(); c->img_own_words.clear();
    if (const int rc = img_own_restage(c)) return rc;
    if (c->img_R == 0) return SIMON_OK;
    c->h_img_slot.resize(c->S);
    for (int s = 0; s < c->S; ++s) c->h_img_slot[s] = (int32_t)(std::lower_bound(c->img_sizes.begin(), c->img_sizes.end(), c->scen[s].n_nodes) - c->img_sizes.begin());
    return img_slots_upload(c);
}

// An image problem enters an own-nodes batch (simon_set_scenario_segments / simon_set_scenario_nodes after their validation; words [S][W]
// = the presence rows).  The caller's NumNodes / Size must be the pool-order reading of the whole pool, which is what the slots'
// own readings restrict.  A slot is (node count, presence of the listing nodes): scenarios that agree on both score alike.
static int img_own_enter(simon_ctx* c, const char* who, const std::vector<uint32_t>& words) {
    const int S = c->S, N = c->N, W = (N + 31) / 32, I = (int)c->img_size.size();
    if (c->img_orders.size() != (size_t)c->n_orders * c->P)      // (cannot happen through the public calls: every road to a staged image batch keeps them)
        return fail(c, SIMON_ESTATE, "%s: the loaded orders of the image batch are gone; load the scenarios again", who);
    std::vector<int32_t> run(I, 0);
    std::vector<uint32_t> lists(W, 0);
    for (int j = 0; j < N; ++j)
        for (int q = c->img_node_off[j]; q < c->img_node_off[j + 1]; ++q) {
            const int im = c->img_node_image[q];
            lists[j >> 5] |= 1u << (j & 31);
            if (c->img_node_count[q] != ++run[im] || (run[im] == 1 && c->img_size[im] != c->img_node_size[q]))
                return fail(c, SIMON_EINVAL, "%s: image %d at node %d: arrival order is not pool order (NumNodes %d, the pool-order reading is %d; Size is the first lister's)", who, im, j, c->img_node_count[q], run[im]);
        }
    std::map<std::vector<uint32_t>, int> ids;
    std::vector<int32_t> slot(S), own_n;
    std::vector<uint32_t> own_words, key(W + 1);
    for (int s = 0; s < S; ++s) {
        key[0] = (uint32_t)c->scen[s].n_nodes;
        for (int w = 0; w < W; ++w) key[w + 1] = words[(size_t)s * W + w] & lists[w];
        const auto it = ids.emplace(key, (int)ids.size());
        if (it.second) {
            own_n.push_back(c->scen[s].n_nodes);
            own_words.insert(own_words.end(), words.begin() + (size_t)s * W, words.begin() + (size_t)(s + 1) * W);
        }
        slot[s] = it.first->second;
    }
    int img_R = 0, listing = 0;
    for (int cp = 0; cp < c->Cp; ++cp)
        for (int e = c->img_class_off[cp]; e < c->img_class_off[cp + 1]; ++e)
            if (c->img_class_image[e] >= 0) { ++img_R; break; }
    for (int j = 0; j < N; ++j) listing += c->img_node_off[j + 1] > c->img_node_off[j];
    const size_t Cn1 = (size_t)(c->img_refined ? c->img_base_Cn : c->Cn) + (img_R ? listing : 0);
    // (the cap also counts the kernel's global count rows, one per slot, where the counts do not fit its LDS)
    const size_t per_slot = (c->img_node_image.size() + (size_t)I) * sizeof(int32_t);
    const size_t scratch = (!c->image_host && per_slot > kImageLdsBudget) ? ids.size() * per_slot : 0;
    if (ids.size() * (size_t)img_R * Cn1 + scratch > c->img_state_cap)
        return fail(c, SIMON_ESTATE, "%s: %zu image states x %d image-scoring pod classes x %zu node classes (+ %zu bytes of count rows) exceed the cap of %zu MB (SIMON_IMAGE_STATE_MB)", who, ids.size(), img_R, Cn1, scratch, c->img_state_cap >> 20);
    c->img_own_T = (int32_t)ids.size(); c->img_own_n = own_n; c->img_own_words = own_words;
    if (const int rc = img_own_restage(c)) return rc;
    if (c->img_R == 0) return SIMON_OK;
    c->h_img_slot = slot;
    return img_slots_upload(c);
}

// a failed simon_set_scenario_segments / simon_set_scenario_nodes leaves the batch as a prefix batch: its own layout again, no ranks
static int seg_abandon(simon_ctx* c, int rc) {
    c->seg_n = 0; c->sub_on = false;
    if (c->img_own_T > 0) {                                       // (the per-size slots restored; the refusal keeps its own code and text)
        const std::string why = c->err;
        (void)img_own_leave(c);
        c->err = why;
    }
    c->has_ranks = false; c->table_ranks_ok = false; c->have_results = false;
    if (c->variant == SIMON_KERNEL_NARROW && c->table_ok && c->orders_perm) (void)table_layout(c);
    return rc;
}

// does pool node j carry pods bound before the stream (init_* state)?  Such a node has to be part of every scenario.
static bool node_busy(const simon_ctx* c, int j) {
    const int N = c->N;
    auto nz = [](const auto& v, size_t i) { return i < v.size() && v[i] != 0; };
    bool busy = nz(c->i_npods, j) || nz(c->i_req_cpu, j) || nz(c->i_req_mem, j) || nz(c->i_req_eph, j) || nz(c->i_nz_cpu, j) || nz(c->i_nz_mem, j) || nz(c->l_dev_alloc, j);
    for (int k = 0; k < SIMON_MAX_GPU_DEV; ++k) busy = busy || nz(c->i_gpu_used, (size_t)j * SIMON_MAX_GPU_DEV + k);
    for (int k = 0; k < SIMON_MAX_VG; ++k) busy = busy || nz(c->l_vg_req, (size_t)j * SIMON_MAX_VG + k);
    for (size_t k = 0; k < c->i_scalar_req.size() / std::max(N, 1); ++k) busy = busy || nz(c->i_scalar_req, k * N + j);
    return busy;
}

int simon_set_scenario_segments(simon_ctx* c, int32_t n_seg, const int32_t* seg_start, const int32_t* count) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "set_scenario_segments: load scenarios first");
    if (c->has_img && c->img_node_size.empty()) return fail(c, SIMON_ESTATE, "set_scenario_segments: ImageLocality is in effect (its image counts depend on the node set)");
    const int S = c->S, N = c->N;
    // (with an own-nodes image batch loaded a refusal also gives the per-size slots back: "a call that fails leaves a prefix batch")
    auto bad = [&](int rc) { return c->img_own_T > 0 ? seg_abandon(c, rc) : rc; };
    if (n_seg < 0 || n_seg > SIMON_MAX_SEGMENTS) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: n_seg %d outside [0,%d]", n_seg, SIMON_MAX_SEGMENTS));
    if (n_seg > 0 && (!seg_start || !count)) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: %d segments without starts / counts", n_seg));
    if (n_seg == 0) {                                        // back to prefix scenarios
        if (!own_nodes(c)) return SIMON_OK;
        c->seg_n = 0; c->sub_on = false;
        c->has_ranks = false; c->table_ranks_ok = false; c->have_results = false;
        if (c->img_own_T > 0) return img_own_leave(c);           // (re-stages for the per-size slots, the layout included)
        return (c->variant == SIMON_KERNEL_NARROW && c->table_ok && c->orders_perm) ? table_layout(c) : SIMON_OK;
    }
    for (int g = 0; g < n_seg; ++g) {
        const int end = g + 1 < n_seg ? seg_start[g + 1] : N;
        if (seg_start[g] < 0 || seg_start[g] > end || end > N) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: segment %d [%d,%d) is not ascending inside [0,%d]", g, seg_start[g], end, N));
    }
    const int fixed = seg_start[0];
    for (int s = 0; s < S; ++s) {
        long long tot = fixed;
        for (int g = 0; g < n_seg; ++g) {
            const int cnt = count[(size_t)s * n_seg + g], len = (g + 1 < n_seg ? seg_start[g + 1] : N) - seg_start[g];
            if (cnt < 0 || cnt > len) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: scenario %d: count %d of segment %d outside [0,%d]", s, cnt, g, len));
            tot += cnt;
        }
        if (tot != c->scen[s].n_nodes) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: scenario %d: n_nodes %d, but its fixed nodes and counts make %lld", s, c->scen[s].n_nodes, tot));
        if (tot == 0) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: scenario %d holds no node at all (no fixed nodes, every count 0)", s));   // (the ranked instantiations have never run an empty scenario)
    }
    // a segment node starts empty: pods bound before the stream or by Spec.NodeName would need it in every scenario
    for (int j = fixed; j < N; ++j) {
        if (node_busy(c, j)) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: segment node %d carries pods bound before the stream", j));
    }
    for (int p = 0; p < c->P; ++p)
        if (c->p_preset[p] >= fixed) return bad(fail(c, SIMON_EINVAL, "set_scenario_segments: pod %d is preset to segment node %d", p, c->p_preset[p]));
    if (c->has_img) {                                          // image states of the scenarios' own node sets (presence words from the counts)
        const int W = (N + 31) / 32;
        std::vector<uint32_t> words((size_t)S * W, 0);
        for (int s = 0; s < S; ++s) {
            uint32_t* row = words.data() + (size_t)s * W;
            for (int j = 0; j < fixed; ++j) row[j >> 5] |= 1u << (j & 31);
            for (int g = 0; g < n_seg; ++g)
                for (int j = seg_start[g]; j < seg_start[g] + count[(size_t)s * n_seg + g]; ++j) row[j >> 5] |= 1u << (j & 31);
        }
        if (const int rc = img_own_enter(c, "set_scenario_segments", words)) return seg_abandon(c, rc);
    }
    c->seg_n = n_seg; c->sub_on = false;                       // (segments replace a node-subset batch)
    c->seg_start.assign(seg_start, seg_start + n_seg);
    c->seg_count.assign(count, count + (size_t)S * n_seg);
    c->seg_of.assign(N, -1);
    for (int g = 0; g < n_seg; ++g)
        for (int j = seg_start[g]; j < (g + 1 < n_seg ? seg_start[g + 1] : N); ++j) c->seg_of[j] = g;
    // satisfyResourceSetting's denominators over each scenario's own nodes: prefix differences per segment
    const std::vector<int64_t>* pf[3] = {&c->prefix_cpu, &c->prefix_mem, &c->prefix_vg};
    c->seg_tot.assign((size_t)3 * S, 0);
    for (int q = 0; q < 3; ++q) {
        const std::vector<int64_t>& v = *pf[q];
        if (v.size() < (size_t)N + 1) continue;
        for (int s = 0; s < S; ++s) {
            int64_t t = v[fixed];
            for (int g = 0; g < n_seg; ++g) t += v[seg_start[g] + c->seg_count[(size_t)s * n_seg + g]] - v[seg_start[g]];
            c->seg_tot[(size_t)q * S + s] = t;
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_seg_tot.upload(c->seg_tot, c->stream));
    if (c->variant == SIMON_KERNEL_NARROW && c->table_ok) {    // per-class counts of every scenario: the score-table kernel's prologue and layout
        const int Ct = c->Cn_t;
        c->h_scls.assign((size_t)S * Ct, 0);
        for (int s = 0; s < S; ++s)
            for (int j = 0; j < N; ++j)
                if (node_in(c, s, j)) ++c->h_scls[(size_t)s * Ct + c->h_ncls_t[j]];
        HIP_TRY(c, c->d_scls.upload(c->h_scls, c->stream));
        if (c->orders_perm) {
            const int rc = table_layout(c);
            if (rc) return seg_abandon(c, rc);
        }
    }
    const int rc = load_ranks(c, nullptr);
    return rc ? seg_abandon(c, rc) : SIMON_OK;
}

// The per-scenario arrays of a node-subset batch (c->sub_words, c->sub_zone): rank rows in each scenario's nodeTree order and their
// inverse, per-class node lists, class counts (h_scls) and allocatable / VG totals (seg_tot), then the score-table layout of the batch.
// On the device (simon_subset.hip; only the counts and totals come back), or with SIMON_SUBSET_STAGE=host in the loops a segmented
// batch uses.
static int subset_stage(simon_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t S = c->S, N = c->N;
    const int Ct = c->Cn_t;
    const bool cls = c->variant == SIMON_KERNEL_NARROW && c->table_ok;
    c->has_ranks = false; c->table_ranks_ok = false; c->have_results = false;
    c->seg_tot.assign(3 * S, 0);
    if (cls) c->h_scls.assign(S * Ct, 0);
    if (c->subset_host) {
        // nodeTree.list() of every scenario: its nodes by zone in pool order, zones in first-appearance order, one node per zone per round
        std::vector<int32_t> rows(S * N, (int32_t)N);
        std::vector<std::vector<int>> tree;
        std::vector<int> slot;
        for (size_t s = 0; s < S; ++s) {
            tree.clear();
            slot.assign(SIMON_MAX_ZONES, -1);
            for (int j = 0; j < (int)N; ++j) {
                if (!node_in(c, s, j)) continue;
                const int z = c->sub_zone.empty() ? 0 : c->sub_zone[j];
                if (slot[z] < 0) { slot[z] = (int)tree.size(); tree.emplace_back(); }
                tree[slot[z]].push_back(j);
                c->seg_tot[s] += c->alloc_cpu[j];
                c->seg_tot[S + s] += c->alloc_mem[j];
                c->seg_tot[2 * S + s] += c->prefix_vg[j + 1] - c->prefix_vg[j];
                if (cls) ++c->h_scls[s * Ct + c->h_ncls_t[j]];
            }
            int r = 0;
            for (size_t round = 0; r < c->scen[s].n_nodes; ++round)
                for (const std::vector<int>& zone : tree)
                    if (round < zone.size()) rows[s * N + zone[round]] = r++;
        }
        HIP_TRY(c, c->d_seg_tot.upload(c->seg_tot, c->stream));
        if (cls) {
            HIP_TRY(c, c->d_scls.upload(c->h_scls, c->stream));
            if (c->orders_perm)
                if (const int rc = table_layout(c)) return rc;
        }
        return load_ranks(c, rows.data());
    }
    HIP_TRY(c, c->d_node_rank.ensure(S * N));
    HIP_TRY(c, c->d_node_inv.ensure(S * N));
    HIP_TRY(c, c->d_seg_tot.ensure(3 * S));
    HIP_TRY(c, hipMemsetAsync(c->d_node_inv.p, 0, S * N * sizeof(int32_t), c->stream));
    if (cls) {
        HIP_TRY(c, c->d_rk_ids.ensure(S * N));
        HIP_TRY(c, c->d_rk_pos.ensure(S * N));
        HIP_TRY(c, c->d_scls.ensure(S * Ct));
        HIP_TRY(c, hipMemsetAsync(c->d_rk_ids.p, 0, S * N * sizeof(int32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_rk_pos.p, 0, S * N * sizeof(int32_t), c->stream));
    }
    SubsetStage a{};
    a.present = c->d_sub_words.p; a.node_zone = c->sub_zone.empty() ? nullptr : c->d_sub_zone.p;
    a.ncls = cls ? c->d_t_ncls.p : nullptr; a.cls_off = c->d_cls_off.p;
    a.prefix_cpu = c->d_prefix_cpu.p; a.prefix_mem = c->d_prefix_mem.p; a.prefix_vg = c->d_prefix_vg.p;
    a.S = (int32_t)S; a.N = (int32_t)N; a.W = c->sub_W; a.Ct = Ct;
    a.rank = c->d_node_rank.p; a.inv = c->d_node_inv.p; a.rk_ids = c->d_rk_ids.p; a.rk_pos = c->d_rk_pos.p; a.scls = c->d_scls.p; a.tot = c->d_seg_tot.p;
    HIP_TRY(c, launch_subset_stage(a, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->seg_tot.data(), c->d_seg_tot.p, 3 * S * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (cls) HIP_TRY(c, hipMemcpyAsync(c->h_scls.data(), c->d_scls.p, S * Ct * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (cls && c->orders_perm)
        if (const int rc = table_layout(c)) return rc;
    c->table_ranks_ok = cls && c->table_perm_ok;
    c->has_ranks = true;
    return SIMON_OK;
}

int simon_set_scenario_nodes(simon_ctx* c, const uint32_t* present, const int32_t* node_zone, int32_t n_zones) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "set_scenario_nodes: load scenarios first");
    if (!present) return simon_set_scenario_segments(c, 0, nullptr, nullptr);        // back to prefix scenarios
    if (c->has_img && c->img_node_size.empty()) return fail(c, SIMON_ESTATE, "set_scenario_nodes: ImageLocality is in effect (its image counts depend on the node set)");
    const int S = c->S, N = c->N, W = (N + 31) / 32;
    // every refusal leaves a prefix batch, whatever the batch was before
    if (node_zone) {
        if (n_zones < 1 || n_zones > SIMON_MAX_ZONES) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: n_zones %d outside [1,%d]", n_zones, SIMON_MAX_ZONES));
        for (int j = 0; j < N; ++j)
            if (node_zone[j] < 0 || node_zone[j] >= n_zones) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: node %d: zone %d outside [0,%d)", j, node_zone[j], n_zones));
    }
    const uint32_t tail = (N & 31) ? ~0u << (N & 31) : 0u;           // bits of the last word at or beyond N
    std::vector<uint32_t> every(W, ~0u);                             // nodes that every scenario holds
    for (int s = 0; s < S; ++s) {
        const uint32_t* row = present + (size_t)s * W;
        if (row[W - 1] & tail) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: scenario %d: bits set at or beyond node %d", s, N));
        int n = 0;
        for (int w = 0; w < W; ++w) { n += __builtin_popcount(row[w]); every[w] &= row[w]; }
        if (n == 0) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: scenario %d holds no node at all", s));   // (the ranked instantiations have never run an empty scenario)
        if (n != c->scen[s].n_nodes) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: scenario %d: n_nodes %d, but its row holds %d nodes", s, c->scen[s].n_nodes, n));
    }
    auto always = [&](int j) { return (every[j >> 5] >> (j & 31)) & 1u; };
    // a node that some scenario lacks starts empty there: pods bound before the stream would need it in every scenario; a pod preset to
    // it has to vanish with it (gated on that same node) or be flagged for eviction (simon_set_pod_eviction: scheduled where the node is
    // absent).  The score-table kernel relies on this: "preset, not gated on it, node absent" is a flagged pod, it reads no flag array.
    for (int j = 0; j < N; ++j)
        if (!always(j) && node_busy(c, j)) return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: node %d, absent from some scenario, carries pods bound before the stream", j));
    for (int p = 0; p < c->P; ++p)
        if (c->p_preset[p] >= 0 && !always(c->p_preset[p]) && c->p_gate[p] != c->p_preset[p] && !evicted_pod(c, p))
            return seg_abandon(c, fail(c, SIMON_EINVAL, "set_scenario_nodes: pod %d is preset to node %d, absent from some scenario, and not gated on it", p, c->p_preset[p]));
    HIP_TRY(c, hipSetDevice(c->device));
    {
        const std::vector<uint32_t> words(present, present + (size_t)S * W);     // (also: present may be c->sub_words' own storage no longer)
        if (c->has_img)
            if (const int rc = img_own_enter(c, "set_scenario_nodes", words)) return seg_abandon(c, rc);
        c->sub_words = words;
    }
    c->seg_n = 0; c->sub_on = true; c->sub_W = W;                    // (a node-subset batch replaces segments)
    if (node_zone) c->sub_zone.assign(node_zone, node_zone + N); else c->sub_zone.clear();
    int rc = SIMON_OK;
    if (!c->subset_host) {
        hipError_t e = c->d_sub_words.upload(c->sub_words, c->stream);
        if (e == hipSuccess && node_zone) e = c->d_sub_zone.upload(c->sub_zone, c->stream);
        if (e != hipSuccess) rc = fail(c, e == hipErrorOutOfMemory ? SIMON_ENOMEM : SIMON_ENODEV, "set_scenario_nodes: %s", hipGetErrorString(e));
    }
    if (!rc) rc = subset_stage(c);
    return rc ? seg_abandon(c, rc) : SIMON_OK;
}

int simon_fetch_node_ranks(simon_ctx* c, int32_t* rank) {
    if (!c || !rank) return c ? fail(c, SIMON_EINVAL, "fetch_node_ranks: bad arguments") : SIMON_EINVAL;
    if (!c->staged || c->S <= 0 || !c->has_ranks) return fail(c, SIMON_ESTATE, "fetch_node_ranks: the loaded batch has no rank rows");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rank, c->d_node_rank.p, (size_t)c->S * c->N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

// Pod-subset batches: the presence words go to the device as given ([S][ceil(P / 32)] u32); every kernel tests the pod's bit next to its gate.
int simon_set_scenario_pods(simon_ctx* c, const uint32_t* present) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "set_scenario_pods: load scenarios first");
    if (!present) { c->pods_on = false; c->order_rows_on = false; c->have_results = false; return SIMON_OK; }
    const int S = c->S, P = c->P, W = pod_row_words(P);
    int bit = 0;
    if (const int s = pod_rows_first_bad(present, S, P, &bit); s >= 0)
        return fail(c, SIMON_EINVAL, "set_scenario_pods: scenario %d sets bit %d, the problem has %d pods", s, bit, P);
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> words(present, present + (size_t)S * W);
    DevBuf<uint32_t> fresh;                                      // (a failed upload leaves the batch as it was)
    HIP_TRY(c, fresh.upload(words, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::swap(c->d_pod_words.p, fresh.p); std::swap(c->d_pod_words.n, fresh.n);
    c->pod_W = W;
    c->pods_on = true;
    c->order_rows_on = false;                                    // (the caller's rows replace a composed batch's)
    c->have_results = false;
    return SIMON_OK;
}

int simon_fetch_group_counts(simon_ctx* c, const int32_t* pod_group, int32_t G, int32_t* unscheduled, int32_t* placed) {
    if (!c || !pod_group || !unscheduled) return c ? fail(c, SIMON_EINVAL, "fetch_group_counts: bad arguments") : SIMON_EINVAL;
    if (G < 1 || G > SIMON_MAX_POD_GROUPS) return fail(c, SIMON_EINVAL, "fetch_group_counts: %d groups outside [1, %d]", G, SIMON_MAX_POD_GROUPS);
    if (const int p = pod_groups_first_bad(pod_group, c->P, G); p >= 0)
        return fail(c, SIMON_EINVAL, "fetch_group_counts: pod %d has group %d outside [-1, %d)", p, pod_group[p], G);
    if (!c->have_results || !c->have_placement) return fail(c, SIMON_ESTATE, "fetch_group_counts: no placements on device (run with SIMON_WANT_PLACEMENT)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t S = c->S, P = c->P, cells = S * (size_t)G;
    HIP_TRY(c, c->d_pod_group.ensure(P));
    HIP_TRY(c, c->d_grp_uns.ensure(cells));
    if (placed) HIP_TRY(c, c->d_grp_placed.ensure(cells));
    HIP_TRY(c, hipMemcpyAsync(c->d_pod_group.p, pod_group, P * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_group_counts(c->d_place.p, c->d_pod_group.p, (int)S, (int)P, G, c->d_grp_uns.p, placed ? c->d_grp_placed.p : nullptr, c->stream));
    HIP_TRY(c, hipMemcpyAsync(unscheduled, c->d_grp_uns.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    if (placed) HIP_TRY(c, hipMemcpyAsync(placed, c->d_grp_placed.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (simon_stats is left alone: d2h_ms stays the last result fetch's)
    return SIMON_OK;
}

// ---- simon_fetch_node_usage / _gpu_usage / _local_usage and simon_fetch_headroom / _gpu / _local ----
static_assert(sizeof(ScenarioDesc) == 8, "the usage kernels read ScenarioDesc as int32 pairs");

// the launch arguments every usage and headroom call shares
static void usage_base(const simon_ctx* c, UsageCommon& a) {
    a.placement = c->d_place.p; a.scen = reinterpret_cast<const int32_t*>(c->d_scen.p);
    a.rank = own_nodes(c) && c->has_ranks ? c->d_node_rank.p : nullptr;
    a.P = c->P; a.N = c->N;
}

// the tile a launch of `blocks` workgroups forces (usage_tile's `forced`): SIMON_USAGE_TILE; or, where the launch puts at most one
// workgroup on a CU anyway, the largest that fits a workgroup (fewer passes over the placement row: config 5's 256 scenarios,
// profiles/usage/README.md); or 0 = the LDS budget's (four workgroups per CU)
static int usage_forced_tile(const simon_ctx* c, int blocks) { return c->usage_tile ? c->usage_tile : blocks <= c->n_cus ? 1 << 30 : 0; }

// The opening of the three listed-scenario calls, in two steps with the call's own test of its required arrays between them (no field
// behind struct_size is read before the ABI guard has passed).  First the context and the output struct: `size` = its struct_size
// (null without a struct) against the `want` of `type`.
static int usage_out_check(simon_ctx* c, const char* what, const char* type, const uint32_t* size, size_t want) {
    if (!c) return SIMON_EINVAL;
    if (!size) return fail(c, SIMON_EINVAL, "%s: bad arguments", what);
    if (*size != want) return fail(c, SIMON_EINVAL, "%s: %s size mismatch", what, type);
    return SIMON_OK;
}

// Then the scenario list and the state of the context (`devices`: the recorded devices too), the launch arguments every usage kernel
// takes and the listed ids on the device (*d_ids: null for scen_ids = null).
static int usage_open(simon_ctx* c, const char* what, const int32_t* scen_ids, int32_t n, bool devices, UsageCommon& a, const int32_t** d_ids) {
    if (n < 1) return fail(c, SIMON_EINVAL, "%s: %d scenarios listed", what, n);
    if (!c->have_results || !c->have_placement) return fail(c, SIMON_ESTATE, "%s: no placements on device (run with SIMON_WANT_PLACEMENT)", what);
    if (!scen_ids && n > c->S) return fail(c, SIMON_EINVAL, "%s: scenario %d outside [0,%d)", what, c->S, c->S);
    for (int i = 0; scen_ids && i < n; ++i)
        if (scen_ids[i] < 0 || scen_ids[i] >= c->S) return fail(c, SIMON_EINVAL, "%s: scenario %d outside [0,%d)", what, scen_ids[i], c->S);
    if (devices && c->has_gpu && !c->have_slices) return fail(c, SIMON_ESTATE, "%s: the last run did not record GPU devices (SIMON_WANT_GPU_SLICES)", what);
    HIP_TRY(c, hipSetDevice(c->device));
    usage_base(c, a);
    *d_ids = nullptr;
    if (scen_ids) {
        HIP_TRY(c, c->d_u_ids.ensure((size_t)n));
        HIP_TRY(c, hipMemcpyAsync(c->d_u_ids.p, scen_ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        *d_ids = c->d_u_ids.p;
    }
    return SIMON_OK;
}

// The compact int64 copies node_usage_kernel and headroom_kernel read (the per-family pod rows are normalised: not usable here),
// uploaded on the first call after a reload, and their launch arguments (on top of usage_base's).
static int usage_stage(simon_ctx* c, UsageCommon& a) {
    const size_t P = c->P, N = c->N;
    const int K = c->K;
    if (!c->usage_pods_staged) {
        std::vector<int64_t> h((size_t)kUsageRows * std::max<size_t>(P, 1), 0);
        c->usage_rows = 3;
        for (size_t p = 0; p < P; ++p) {
            h[p] = c->p_req_cpu[p]; h[P + p] = c->p_req_mem[p]; h[2 * P + p] = c->p_req_eph[p];
            if (c->p_req_eph[p] != 0) c->usage_rows |= 4u;
            for (int k = 0; k < K; ++k)
                if ((h[(3 + k) * P + p] = c->p_scalar[(size_t)k * P + p]) != 0) c->usage_rows |= 8u << k;
        }
        HIP_TRY(c, c->d_u_pod_req.upload(h, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));             // (h leaves scope)
        c->usage_pods_staged = true;
    }
    if (!c->usage_nodes_staged) {
        std::vector<int64_t> init((size_t)kUsageRows * N, 0), alloc((size_t)kUsageRows * N, 0);
        for (size_t j = 0; j < N; ++j) {
            init[j] = c->i_req_cpu[j]; init[N + j] = c->i_req_mem[j]; init[2 * N + j] = c->i_req_eph[j];
            alloc[j] = c->alloc_cpu[j]; alloc[N + j] = c->alloc_mem[j]; alloc[2 * N + j] = c->alloc_eph[j];
            for (int k = 0; k < K; ++k) {
                init[(3 + k) * N + j] = c->i_scalar_req[(size_t)k * N + j];
                alloc[(3 + k) * N + j] = c->scalar_alloc[(size_t)k * N + j];
            }
        }
        HIP_TRY(c, c->d_u_node_init.upload(init, c->stream));
        HIP_TRY(c, c->d_u_node_alloc.upload(alloc, c->stream));
        HIP_TRY(c, c->d_u_init_npods.upload(c->i_npods, c->stream));
        HIP_TRY(c, c->d_u_alloc_pods.upload(c->alloc_pods, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->usage_nodes_staged = true;
    }
    a.pod_req = c->d_u_pod_req.p; a.node_init = c->d_u_node_init.p; a.init_npods = c->d_u_init_npods.p;
    return SIMON_OK;
}

// the rows a launch accumulates: `rows` (bits over the resource rows) in ascending order
static void usage_rows_of(uint32_t rows, UsageCommon& a) {
    a.nrows = 0;
    for (int r = 0; r < kUsageRows; ++r)
        if ((rows >> r) & 1u) a.row_src[a.nrows++] = r;
    for (int i = a.nrows; i < kUsageRows; ++i) a.row_src[i] = -1;
}

int simon_fetch_node_usage(simon_ctx* c, const int32_t* scen_ids, int32_t n, simon_node_usage* out) {
    UsageCommon a{};
    UsageOut o{};
    if (const int rc = usage_out_check(c, "fetch_node_usage", "simon_node_usage", out ? &out->struct_size : nullptr, sizeof *out)) return rc;
    if (!out->req_cpu || !out->req_mem || !out->npods) return fail(c, SIMON_EINVAL, "fetch_node_usage: missing required arrays (req_cpu, req_mem, npods)");
    if (const int rc = usage_open(c, "fetch_node_usage", scen_ids, n, false, a, &o.scen_ids)) return rc;
    if (const int rc = usage_stage(c, a)) return rc;
    const size_t N = c->N, K = c->K, cells = (size_t)n * N;
    const bool eph = out->req_eph != nullptr, sc = out->scalar_req != nullptr && K > 0;
    usage_rows_of(3u | (eph ? 4u : 0u) | (sc ? ((1u << K) - 1u) << 3 : 0u), a);
    a.tile = usage_tile(c->N, usage_node_bytes(a.nrows), kTileReserve, usage_forced_tile(c, n));
    HIP_TRY(c, c->d_u_out64.ensure(cells * (size_t)a.nrows));
    HIP_TRY(c, c->d_u_npods.ensure(cells));
    o.npods = c->d_u_npods.p;
    int64_t* const d_sc = c->d_u_out64.p + cells * (2 + (eph ? 1 : 0));          // [n][K][N]
    for (int i = 0; i < a.nrows; ++i) {
        const int r = a.row_src[i];
        if (r < 3) { o.rows[i] = c->d_u_out64.p + cells * i; o.row_stride[i] = N; }
        else { o.rows[i] = d_sc + (size_t)(r - 3) * N; o.row_stride[i] = K * N; }
    }
    HIP_TRY(c, launch_node_usage(a, o, n, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->req_cpu, o.rows[0], cells * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->req_mem, o.rows[1], cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (eph) HIP_TRY(c, hipMemcpyAsync(out->req_eph, o.rows[2], cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (sc) HIP_TRY(c, hipMemcpyAsync(out->scalar_req, d_sc, cells * K * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->npods, c->d_u_npods.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (simon_stats is left alone, as in simon_fetch_group_counts)
    return SIMON_OK;
}

// The GPU-share arrays of both device calls, uploaded on the first call after a reload; g.slices = the last run's record (nullptr for a
// problem without any GPU request: nothing was booked).
static int usage_stage_gpu(simon_ctx* c, DevUsage& g) {
    const size_t N = c->N;
    if (!c->usage_gpu_pods_staged) {
        HIP_TRY(c, c->d_g_pod_mem.upload(c->p_gpu_mem, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->usage_gpu_pods_staged = true;
    }
    if (!c->usage_gpu_nodes_staged) {
        std::vector<int32_t> cnt(N, 0);
        std::vector<int64_t> per(N, 0), init(N * SIMON_MAX_GPU_DEV, 0);
        for (size_t j = 0; j < N && c->has_gpu_nodes; ++j) {
            if (c->gpu_cnt[j] <= 0) continue;
            cnt[j] = std::min(c->gpu_cnt[j], SIMON_MAX_GPU_DEV);
            per[j] = c->gpu_mem_total[j] / c->gpu_cnt[j];         // (by the unclamped count, as AllocateGpuId's per-device total)
            std::copy_n(c->i_gpu_used.data() + j * SIMON_MAX_GPU_DEV, SIMON_MAX_GPU_DEV, init.data() + j * SIMON_MAX_GPU_DEV);
        }
        HIP_TRY(c, c->d_g_node_cnt.upload(cnt, c->stream));
        HIP_TRY(c, c->d_g_per_dev.upload(per, c->stream));
        HIP_TRY(c, c->d_g_init_used.upload(init, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));             // (the vectors leave scope)
        c->usage_gpu_nodes_staged = true;
    }
    g.slices = c->has_gpu ? c->d_gpu_slices.p : nullptr;
    g.gpu_mem = c->d_g_pod_mem.p; g.node_cnt = c->d_g_node_cnt.p; g.per_dev = c->d_g_per_dev.p; g.init_used = c->d_g_init_used.p;
    return SIMON_OK;
}

static_assert(SIMON_MAX_GPU_DEV == kGpuDev, "the device kernels unpack one slices byte per device");

int simon_fetch_gpu_usage(simon_ctx* c, const int32_t* scen_ids, int32_t n, simon_gpu_usage* out) {
    UsageCommon a{};
    GpuUsageOut o{};
    if (const int rc = usage_out_check(c, "fetch_gpu_usage", "simon_gpu_usage", out ? &out->struct_size : nullptr, sizeof *out)) return rc;
    if (!out->dev_used) return fail(c, SIMON_EINVAL, "fetch_gpu_usage: missing required arrays (dev_used)");
    if (const int rc = usage_open(c, "fetch_gpu_usage", scen_ids, n, true, a, &o.scen_ids)) return rc;
    DevUsage g{};
    if (const int rc = usage_stage_gpu(c, g)) return rc;
    a.tile = usage_tile(c->N, usage_node_bytes(0, kDevBytes + (out->dev_pods ? kDevPodsBytes : 0)), kTileReserve, usage_forced_tile(c, n));
    const size_t cells = (size_t)n * c->N * SIMON_MAX_GPU_DEV;
    HIP_TRY(c, c->d_g_out_used.ensure(cells));
    o.dev_used = c->d_g_out_used.p;
    if (out->dev_pods) { HIP_TRY(c, c->d_g_out_pods.ensure(cells)); o.dev_pods = c->d_g_out_pods.p; }
    HIP_TRY(c, launch_gpu_usage(a, g, o, n, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->dev_used, o.dev_used, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (out->dev_pods) HIP_TRY(c, hipMemcpyAsync(out->dev_pods, o.dev_pods, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (simon_stats is left alone, as in simon_fetch_node_usage)
    return SIMON_OK;
}

static_assert(sizeof(LocalSpec) == sizeof(simon_local_spec) && offsetof(LocalSpec, hdd_size) == offsetof(simon_local_spec, hdd_size) &&
              offsetof(LocalSpec, lvm_vg) == offsetof(simon_local_spec, lvm_vg), "the storage kernels read simon_local_spec as LocalSpec");
static_assert(SIMON_MAX_VG == kLocalVG && SIMON_MAX_LDEV == kLocalDev && SIMON_MAX_LVOL == kLocalVol, "the storage kernels' array sizes");

// the Open-Local spec of pod class cls: its index in l_specs, or -1 (none, or no volume at all: local_spec_of of the oracle)
static int local_spec_index(const simon_ctx* c, int cls) {
    if ((size_t)cls >= c->l_spec_of.size() || c->l_spec_of[cls] < 0) return -1;
    const simon_local_spec& sp = c->l_specs[c->l_spec_of[cls]];
    return sp.n_lvm + sp.n_ssd + sp.n_hdd > 0 ? c->l_spec_of[cls] : -1;
}

// The Open-Local arrays of both storage calls, uploaded on the first call after a reload.  A problem without Open-Local leaves l.flags
// null: the kernels replay nothing and bound nothing.
static int local_stage(simon_ctx* c, LocalUsage& l) {
    if (!c->has_local) return SIMON_OK;
    const size_t P = c->P;
    if (!c->local_nodes_staged) {
        HIP_TRY(c, c->d_l_flags.upload(c->l_flags, c->stream));
        HIP_TRY(c, c->d_l_vg_cnt.upload(c->l_vg_cnt, c->stream));
        HIP_TRY(c, c->d_l_vg_cap.upload(c->l_vg_cap, c->stream));
        HIP_TRY(c, c->d_l_vg_init.upload(c->l_vg_req, c->stream));
        HIP_TRY(c, c->d_l_vg_name.upload(c->l_vg_name, c->stream));
        HIP_TRY(c, c->d_l_dev_cnt.upload(c->l_dev_cnt, c->stream));
        HIP_TRY(c, c->d_l_dev_cap.upload(c->l_dev_cap, c->stream));
        HIP_TRY(c, c->d_l_dev_media.upload(c->l_dev_media, c->stream));
        HIP_TRY(c, c->d_l_dev_init.upload(c->l_dev_alloc, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->local_nodes_staged = true;
    }
    if (!c->local_pods_staged) {
        std::vector<LocalSpec> specs(c->l_specs.size());
        if (!specs.empty()) memcpy(specs.data(), c->l_specs.data(), specs.size() * sizeof(LocalSpec));
        std::vector<int32_t> pod_spec(P, -1), list, off((size_t)c->n_orders + 1, 0);
        for (size_t p = 0; p < P; ++p)
            if (c->p_preset[p] < 0) pod_spec[p] = local_spec_index(c, c->p_cls[p]);
        for (int o = 0; o < c->n_orders; ++o) {
            for (size_t i = 0; i < P; ++i) {
                const int32_t p = c->h_orders[(size_t)o * P + i];
                if (pod_spec[p] >= 0) list.push_back(p);
            }
            off[o + 1] = (int32_t)list.size();
        }
        HIP_TRY(c, c->d_l_specs.upload(specs, c->stream));
        HIP_TRY(c, c->d_l_pod_spec.upload(pod_spec, c->stream));
        HIP_TRY(c, c->d_l_list.upload(list, c->stream));
        HIP_TRY(c, c->d_l_list_off.upload(off, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));             // (the vectors leave scope)
        c->local_pods_staged = true;
    }
    l.specs = c->d_l_specs.p; l.pod_spec = c->d_l_pod_spec.p; l.list = c->d_l_list.p; l.list_off = c->d_l_list_off.p;
    l.flags = c->d_l_flags.p; l.vg_cnt = c->d_l_vg_cnt.p; l.vg_cap = c->d_l_vg_cap.p; l.vg_init = c->d_l_vg_init.p; l.vg_name = c->d_l_vg_name.p;
    l.dev_cnt = c->d_l_dev_cnt.p; l.dev_cap = c->d_l_dev_cap.p; l.dev_media = c->d_l_dev_media.p; l.dev_init = c->d_l_dev_init.p;
    return SIMON_OK;
}

// The bounds of a headroom call: resources = simon_fetch_headroom, devices = simon_fetch_headroom_gpu (the device bound on top), storage =
// simon_fetch_headroom_local: the storage bound on top, and the device bound under simon_fetch_headroom_gpu's rule where the problem has
// GPU requests or GPU nodes (a problem without GPUs pays no device LDS).
enum class Headroom { resources, devices, storage };
static bool headroom_devices(const simon_ctx* c, Headroom bounds) {
    return bounds == Headroom::devices || (bounds == Headroom::storage && (c->has_gpu || c->has_gpu_nodes));
}

// the three headroom calls (`what` names the call in messages)
static int fetch_headroom(simon_ctx* c, const int32_t* probe_pod, int32_t K, int64_t* fit, int32_t* fit_nodes, uint8_t* exact, Headroom bounds,
                          const char* what) {
    if (!c) return SIMON_EINVAL;
    const bool devices = headroom_devices(c, bounds), storage = bounds == Headroom::storage;
    if (!probe_pod || !fit) return fail(c, SIMON_EINVAL, "%s: missing required arrays (probe_pod, fit)", what);
    if (K < 1 || K > SIMON_MAX_PROBES) return fail(c, SIMON_EINVAL, "%s: %d probes outside [1, %d]", what, K, SIMON_MAX_PROBES);
    if (!c->have_results || !c->have_placement) return fail(c, SIMON_ESTATE, "%s: no placements on device (run with SIMON_WANT_PLACEMENT)", what);
    for (int k = 0; k < K; ++k)
        if (probe_pod[k] < 0 || probe_pod[k] >= c->P) return fail(c, SIMON_EINVAL, "%s: probe %d: pod %d outside [0,%d)", what, k, probe_pod[k], c->P);
    if (devices && c->has_gpu && !c->have_slices) return fail(c, SIMON_ESTATE, "%s: the last run did not record GPU devices (SIMON_WANT_GPU_SLICES)", what);
    HIP_TRY(c, hipSetDevice(c->device));
    UsageCommon a{};
    usage_base(c, a);
    if (const int rc = usage_stage(c, a)) return rc;
    DevUsage g{};
    if (devices)
        if (const int rc = usage_stage_gpu(c, g)) return rc;
    LocalUsage l{};
    if (storage)
        if (const int rc = local_stage(c, l)) return rc;
    usage_rows_of(c->usage_rows, a);
    const HeadroomLds lds{a.nrows, K, devices, storage};
    a.tile = usage_tile(c->N, lds.node_bytes(), lds.reserve_bytes(), usage_forced_tile(c, c->S));
    // the probe rows: request, the resources fitsRequest compares (fit.go:244-299), the class's static mask
    const size_t S = c->S, N = c->N, W = (N + 63) / 64, P = c->P;
    std::vector<ProbeRow> rows((size_t)K);
    std::vector<uint64_t> mask((size_t)K * W, ~0ull);
    std::vector<int64_t> gmem((size_t)K, 0);
    std::vector<int32_t> gcnt((size_t)K, 0), lspec((size_t)K, -1);
    auto none = [](const std::vector<int32_t>& off, int cls) { return (size_t)cls + 1 >= off.size() || off[cls + 1] == off[cls]; };
    for (int k = 0; k < K; ++k) {
        const int p = probe_pod[k], cls = c->p_cls[p];
        ProbeRow& r = rows[k];
        r = ProbeRow{};
        r.q[0] = c->p_req_cpu[p]; r.q[1] = c->p_req_mem[p]; r.q[2] = c->p_req_eph[p];
        uint32_t entries = c->p_entries.empty() ? 0u : c->p_entries[p];
        for (int i = 0; i < c->K; ++i) {
            r.q[3 + i] = c->p_scalar[(size_t)i * P + p];
            if (r.q[3 + i] != 0) entries |= 1u << i;             // a non-zero quantity IS an entry
        }
        const bool shortcut = r.q[0] == 0 && r.q[1] == 0 && r.q[2] == 0 && entries == 0;
        r.checked = shortcut ? 0u : 7u | ((entries & ((1u << c->K) - 1u)) << 3);
        if (c->has_mask) std::copy_n(c->static_mask.data() + (size_t)cls * W, W, mask.data() + (size_t)k * W);
        // the device bound: a GPU request without a gpu-index annotation (such a pod short-cuts AllocateGpuId: no bound, not exact)
        const bool bound = devices && c->p_gpu_mem[p] > 0 && c->p_gpu_index[p] == 0;
        if (bound) { gmem[k] = c->p_gpu_mem[p]; gcnt[k] = std::min(c->p_gpu_cnt[p], 64); }
        if (exact)
            exact[k] = (bound || (c->p_gpu_mem[p] == 0 && c->p_gpu_cnt[p] == 0 && c->p_gpu_index[p] == 0)) && c->p_pin[p] < 0 && c->p_preset[p] < 0 &&
                       none(c->match_off, cls) && none(c->anti_off, cls) && none(c->port_off, cls) && none(c->aff_off, cls) && none(c->sh_off, cls) &&
                       (storage || (size_t)cls >= c->l_spec_of.size() || c->l_spec_of[cls] < 0);
        if (storage && c->has_local) lspec[k] = local_spec_index(c, cls);
    }
    HeadroomArgs h{};
    const size_t cells = S * (size_t)K;
    HIP_TRY(c, c->d_u_probes.upload(rows, c->stream));
    HIP_TRY(c, c->d_u_probe_mask.upload(mask, c->stream));
    HIP_TRY(c, c->d_u_fit.ensure(cells));
    if (fit_nodes) HIP_TRY(c, c->d_u_fit_nodes.ensure(cells));
    h.node_alloc = c->d_u_node_alloc.p; h.alloc_pods = c->d_u_alloc_pods.p; h.probes = c->d_u_probes.p; h.probe_mask = c->d_u_probe_mask.p;
    h.K = K; h.fit = c->d_u_fit.p; h.fit_nodes = fit_nodes ? c->d_u_fit_nodes.p : nullptr;
    if (devices) {
        HIP_TRY(c, c->d_g_probe_mem.upload(gmem, c->stream));
        HIP_TRY(c, c->d_g_probe_cnt.upload(gcnt, c->stream));
        g.probe_mem = c->d_g_probe_mem.p; g.probe_cnt = c->d_g_probe_cnt.p;
    }
    if (storage) {
        HIP_TRY(c, c->d_l_probe_spec.upload(lspec, c->stream));
        l.probe_spec = c->d_l_probe_spec.p;
    }
    HIP_TRY(c, launch_headroom(a, h, g, l, devices, storage, (int)S, c->stream));
    HIP_TRY(c, hipMemcpyAsync(fit, c->d_u_fit.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    if (fit_nodes) HIP_TRY(c, hipMemcpyAsync(fit_nodes, c->d_u_fit_nodes.p, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (also: rows and mask outlive their uploads)
    return SIMON_OK;
}

int simon_fetch_headroom(simon_ctx* c, const int32_t* probe_pod, int32_t K, int64_t* fit, int32_t* fit_nodes, uint8_t* exact) {
    return fetch_headroom(c, probe_pod, K, fit, fit_nodes, exact, Headroom::resources, "fetch_headroom");
}

int simon_fetch_headroom_gpu(simon_ctx* c, const int32_t* probe_pod, int32_t K, int64_t* fit, int32_t* fit_nodes, uint8_t* exact) {
    return fetch_headroom(c, probe_pod, K, fit, fit_nodes, exact, Headroom::devices, "fetch_headroom_gpu");
}

int simon_fetch_headroom_local(simon_ctx* c, const int32_t* probe_pod, int32_t K, int64_t* fit, int32_t* fit_nodes, uint8_t* exact) {
    return fetch_headroom(c, probe_pod, K, fit, fit_nodes, exact, Headroom::storage, "fetch_headroom_local");
}

int simon_fetch_local_usage(simon_ctx* c, const int32_t* scen_ids, int32_t n, simon_local_usage* out) {
    UsageCommon a{};
    LocalUsageOut o{};
    if (const int rc = usage_out_check(c, "fetch_local_usage", "simon_local_usage", out ? &out->struct_size : nullptr, sizeof *out)) return rc;
    if (!out->vg_req) return fail(c, SIMON_EINVAL, "fetch_local_usage: missing required arrays (vg_req)");
    if (const int rc = usage_open(c, "fetch_local_usage", scen_ids, n, false, a, &o.scen_ids)) return rc;
    LocalUsage l{};
    if (const int rc = local_stage(c, l)) return rc;
    a.tile = usage_tile(c->N, kLocalBytes, kTileReserve + kLocalStageBytes, usage_forced_tile(c, n));
    const size_t cells = (size_t)n * c->N;
    HIP_TRY(c, c->d_l_out_vg.ensure(cells * SIMON_MAX_VG));
    o.vg_req = c->d_l_out_vg.p;
    if (out->dev_alloc) { HIP_TRY(c, c->d_l_out_dev.ensure(cells)); o.dev_alloc = c->d_l_out_dev.p; }
    HIP_TRY(c, launch_local_usage(a, l, o, n, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->vg_req, o.vg_req, cells * SIMON_MAX_VG * 8, hipMemcpyDeviceToHost, c->stream));
    if (out->dev_alloc) HIP_TRY(c, hipMemcpyAsync(out->dev_alloc, o.dev_alloc, cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                 // (simon_stats is left alone, as in simon_fetch_node_usage)
    return SIMON_OK;
}

// The all-feature kernel gives every problem its failure codes and runs the batches no other kernel takes: staged on first use where
// stage() chose another kernel.
static int ensure_wide_staged(simon_ctx* c) {
    const int rc = c->wide_staged ? SIMON_OK : wide_stage(c->wide, *c, c->stream, c->err);
    c->wide_staged = rc == SIMON_OK;
    return rc;
}

// Workgroup shape of the all-feature kernel for a batch of S scenarios (a run, or simon_explain_batch's replays).  A 256-thread
// group fits twice on a CU (launch bounds 256 x 2: two independent barrier domains per SIMD), which wins as soon as the batch
// offers two groups per CU; with fewer scenarios than that a CU holds ONE group and the 512-thread shape keeps all four SIMDs at
// two waves.  Measured on config 5 (50 000 pods x 2 500..5 000 nodes): S = 256: 512 threads 536 ms, 256 threads 734 ms;
// S = 1 024: 512 threads 2 033 ms, 256 threads 1 611 ms.  SIMON_WG overrides (tuning knob).
static int wide_workgroup(const simon_ctx* c, int S, int max_n) {
    const bool two_groups = S >= 2 * c->n_cus && max_n <= 8192;          // 32 nodes per lane at most
    const int T = c->force_T ? c->force_T : (max_n <= 1024 || two_groups ? 256 : max_n <= 16384 ? 512 : 1024);
    return T == 128 ? 256 : T;                                  // (SIMON_WG=128: the all-feature kernel is built for 64 / 256 / 512 / 1 024 threads since round 5)
}

// Where a loaded batch runs and in which shape: route_batch decides, simon_run_loaded's launchers carry it out ("Which kernel runs what")
struct BatchRoute {
    int kernel;            // SIMON_KERNEL_*: the kernel that runs the batch
    int generation;        // simon_stats.kernel_generation (0: the all-feature kernel)
    int T, slots;          // threads per workgroup; node slots per lane (score table: 64-lane rounds over the summary entries)
    int team;              // score table: waves per scenario, 1 or kTeamWaves
    bool lds_ws, lds_x;    // score table: the workspace (generation 4) / the mask rows (generation 6) live in LDS
    size_t lds;            // dynamic LDS of the launch
};

// dynamic LDS of a score-table launch with an LDS-resident home: the kernel puts it at the next 128-byte boundary behind tcarve's total
static size_t lds_with_home(const simon_ctx* c, size_t table_lds, size_t home) { return ((table_lds - c->lds_pad + 127) & ~(size_t)127) + home + c->lds_pad; }

// The route of the loaded batch, from the staged problem and the batch alone: no HIP call, nothing written to the context
// (SIMON_DEBUG_ROUTE: the `[route] variant` line on stderr).
static BatchRoute route_batch(const simon_ctx* c) {
    const int S = c->S;
    // (an own-nodes batch that the context's opt-in lets run on the all-feature kernel walks the pool: its workgroup is sized by N.  With the
    // option off such a batch is refused, and its route is what it was)
    auto wide = [&](int slots) { return BatchRoute{SIMON_KERNEL_WIDE, 0, wide_workgroup(c, S, own_nodes(c) && c->own_wide ? c->N : c->max_n), slots, 1, false, false, 0}; };
    // per-scenario node ranks: the score-table kernel (own per-class lists) or the all-feature kernel
    if (c->variant != SIMON_KERNEL_NARROW || (c->has_ranks && !c->table_ranks_ok)) return wide(0);
    // workgroup shape: T = 256 (4 waves) with up to 8 node slots per lane covers 2048 nodes;
    // larger pools widen the workgroup.  SIMON_WG overrides (tuning knob).
    const int T = c->force_T ? c->force_T : (c->max_n <= 2048 ? 256 : c->max_n <= 4096 ? 512 : 1024);
    int slots = (std::max(c->max_n, 1) + T - 1) / T;
    const bool too_big = slots > 8;   // pool too large for register residency even at T = 1024: the all-feature kernel takes it
    if (slots == 5) slots = 6;
    if (slots == 7) slots = 8;
    // the score-table kernel: one workgroup (one wave) per scenario, ONE launch, scenarios in LPT order
    const int ni_top = c->table_ni_top;
    // team mode: a small batch of a problem with soft spread constraints gets kTeamWaves waves per scenario (the walks of
    // spread_select and the prologue are split; LDS: + one score table, the canonical indices and the exchange slots)
    const int team_max = c->team_max_s >= 0 ? c->team_max_s : 2 * c->n_cus;
    int team = (c->spread && c->table_coarse && (!c->rest || c->rs) && c->team_mode != 0 && (c->team_mode > 0 || S <= team_max)) ? kTeamWaves : 1;
    auto lds_for = [&](int tm) -> size_t { return c->table_ok ? table_lds_bytes(c->n_sigs, ni_top, c->Cn_t, c->table_coarse, c->rest, spread_lds_word(c, tm)) + c->lds_pad : 0; };
    if (team > 1 && lds_for(team) > kTableLdsMaxWG) team = 1;           // (its extra table does not fit: the single-wave shape still may)
    size_t table_lds = lds_for(team);
    // The LDS-resident homes (LDSWS, LDSX) trade occupancy for latency: a workgroup asks for up to 159 KB, so a CU holds ONE.  They are
    // the default only where that costs nothing whatever the dispatcher does: a batch of at most one scenario per CU (what a real
    // Applier.Run offers).  Round 5 also took batches of a few workgroups per CU when ceil(S / CUs) of them fit the CU's LDS together --
    // which assumed the dispatcher places exactly that many per CU, and left simon_load_scenarios' fine / coarse cost model (lds16 /
    // lds64, fitted before this LDS growth) describing another launch; those batches keep the HBM homes now (SIMON_LDS_WS=1: whenever
    // one scenario fits).
    auto lds_home = [&](size_t need) { return need <= kTableLdsMaxWG && c->ldsws_mode != 0 && (c->ldsws_mode > 0 || S <= std::max(c->n_cus, 1)); };
    // Generation 4 with the scenario's workspace in LDS (round 5; simon_table.hip: LDSWS), for a problem whose byte table + node state
    // fit the CU's LDS next to the summaries: the one memory round trip of a scheduling cycle becomes an LDS access
    bool lds_ws = false;
    if (c->table_ok && !c->table_coarse && !c->rest && !c->spread && !c->fold && !c->gfold && c->n_sigs <= 128 && c->Cn_t <= 128 && team == 1) {
        size_t ws_max = 0;
        for (int s = 0; s < S; ++s) ws_max = std::max(ws_max, table_ws_bytes(c->n_sigs, c->scen_ni[s], c->nzeq, false, c->Cn_t, 0, 0, 0, 0));
        const size_t need = lds_with_home(c, table_lds, ws_max);
        if (lds_home(need)) { lds_ws = true; table_lds = need; }
    }
    // Generation 6 with its mask rows, row totals and canonical indices in LDS (round 5; simon_table.hip: LDSX), under the same rule
    bool lds_x = false;
    if (c->table_ok && c->table_coarse && c->rest && !c->spread && team == 1 && c->Cn_t <= kTableMaxClasses && c->n_sigs <= 128) {   // (65 .. 128 node classes: the rows stay in HBM, simon_table_rest2.hip)
        const size_t need = lds_with_home(c, table_lds, table_ldsx_bytes(ni_top, c->rest_M));
        if (lds_home(need)) { lds_x = true; table_lds = need; }
    }
    bool use_table = c->table_ok && c->table_perm_ok && (c->Cn_t <= 128 || (!c->table_coarse && !c->fold && !c->gfold && c->n_sigs <= 128)) && !c->no_cache && !c->force_v1 && c->max_n <= (c->table_coarse ? kTableMaxNodesCoarse : kTableMaxNodes) &&
                     ni_top <= (c->table_coarse ? kTableMaxPaddedCoarse : kTableMaxPadded) && table_lds <= ((c->table_coarse || lds_ws) ? kTableLdsMaxWG : (size_t)64 * 1024);
    if (c->debug_route)
        fprintf(stderr, "[route] variant %d rest %d spread %d fold %d gfold %d table_ok %d perm_ok %d coarse %d n_sigs %d Cn_t %d ni_top %d lds %zu max_n %d M %d NZ %d TH %d TZ %d segments %d\n", c->variant, (int)c->rest,
                (int)c->spread, (int)c->fold, (int)c->gfold, (int)c->table_ok, (int)c->table_perm_ok, (int)c->table_coarse, c->n_sigs, c->Cn_t, ni_top, table_lds, c->max_n,
                c->rest_M, (int)c->zone_keys.size(), c->sp_TH, c->sp_TZ, c->seg_n);
    // pinned pods (pin_node) are known to the score-table kernel and the all-feature kernel only
    const bool needs_table_or_wide = c->has_pin || too_big || c->rest || c->spread || c->fold || c->gfold || !c->raw_fits_lds || c->has_ranks || c->has_static;
    const bool fast = c->fast_ok && !c->force_v1 && T >= 128;      // generation 2 is built for 128 threads and more
    // Beyond 256 signatures generation 2 (register-resident state, every node re-evaluated per cycle: its time does not depend on
    // the signature count) overtakes the score table (measured, profiles/r03: 300 signatures 124 ms against 119 ms, 384: 169 ms) --
    // where it is eligible; otherwise the table (K <= 384) still beats the all-feature kernel by far.
    if (use_table && c->n_sigs > 256 && !needs_table_or_wide && fast && !c->force_table) use_table = false;
    if (use_table)
        return BatchRoute{SIMON_KERNEL_NARROW_CACHE, c->spread ? 7 : c->rest ? 6 : c->table_coarse ? 5 : 4, 64 * team, (ni_top / (c->table_coarse ? 64 : 16) + 63) / 64, team, lds_ws, lds_x, table_lds};
    if (needs_table_or_wide) return wide(slots);                   // (simon_stats keeps the slot count weighed here)
    // the register-resident kernels: simon_raw in LDS, generation 2 with its second copy
    const size_t raw = (size_t)c->Cp * c->Cn * sizeof(int32_t);
    if (fast) return BatchRoute{SIMON_KERNEL_NARROW_FAST, 2, T, slots, 1, false, false, (raw * 2 + 15) & ~(size_t)15};
    return BatchRoute{SIMON_KERNEL_NARROW, 1, T, slots, 1, false, false, (raw + 15) & ~(size_t)15};
}

// SIMON_DEBUG_ROUTE: what became of a segmented batch
static void trace_segmented(const simon_ctx* c, const char* outcome) {
    if (c->debug_route && c->seg_n) fprintf(stderr, "[route] segmented batch (%d segments, %d fixed nodes): %s\n", c->seg_n, c->seg_start[0], outcome);
    if (c->debug_route && c->sub_on) fprintf(stderr, "[route] node-subset batch (%s staging): %s\n", c->subset_host ? "host" : "device", outcome);
}

// The launchers of simon_run_loaded, one per kernel: the loaded batch on route `r`, its launches between the context's event pair.
static int run_wide_batch(simon_ctx* c, const BatchRoute& r, bool want_placement, bool want_slices) {
    if (int rc = ensure_wide_staged(c)) return rc;   // (a NARROW problem whose batch cannot use the cache kernel but has pinned pods)
    const bool own = own_nodes(c);                   // (simon_run_loaded let it through: the option is on and the rank rows are staged)
    return timed_launch(c, [&] {
        return wide_run(c->wide, *c, reinterpret_cast<const WideScenario*>(c->d_scen.p), c->S, c->d_orders.p, own ? c->N : c->max_n, r.T, c->d_unsched.p,
                        c->d_used_cpu.p, c->d_used_mem.p, c->d_used_vg.p, want_placement ? c->d_place.p : nullptr,
                        c->has_ranks ? c->d_node_rank.p : nullptr, c->has_ranks ? c->d_node_inv.p : nullptr,
                        want_slices ? c->d_gpu_slices.p : nullptr, c->stream, c->err, pod_rows(c), c->pod_W, own);
    });
}

// the score-table kernel's device-resident pointer block for the loaded batch (TableCold::prof: run_table_batch)
static TableCold table_cold(const simon_ctx* c, bool want_slices) {
    TableCold cold{};
    cold.ncls = c->d_t_ncls.p; cold.rank = c->d_rank.p; cold.cls_off = c->d_cls_off.p;
    cold.clsprefix = c->d_clsprefix.p; cold.a_pods = c->d_a_pods.p;
    cold.i_rq_cpu = c->d_i_rq_cpu.p; cold.i_rq_mem = c->d_i_rq_mem.p; cold.i_nz_cpu = c->d_i_nz_cpu.p; cold.i_nz_mem = c->d_i_nz_mem.p;
    cold.foldx = c->fold ? c->d_foldx.p : nullptr; cold.i_npods = c->d_i_npods.p; cold.sigs = c->d_sigs.p; cold.shapes = c->d_shapes.p; cold.scen = c->d_scen.p;
    cold.static_mask = c->has_mask ? c->d_t_mask.p : nullptr; cold.simon_raw = c->d_t_raw.p;
    cold.unscheduled = c->d_unsched.p; cold.used_cpu = c->d_used_cpu.p; cold.used_mem = c->d_used_mem.p;
    cold.N = c->N;
    cold.gpu_slices = want_slices ? reinterpret_cast<unsigned long long*>(c->d_gpu_slices.p) : nullptr;
    cold.na_raw = c->has_na ? c->d_t_na.p : nullptr; cold.tt_raw = c->has_tt ? c->d_t_tt.p : nullptr; cold.add_raw = c->has_add ? c->d_t_add.p : nullptr;
    if (c->has_ranks) { cold.rk_pos = c->d_rk_pos.p; cold.rk_rank = c->d_node_rank.p; }
    if (own_nodes(c)) cold.scls = c->d_scls.p;
    if (c->pods_on) { cold.pod_present = c->d_pod_words.p; cold.pp_words = c->pod_W; }
    if (c->img_R > 0) { cold.img = c->d_t_img.p; cold.img_slot = c->d_img_slot.p; cold.img_stride = c->img_stride_t; }
    if (c->rest) { cold.xrows = c->d_xrows.p; cold.zdom = c->d_zdom.p; cold.xsig = c->d_xsig.p; cold.xalloc = c->d_xalloc.p; cold.i_xused = c->d_i_xused.p; cold.gsig = c->d_gsig.p; }
    if (c->rest || c->gfold) { cold.gpu_cnt = c->d_gpu_cnt.p; cold.gpu_devtot = c->d_gpu_devtot.p; cold.i_gused = c->d_i_gused.p; }
    if (c->spread) {
        cold.sp_ent = (const int2*)c->d_sp_ent.p; cold.spread_log = c->d_spread_log.p;
        cold.node_sets = c->d_node_sets.p; cold.set_words = (c->N + 63) / 64; cold.cls_zdom = c->d_cls_zdom.p;
        if (c->rest) cold.sp_word = c->d_sp_word.p;
    }
    return cold;
}

// TableScalars::static_tables of the loaded batch
static int32_t table_static_bits(const simon_ctx* c, bool want_slices) {
    return (c->has_na ? kStNa : 0) | (c->has_tt ? kStTt : 0) | (c->has_add ? kStAdd : 0) | (want_slices ? kStGpuSlices : 0) | (c->sig_twins ? kStTwins : 0) |
           (c->fold ? kStFold : 0) | ((c->spread && (c->ipa_fold || c->hard_fold)) ? kStSpreadAff : 0) | (c->gfold ? kStGpuFold : 0) | (c->img_R > 0 ? kStImg : 0) |
           (own_nodes(c) ? kStSegments : 0) | (c->pods_on ? kStPodSets : 0) | (c->no_size_dispatch ? kStOneSize : 0);
}

static TableScalars table_scalars(const simon_ctx* c, bool want_slices) {
    TableScalars sc{};
    sc.mask_words = (c->N + 63) / 64;
    sc.Cn = c->Cn_t;
    sc.Cp = c->Cp;
    sc.P = c->P;
    sc.S = c->S;
    sc.K = c->n_sigs;
    sc.rk_stride = c->has_ranks ? c->N : 0;
    sc.static_tables = table_static_bits(c, want_slices);
    sc.NZ = c->rest ? (int)c->zone_keys.size() : 0;
    sc.M = c->rest ? c->rest_M : 0;
    sc.G = c->rest ? c->rest_G : 0;
    sc.X = c->rest ? c->rest_X : 0;
    sc.TH = c->spread ? c->sp_TH : 0;
    sc.TZ = c->spread ? c->sp_TZ : 0;
    sc.NZK = c->spread ? (int)c->sp_zkeys.size() : 0;
    sc.ni_max = c->table_ni_top;
    sc.g_cpu = c->g_cpu;
    sc.g_mem = c->g_mem;
    return sc;
}

// SIMON_TABLE_PROF (profile builds only): mean ticks per scheduling cycle over the batch that just ran, by phase
static int report_table_prof(simon_ctx* c) {
    const int S = c->S, P = c->P;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> hp((size_t)S * 24);
    HIP_TRY(c, hipMemcpy(hp.data(), c->d_table_prof.p, hp.size() * 8, hipMemcpyDeviceToHost));
    double acc[24] = {0};
    for (int s = 0; s < S; ++s) for (int q = 0; q < 24; ++q) acc[q] += (double)hp[(size_t)s * 24 + q];
    // the prologue (slots 22 / 23, stamped once per scenario): ticks per scenario, and its share of everything the wave stamped
    double all = 0;
    for (double a : acc) all += a;
    all -= acc[7] + (c->rest ? acc[20] : 0.0) + acc[23];              // (7 and REST's 20 count events; 23 is a part of 22)
    fprintf(stderr, "[SIMON_TABLE_PROF] S=%d ticks/scenario: prologue %.0f (%.2f %% of the wave's %.0f) | of it the table pass %.0f (%.2f %%)\n",
            S, acc[22] / S, all > 0 ? 100.0 * acc[22] / all : 0.0, all / S, acc[23] / S, all > 0 ? 100.0 * acc[23] / all : 0.0);
    for (double& a : acc) a = a / S / P;
    fprintf(stderr, "[SIMON_TABLE_PROF] S=%d ticks/cycle: loop %.0f | row+summary read %.0f | key+wavemax %.0f | tie check %.0f | lds(shape,sn) %.0f | mem(state,row) %.0f | state update %.0f | eval+patch+store %.0f | REST assume %.0f | REST select %.0f | canonical tie-breaks per cycle %.3f\n",
            S, acc[0], acc[1], acc[2], acc[3], acc[4], acc[5] + ((c->rest || c->spread) ? 0.0 : acc[20]), acc[8], acc[9], acc[6], acc[10], acc[7]);
    if (!c->rest && !c->spread)                                       // (straight-line instantiations: slot 20 splits the memory wait, slot 5 is the rest of it)
        fprintf(stderr, "[SIMON_TABLE_PROF] S=%d ticks/cycle, of mem(state,row): state arrived %.0f | row and byte arrived after it %.0f\n", S, acc[20], acc[5]);
    if (c->rest)
        fprintf(stderr, "[SIMON_TABLE_PROF] REST select, ticks/cycle (averaged over ALL pods): pod row %.0f | filter words + summaries %.0f | candidates %.0f | table rows of excluded bests %.0f (needed on %.3f of the cycles) | per-class best %.0f | class term %.0f | totals + tie %.0f | rest %.0f\n",
                acc[11], acc[12], acc[13], acc[14], acc[20], acc[15], acc[16], acc[17], acc[10]);
    if (c->spread)
        fprintf(stderr, "[SIMON_TABLE_PROF] spread pods, ticks/cycle: entries arrived %.0f | descriptor + first loads %.0f | counters, sizes %.0f | zone counters, Log, raw table %.0f | pass 1 %.0f | extremes, totals table %.0f | pass 2 %.0f | winner %.0f | counter stores %.0f\n",
                acc[21], acc[12], acc[13], acc[14], acc[15], acc[16], acc[17], acc[18], acc[19]);
    return SIMON_OK;
}

static int run_table_batch(simon_ctx* c, const BatchRoute& r, bool want_placement, bool want_slices) {
    const int S = c->S, P = c->P;
    HIP_TRY(c, c->d_ws.ensure(c->ws_total));
    if (const char* fill = getenv("SIMON_WS_FILL"))          // debugging aid: the workspace starts from a byte pattern (a read of something the prologue never wrote shows)
        HIP_TRY(c, hipMemsetAsync(c->d_ws.p, atoi(fill), c->ws_total, c->stream));
    if (want_placement) HIP_TRY(c, c->d_place_step.ensure((size_t)S * P));
    TableCold cold = table_cold(c, want_slices);
    TableLaunch f{};
    f.team = r.team; f.lds_ws = r.lds_ws; f.lds_x = r.lds_x;
    f.coarse = c->table_coarse; f.rest = c->rest; f.spread = c->spread; f.aff = c->rest && !c->aff_idx.empty(); f.nzeq = c->nzeq; f.has_pin = c->has_pin;
    f.sc = table_scalars(c, want_slices);
    // Prefix scenarios in canonical order on the one-level kernels take their initial table from an image of the largest scenario, written once per run (not
    // kept across runs: the initial state may change between them, and the image costs a launch of microseconds)
    const bool shared_pro = !c->no_shared_prologue && c->pro_nb > 0 && !c->has_ranks && !own_nodes(c) && table_shared_prologue(f);
    if (shared_pro) {
        HIP_TRY(c, c->d_pro_image.ensure(c->pro_bytes));
        cold.pro_image = c->d_pro_image.p; cold.pro_seg = c->d_pro_seg.p; cold.pro_nb = c->pro_nb; cold.pro_n = c->max_n;
    }
    if (c->table_prof) { HIP_TRY(c, c->d_table_prof.ensure((size_t)S * 24)); HIP_TRY(c, hipMemsetAsync(c->d_table_prof.p, 0, (size_t)S * 192, c->stream)); cold.prof = c->d_table_prof.p; }
    HIP_TRY(c, c->d_table_cold.ensure(sizeof cold));
    HIP_TRY(c, hipMemcpyAsync(c->d_table_cold.p, &cold, sizeof cold, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));             // `cold` is a stack object
    f.cold = reinterpret_cast<const TableCold*>(c->d_table_cold.p);
    f.cls_list = c->has_ranks ? c->d_rk_ids.p : c->d_cls_list.p; f.pods = c->d_podsC.p; f.orders = c->d_orders.p; f.perm = c->d_perm.p;
    f.place_step = want_placement ? c->d_place_step.p : nullptr;
    f.ws_off = c->d_ws_off.p; f.ws = c->d_ws.p;
    if (c->debug_route) {
        // entries per lane of the launch, and the scenarios that scan fewer because their own padded size fits (table_kernel: LO)
        char own[64] = "none";
        if (const int lo = table_entries_own_size(f)) {
            int fits = 0;
            for (int s = 0; s < S; ++s) fits += c->scen_ni[s] <= 1024 * lo;
            if (c->no_size_dispatch) snprintf(own, sizeof own, "off");
            else snprintf(own, sizeof own, "%d of %d scenarios at %d", fits, S, lo);
        }
        fprintf(stderr, "[route] unit %s nzeq %d team %d prologue %s entries/lane %d (own size: %s) re-base %s twins %d\n", table_unit_name(f), (int)f.nzeq, f.team,
                shared_pro ? "shared-image" : "per-scenario", table_entries_per_lane(f), own, table_rebase_at_event(f) ? "at-event" : "at-use",
                (int)((f.sc.static_tables & kStTwins) != 0));
    }
    trace_segmented(c, "score-table kernel, ranked instantiation");
    if (int rc = timed_launch(c, [&] {
            if (shared_pro) HIP_TRY(c, launch_table_image(f, c->pro_nb, c->stream));
            HIP_TRY(c, launch_table(f, S, r.lds, c->stream));
            if (want_placement) HIP_TRY(c, launch_unpermute(c->d_place_step.p, c->d_inv_orders.p, c->d_scen.p, S, P, c->d_place.p, c->stream));
            return (int)SIMON_OK;
        })) return rc;
    return c->table_prof ? report_table_prof(c) : SIMON_OK;
}

static int run_fast_batch(simon_ctx* c, const BatchRoute& r, bool want_placement) {
    FastLaunch f{};
    fill_register_args(c, want_placement, f);
    f.pods = c->d_podsF.p;
    f.sc = FastScalars{(c->N + 63) / 64, c->Cn, c->Cp, c->P, c->S, c->g_cpu, c->g_mem, pod_rows(c), c->pod_W};
    return timed_launch(c, [&] { HIP_TRY(c, launch_fast(f, r.T, r.slots, c->has_mask, c->nzeq, r.lds, c->stream)); return (int)SIMON_OK; });
}

static int run_narrow_batch(simon_ctx* c, const BatchRoute& r, bool want_placement) {
    NarrowArgs a{};
    fill_register_args(c, want_placement, a);
    a.pods = c->d_podsN.p;
    a.mask_words = (c->N + 63) / 64; a.Cn = c->Cn; a.Cp = c->Cp; a.P = c->P; a.S = c->S;
    a.g_cpu = c->g_cpu; a.g_mem = c->g_mem;
    a.pod_present = pod_rows(c); a.pp_words = c->pod_W;
    return timed_launch(c, [&] { HIP_TRY(c, launch_narrow(a, r.T, r.slots, c->has_mask, c->rcp_div, r.lds, c->stream)); return (int)SIMON_OK; });
}

int simon_run_loaded(simon_ctx* c, int32_t want_placement) {
    if (!c) return SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "run_loaded: no scenarios loaded");
    if (c->evict_short >= 0 && !c->sub_on)   // (the prefix rule of simon_load_scenarios, deferred for flagged pods)
        return fail(c, SIMON_ESTATE, "run_loaded: pod %d, flagged for eviction, is preset to node %d which a scenario of this prefix batch lacks; set the batch's node rows (simon_set_scenario_nodes)", c->evict_short, c->p_preset[c->evict_short]);
    HIP_TRY(c, hipSetDevice(c->device));
    const int S = c->S, P = c->P;
    // bit 1: also record the devices Reserve books for every placed GPU pod (only problems with GPU requests have any)
    const bool want_slices = (want_placement & SIMON_WANT_GPU_SLICES) != 0 && c->has_gpu;
    const bool want_risk = !c->p_priority.empty();               // pods of unequal priority: the flags come from the placement matrix
    // (a pod-subset batch stores it too: simon_fetch_group_counts reads it)
    const bool want_place = (want_placement & SIMON_WANT_PLACEMENT) != 0 || want_risk || c->pods_on;
    c->have_slices = false; c->have_risk = false;
    if (want_slices) {
        HIP_TRY(c, c->d_gpu_slices.ensure((size_t)S * P));
        HIP_TRY(c, hipMemsetAsync(c->d_gpu_slices.p, 0, (size_t)S * P * 8, c->stream));
    }
    if (want_place) HIP_TRY(c, c->d_place.ensure((size_t)S * P));
    const BatchRoute r = route_batch(c);
    // the all-feature kernel takes prefix scenarios, and -- the context's opt-in, simon_set_own_nodes_all_feature -- own-nodes batches
    // whose rank rows are staged
    if (r.kernel == SIMON_KERNEL_WIDE && own_nodes(c) && !(c->own_wide && c->has_ranks)) {
        trace_segmented(c, "all-feature kernel -- refused");
        return fail(c, SIMON_ESTATE, "run_loaded: %s batch on a problem the score-table kernel does not take; run each scenario's own problem", own_kind(c));
    }
    if (r.kernel == SIMON_KERNEL_WIDE && own_nodes(c)) trace_segmented(c, "all-feature kernel, own-nodes run form");
    int rc;
    switch (r.kernel) {
        case SIMON_KERNEL_WIDE: rc = run_wide_batch(c, r, want_place, want_slices); break;
        case SIMON_KERNEL_NARROW_CACHE: rc = run_table_batch(c, r, want_place, want_slices); break;
        case SIMON_KERNEL_NARROW_FAST: rc = run_fast_batch(c, r, want_place); break;
        default: rc = run_narrow_batch(c, r, want_place);
    }
    if (rc) return rc;
    if (want_risk) {                                             // (behind ev1: not part of kernel_ms; one wave per scenario, P / 64 steps)
        if (!c->prio_staged) {
            HIP_TRY(c, c->d_prio.ensure((size_t)P));
            HIP_TRY(c, hipMemcpyAsync(c->d_prio.p, c->p_priority.data(), (size_t)P * 4, hipMemcpyHostToDevice, c->stream));
            c->prio_staged = true;
        }
        HIP_TRY(c, c->d_risk.ensure((size_t)S));
        hipLaunchKernelGGL(preempt_risk_kernel_impl, dim3(S), dim3(64), 0, c->stream, c->d_place.p, c->d_orders.p, c->d_scen.p, c->d_prio.p, P,
                           c->init_min_priority, c->d_risk.p);
        HIP_TRY(c, hipGetLastError());
        c->have_risk = true;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.kernel_ms = ms;
    c->stats.n_launches = 1;
    c->stats.kernel_variant = r.kernel;
    c->stats.kernel_generation = r.generation;
    c->stats.workgroup_size = r.T;
    c->stats.slots_per_lane = r.slots;
    c->stats.lds_bytes = (int64_t)r.lds;
    c->have_results = true;
    c->have_placement = want_place;
    c->have_slices = want_slices;
    return SIMON_OK;
}

int simon_fetch_results(simon_ctx* c, simon_batch_out* caller_out) {
    if (!c || !caller_out) return SIMON_EINVAL;
    simon_batch_out view, *out = &view;
    if (!batch_out_view(caller_out, out)) return fail(c, SIMON_EINVAL, "simon_batch_out size mismatch");
    if (!c->have_results) return fail(c, SIMON_ESTATE, "fetch_results: nothing has run");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t S = c->S, P = c->P;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if (out->unscheduled) HIP_TRY(c, hipMemcpyAsync(out->unscheduled, c->d_unsched.p, S * 4, hipMemcpyDeviceToHost, c->stream));
    if (out->used_cpu) HIP_TRY(c, hipMemcpyAsync(out->used_cpu, c->d_used_cpu.p, S * 8, hipMemcpyDeviceToHost, c->stream));
    if (out->used_mem) HIP_TRY(c, hipMemcpyAsync(out->used_mem, c->d_used_mem.p, S * 8, hipMemcpyDeviceToHost, c->stream));
    if (out->used_vg) {   // only the all-feature kernel tracks Open-Local volume groups
        if (c->stats.kernel_variant == SIMON_KERNEL_WIDE) HIP_TRY(c, hipMemcpyAsync(out->used_vg, c->d_used_vg.p, S * 8, hipMemcpyDeviceToHost, c->stream));
        else memset(out->used_vg, 0, S * 8);
    }
    if (out->placement) {
        if (!c->have_placement) return fail(c, SIMON_ESTATE, "fetch_results: the last run skipped placements");
        HIP_TRY(c, hipMemcpyAsync(out->placement, c->d_place.p, S * P * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (out->gpu_slices) {
        if (c->have_slices) HIP_TRY(c, hipMemcpyAsync(out->gpu_slices, c->d_gpu_slices.p, S * P * 8, hipMemcpyDeviceToHost, c->stream));
        else if (!c->has_gpu) memset(out->gpu_slices, 0, S * P * 8);      // no GPU request anywhere: nothing was ever booked
        else return fail(c, SIMON_ESTATE, "fetch_results: the last run did not record GPU devices (SIMON_WANT_GPU_SLICES)");
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.d2h_ms = ms;
    return SIMON_OK;
}

int simon_fetch_placement(simon_ctx* c, int32_t scenario, int32_t* placement) {
    if (!c || !placement) return SIMON_EINVAL;
    if (!c->have_results || !c->have_placement) return fail(c, SIMON_ESTATE, "fetch_placement: no placements on device");
    if (scenario < 0 || scenario >= c->S) return fail(c, SIMON_EINVAL, "fetch_placement: scenario out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(placement, c->d_place.p + (size_t)scenario * c->P, (size_t)c->P * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

int simon_fetch_gpu_slices(simon_ctx* c, int32_t scenario, uint64_t* slices) {
    if (!c || !slices) return SIMON_EINVAL;
    if (!c->have_results) return fail(c, SIMON_ESTATE, "fetch_gpu_slices: nothing has run");
    if (scenario < 0 || scenario >= c->S) return fail(c, SIMON_EINVAL, "fetch_gpu_slices: scenario out of range");
    if (!c->has_gpu) { memset(slices, 0, (size_t)c->P * 8); return SIMON_OK; }
    if (!c->have_slices) return fail(c, SIMON_ESTATE, "fetch_gpu_slices: the last run did not record GPU devices (SIMON_WANT_GPU_SLICES)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(slices, c->d_gpu_slices.p + (size_t)scenario * c->P, (size_t)c->P * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

int simon_fetch_preempt_risk(simon_ctx* c, uint8_t* risk) {
    if (!c || !risk) return SIMON_EINVAL;
    if (!c->have_results) return fail(c, SIMON_ESTATE, "fetch_preempt_risk: nothing has run");
    if (!c->have_risk) { memset(risk, 0, (size_t)c->S); return SIMON_OK; }       // one priority for all: DefaultPreemption finds no victim anywhere
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(risk, c->d_risk.p, (size_t)c->S, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SIMON_OK;
}

int simon_run_batch(simon_ctx* c, const simon_scenario* scen, int32_t S, const int32_t* orders, int32_t n_orders,
                    simon_batch_out* out) {
    if (!c || !out) return SIMON_EINVAL;
    simon_batch_out view;
    if (!batch_out_view(out, &view)) return fail(c, SIMON_EINVAL, "simon_batch_out size mismatch");
    int rc = simon_load_scenarios(c, scen, S, orders, n_orders);
    if (rc) return rc;
    rc = simon_run_loaded(c, (view.placement ? SIMON_WANT_PLACEMENT : 0) | (view.gpu_slices ? SIMON_WANT_GPU_SLICES : 0));
    if (rc) return rc;
    return simon_fetch_results(c, &view);
}

int simon_min_plan(simon_ctx* c, int32_t max_cpu_pct, int32_t max_mem_pct, simon_plan* best) {
    return simon_min_plan_vg(c, max_cpu_pct, max_mem_pct, 100, best, nullptr);
}

// satisfyResourceSetting + minimum over the batch on the device: leaves the key (n_nodes << 32 | scenario, ~0 = none) in c->d_plan[0]
// and, behind it, the winner's used cpu / memory / VG sums (plan_record_kernel)
static int launch_plan(simon_ctx* c, int32_t max_cpu_pct, int32_t max_mem_pct, int32_t max_vg_pct) {
    if (max_vg_pct > 100 || max_vg_pct < 0) max_vg_pct = 100;
    if (!c->have_results) return fail(c, SIMON_ESTATE, "min_plan: nothing has run");
    HIP_TRY(c, hipSetDevice(c->device));
    if (max_cpu_pct > 100 || max_cpu_pct < 0) max_cpu_pct = 100;  // apply.go:698-700
    if (max_mem_pct > 100 || max_mem_pct < 0) max_mem_pct = 100;
    HIP_TRY(c, hipMemsetAsync(c->d_plan.p, 0xFF, sizeof(unsigned long long), c->stream));
    const int blocks = std::min(64, (c->S + 255) / 256);
    hipLaunchKernelGGL(plan_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_scen.p, c->S, c->d_unsched.p,
                       c->d_used_cpu.p, c->d_used_mem.p, c->d_prefix_cpu.p, c->d_prefix_mem.p, max_cpu_pct, max_mem_pct,
                       c->has_local ? c->d_used_vg.p : nullptr, c->d_prefix_vg.p, max_vg_pct, own_nodes(c) ? c->d_seg_tot.p : nullptr, c->d_plan.p);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(plan_record_kernel, dim3(1), dim3(1), 0, c->stream, c->d_used_cpu.p, c->d_used_mem.p,
                       c->has_local ? c->d_used_vg.p : nullptr, c->d_plan.p);
    HIP_TRY(c, hipGetLastError());
    return SIMON_OK;
}

int simon_min_plan_device(simon_ctx* c, int32_t max_cpu_pct, int32_t max_mem_pct, int32_t max_vg_pct, void** d_key, void** stream) {
    if (!c || !d_key) return SIMON_EINVAL;
    const int rc = launch_plan(c, max_cpu_pct, max_mem_pct, max_vg_pct);
    if (rc) return rc;
    *d_key = c->d_plan.p;                                          // ordered behind plan_kernel on `stream`: a collective enqueued there needs no host sync
    if (stream) *stream = (void*)c->stream;
    return SIMON_OK;
}

int simon_min_plan_vg(simon_ctx* c, int32_t max_cpu_pct, int32_t max_mem_pct, int32_t max_vg_pct, simon_plan* best,
                      int32_t* vg_pct) {
    if (!c || !best) return SIMON_EINVAL;
    if (vg_pct) *vg_pct = 0;
    const int rcl = launch_plan(c, max_cpu_pct, max_mem_pct, max_vg_pct);
    if (rcl) return rcl;
    unsigned long long rec[kPlanRecWords] = {0, 0, 0, 0};          // one read-back per plan: key and the winner's sums
    HIP_TRY(c, hipMemcpyAsync(rec, c->d_plan.p, sizeof rec, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long key = rec[0];
    memset(best, 0, sizeof *best);
    best->scenario = -1;
    if (key == ~0ull) return SIMON_OK;
    const int s = (int)(key & 0xFFFFFFFFu);
    const int64_t uc = (int64_t)rec[1], um = (int64_t)rec[2];
    const int n = c->scen[s].n_nodes;
    int64_t ac = 0, am = 0;
    if (own_nodes(c)) {
        for (int j = 0; j < c->N; ++j)
            if (node_in(c, s, j)) { ac += c->alloc_cpu[j]; am += c->alloc_mem[j]; }
    } else {                                                       // a prefix scenario: the first n nodes
        ac = c->prefix_cpu[n]; am = c->prefix_mem[n];
    }
    best->found = 1; best->scenario = s; best->n_nodes = n; best->order_id = c->scen[s].order_id;
    best->cpu_pct = (int)((double)uc / (double)ac * 100.0);
    best->mem_pct = (int)((double)(um * 1000) / (double)(am * 1000) * 100.0);
    best->used_cpu = uc; best->used_mem = um;
    const int64_t av = own_nodes(c) ? c->seg_tot[(size_t)2 * c->S + s] : c->prefix_vg[n];
    if (vg_pct && c->has_local && av != 0) *vg_pct = (int)((double)(int64_t)rec[3] / (double)av * 100.0);
    return SIMON_OK;
}

// One scenario replayed for simon_explain (order: the caller's, uploaded) and simon_explain_loaded (order == null: the scenario's row
// of the loaded orders, and with per-scenario node ranks its own rank row, so that the replay breaks ties exactly like the batch did).
static int explain_impl(simon_ctx* c, int n_nodes, const int32_t* order, int32_t scenario, int32_t* failed_pods, uint16_t* fail_codes,
                        int32_t max_failed) {
    if (int rc = stage(c)) return rc;
    if (own_nodes(c)) return fail(c, SIMON_ESTATE, "explain: %s batch loaded", own_kind(c));
    if (n_nodes < 0 || n_nodes > c->N) return fail(c, SIMON_EINVAL, "explain: n_nodes out of range");
    for (int i = 0; order && i < c->P; ++i) if (order[i] < 0 || order[i] >= c->P) return fail(c, SIMON_EINVAL, "explain: bad order");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_wide_staged(c)) return rc;   // (NARROW problem: the failure codes still come from the all-feature kernel)
    // not wide_workgroup's rule, on purpose: a single replay is one workgroup, and its thresholds are what existing replays run with
    int T = c->force_T ? c->force_T : (n_nodes <= 512 ? 256 : n_nodes <= 4096 ? 512 : 1024);
    if (T == 128) T = 256;
    const WideScenario hs{n_nodes, order ? 0 : c->scen[scenario].order_id};
    const int32_t slot0 = 0;
    int32_t nf = 0;
    std::vector<int64_t> detail;                                   // (the context's own are set once the replay has succeeded)
    WideReplay job;
    job.scen = &hs; job.S = 1; job.max_n = n_nodes;
    job.d_orders = order ? nullptr : c->d_orders.p; job.h_order = order;
    if (!order && c->has_ranks) { job.rank_row = &scenario; job.d_node_rank = c->d_node_rank.p; job.d_node_inv = c->d_node_inv.p; }
    if (!order && c->pods_on) { job.d_pod_present = c->d_pod_words.p; job.pod_row = &scenario; job.pp_words = c->pod_W; }
    if (c->img_R > 0) {                  // ImageLocality of THIS size, whether or not the batch has it
        std::vector<unsigned char>& one = c->h_img_explain;
        one.assign((size_t)c->img_R * c->Cn, 0);
        img_slot_scores(c, n_nodes, one.data());
        HIP_TRY(c, c->d_img_explain.upload(one, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        job.d_img = c->d_img_explain.p; job.img_slot = &slot0;
    }
    job.max_failed = max_failed; job.n_failed = &nf; job.failed_pods = failed_pods; job.recorded_only = true;
    job.fail_codes = fail_codes; job.code_stride = n_nodes;       // (no bins: the host folds the rows)
    job.detail = &detail;
    if (int rc = wide_replay(c->wide, *c, job, T, c->stream, c->err)) return rc;
    c->explain_detail.swap(detail);
    c->explain_nodes = n_nodes;
    c->explain_ran = true;
    return nf;
}

int simon_explain(simon_ctx* c, simon_scenario scen, const int32_t* order, int32_t* failed_pods, uint16_t* fail_codes,
                  int32_t max_failed) {
    if (!c || !order || !failed_pods || !fail_codes || max_failed <= 0) return c ? fail(c, SIMON_EINVAL, "explain: bad arguments") : SIMON_EINVAL;
    if (c->sub_on) return fail(c, SIMON_ESTATE, "explain: node-subset batch loaded; explain the scenario's own problem (its nodes alone)");
    if (c->pods_on)     // ... and no pod row
        return fail(c, SIMON_ESTATE, "explain: per-scenario pod rows are loaded; use simon_explain_loaded(scenario index)");
    if (c->has_ranks)   // an ad-hoc scenario has no rank row: which loaded scenario's tie-break order would apply is ambiguous
        return fail(c, SIMON_ESTATE, "explain: per-scenario node ranks are loaded; use simon_explain_loaded(scenario index)");
    return explain_impl(c, scen.n_nodes, order, -1, failed_pods, fail_codes, max_failed);
}

int simon_explain_loaded(simon_ctx* c, int32_t scenario, int32_t* failed_pods, uint16_t* fail_codes, int32_t max_failed) {
    if (!c || !failed_pods || !fail_codes || max_failed <= 0) return c ? fail(c, SIMON_EINVAL, "explain_loaded: bad arguments") : SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "explain_loaded: no scenarios loaded");
    if (scenario < 0 || scenario >= c->S) return fail(c, SIMON_EINVAL, "explain_loaded: scenario %d outside [0,%d)", scenario, c->S);
    if (own_nodes(c))    // the replay runs on the all-feature kernel, which takes prefix scenarios only
        return fail(c, SIMON_ESTATE, "explain_loaded: %s batch; explain the scenario's own problem (its nodes alone)", own_kind(c));
    if (c->evict_short >= 0) return fail(c, SIMON_ESTATE, "explain_loaded: pod %d, flagged for eviction, lacks its node in this prefix batch", c->evict_short);
    return explain_impl(c, c->scen[scenario].n_nodes, nullptr, scenario, failed_pods, fail_codes, max_failed);
}

int simon_explain_batch(simon_ctx* c, const int32_t* scenarios, int32_t n_scen, int32_t max_failed, int32_t max_bins, int32_t* n_failed,
                        int32_t* failed_pods, int32_t* n_bins, simon_fail_bin* bins, uint16_t* fail_codes, int32_t code_stride) {
    if (!c) return SIMON_EINVAL;
    if (!scenarios || n_scen <= 0 || max_failed <= 0 || max_bins < 1 || max_bins > SIMON_EXPLAIN_BINS || !n_failed || !failed_pods || !n_bins || !bins)
        return fail(c, SIMON_EINVAL, "explain_batch: bad arguments");
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "explain_batch: no scenarios loaded");
    if (own_nodes(c))    // the replay runs on the all-feature kernel, which takes prefix scenarios only
        return fail(c, SIMON_ESTATE, "explain_batch: %s batch; explain each scenario's own problem (its nodes alone)", own_kind(c));
    if (c->evict_short >= 0) return fail(c, SIMON_ESTATE, "explain_batch: pod %d, flagged for eviction, lacks its node in this prefix batch", c->evict_short);
    const bool image = c->img_R > 0 && !c->img_sizes.empty();
    std::vector<WideScenario> hs((size_t)n_scen);
    std::vector<int32_t> slots(image ? (size_t)n_scen : 0);
    int max_n = 0;
    for (int k = 0; k < n_scen; ++k) {
        if (scenarios[k] < 0 || scenarios[k] >= c->S) return fail(c, SIMON_EINVAL, "explain_batch: scenario %d outside [0,%d)", scenarios[k], c->S);
        hs[k] = WideScenario{c->scen[scenarios[k]].n_nodes, c->scen[scenarios[k]].order_id};
        if (image) slots[k] = c->h_img_slot[scenarios[k]];
        max_n = std::max(max_n, hs[k].n_nodes);
    }
    if (fail_codes && code_stride < std::max(max_n, 1)) return fail(c, SIMON_EINVAL, "explain_batch: code_stride %d below the largest listed n_nodes %d", code_stride, max_n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_wide_staged(c)) return rc;   // (the batch ran on another kernel: the failure codes still come from the all-feature kernel)
    WideReplay job;
    job.scen = hs.data(); job.S = n_scen; job.max_n = max_n; job.d_orders = c->d_orders.p;
    if (c->has_ranks) { job.rank_row = scenarios; job.d_node_rank = c->d_node_rank.p; job.d_node_inv = c->d_node_inv.p; }
    if (image) { job.d_img = c->wide.img; job.img_slot = slots.data(); }
    if (c->pods_on) { job.d_pod_present = c->d_pod_words.p; job.pod_row = scenarios; job.pp_words = c->pod_W; }
    job.max_failed = max_failed; job.n_failed = n_failed; job.failed_pods = failed_pods;
    job.max_bins = max_bins; job.n_bins = n_bins; job.bins = bins;
    job.fail_codes = fail_codes; job.code_stride = code_stride;
    return wide_replay(c->wide, *c, job, wide_workgroup(c, n_scen, max_n), c->stream, c->err);
}

// simon_explain_batch for segmented and node-subset batches: the replay in its own-nodes mode (simon_wide.h: kArgOwn), where a scenario
// holds the pool nodes that its rank row -- the batch's own or the caller's -- ranks below N.  Everything the launch sizes by a node count is
// sized by the pool; code rows are indexed by pool node.  The route decision is simon_run_loaded's: what that refuses, this refuses.
int simon_explain_own_batch(simon_ctx* c, const int32_t* scenarios, int32_t n_scen, int32_t max_failed, int32_t max_bins, int32_t* n_failed,
                            int32_t* failed_pods, int32_t* n_bins, simon_fail_bin* bins, uint16_t* fail_codes, int32_t code_stride) {
    if (!c) return SIMON_EINVAL;
    if (!scenarios || n_scen <= 0 || max_failed <= 0 || max_bins < 1 || max_bins > SIMON_EXPLAIN_BINS || !n_failed || !failed_pods || !n_bins || !bins)
        return fail(c, SIMON_EINVAL, "explain_own_batch: bad arguments");
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "explain_own_batch: no scenarios loaded");
    if (!own_nodes(c)) return fail(c, SIMON_ESTATE, "explain_own_batch: prefix batch; use simon_explain_batch");
    // (the batch simon_run_loaded refuses: its pods' gates and presets were never checked against a run.  With the opt-in a wide-routed batch
    // runs, and replays, unless the problem has Open-Local storage: the replay's own-nodes form is the full variant's)
    if (!c->has_ranks || (route_batch(c).kernel == SIMON_KERNEL_WIDE && !(c->own_wide && !c->has_local)))
        return fail(c, SIMON_ESTATE, "explain_own_batch: %s batch on a problem the score-table kernel does not take; explain each scenario's own problem", own_kind(c));
    const int N = c->N;
    std::vector<WideScenario> hs((size_t)n_scen);
    for (int k = 0; k < n_scen; ++k) {
        if (scenarios[k] < 0 || scenarios[k] >= c->S) return fail(c, SIMON_EINVAL, "explain_own_batch: scenario %d outside [0,%d)", scenarios[k], c->S);
        hs[k] = WideScenario{c->scen[scenarios[k]].n_nodes, c->scen[scenarios[k]].order_id};
    }
    if (fail_codes && code_stride < N) return fail(c, SIMON_EINVAL, "explain_own_batch: code_stride %d below the pool's %d nodes (rows are indexed by pool node)", code_stride, N);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_wide_staged(c)) return rc;   // (the batch runs on the score-table kernel: the failure codes come from the all-feature kernel)
    WideReplay job;
    job.scen = hs.data(); job.S = n_scen; job.max_n = N; job.d_orders = c->d_orders.p; job.own = true;
    job.rank_row = scenarios; job.d_node_rank = c->d_node_rank.p; job.d_node_inv = c->d_node_inv.p;
    std::vector<int32_t> slots;                                  // the batch's image states and each listed scenario's slot
    if (c->img_R > 0 && c->img_own_T > 0) {
        for (int k = 0; k < n_scen; ++k) slots.push_back(c->h_img_slot[scenarios[k]]);
        job.d_img = c->wide.img; job.img_slot = slots.data();
    }
    if (c->pods_on) { job.d_pod_present = c->d_pod_words.p; job.pod_row = scenarios; job.pp_words = c->pod_W; }
    job.max_failed = max_failed; job.n_failed = n_failed; job.failed_pods = failed_pods;
    job.max_bins = max_bins; job.n_bins = n_bins; job.bins = bins;
    job.fail_codes = fail_codes; job.code_stride = code_stride;
    return wide_replay(c->wide, *c, job, wide_workgroup(c, n_scen, N), c->stream, c->err);
}

int simon_fetch_image_scores(simon_ctx* c, int32_t scenario, uint8_t* score) {
    if (!c || !score) return c ? fail(c, SIMON_EINVAL, "fetch_image_scores: bad arguments") : SIMON_EINVAL;
    if (!c->staged || c->S <= 0) return fail(c, SIMON_ESTATE, "fetch_image_scores: no scenarios loaded");
    if (c->img_R == 0) return fail(c, SIMON_ESTATE, "fetch_image_scores: the problem has no image that a pod runs and a node lists");
    if (scenario < 0 || scenario >= c->S) return fail(c, SIMON_EINVAL, "fetch_image_scores: scenario %d outside [0,%d)", scenario, c->S);
    HIP_TRY(c, hipSetDevice(c->device));
    const int N = c->N, Cp = c->Cp, slot = c->h_img_slot[scenario];
    std::fill(score, score + (size_t)Cp * N, (uint8_t)0);
    std::vector<unsigned char> tab;
    if (c->variant == SIMON_KERNEL_NARROW && c->t_img_staged) {      // the score-table kernel's [slot][table class][internal node class]
        const int Ct = c->Cn_t;
        tab.resize((size_t)c->img_stride_t);
        HIP_TRY(c, hipMemcpyAsync(tab.data(), c->d_t_img.p + (size_t)slot * c->img_stride_t, tab.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int cp = 0; cp < Cp; ++cp)
            for (int j = 0; j < N; ++j)
                if (node_in(c, scenario, j)) score[(size_t)cp * N + j] = tab[(size_t)c->h_tc_of[cp] * Ct + c->h_ncls_t[j]];
        return SIMON_OK;
    }
    if (int rc = ensure_wide_staged(c)) return rc;                    // ... or the all-feature kernel's [slot][row][node class]
    tab.resize((size_t)c->img_R * c->Cn);
    HIP_TRY(c, hipMemcpyAsync(tab.data(), c->wide.img + (size_t)slot * tab.size(), tab.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int cp = 0; cp < Cp; ++cp)
        for (int j = 0; c->img_row_of[cp] >= 0 && j < N; ++j)
            if (node_in(c, scenario, j)) score[(size_t)cp * N + j] = tab[(size_t)c->img_row_of[cp] * c->Cn + c->node_class[j]];
    return SIMON_OK;
}

int simon_get_stats(simon_ctx* c, simon_stats* st) {
    if (!c || !st) return SIMON_EINVAL;
    *st = c->stats;
    return SIMON_OK;
}

int simon_explain_local_detail(simon_ctx* c, int64_t* detail, int32_t max_failed) {
    if (!c || !detail || max_failed <= 0) return c ? fail(c, SIMON_EINVAL, "explain_local_detail: bad arguments") : SIMON_EINVAL;
    if (!c->explain_ran) return fail(c, SIMON_ESTATE, "explain_local_detail: no simon_explain call yet");
    const size_t row = (size_t)std::max(c->explain_nodes, 0) * 4;
    const size_t rows = row ? std::min<size_t>(c->explain_detail.size() / row, (size_t)max_failed) : 0;
    if (rows) std::memcpy(detail, c->explain_detail.data(), rows * row * sizeof(int64_t));
    return (int)rows;
}

int simon_device_results(simon_ctx* c, void** d_unscheduled, void** d_used_cpu, void** d_used_mem) {
    if (!c) return SIMON_EINVAL;
    if (!c->have_results) return fail(c, SIMON_ESTATE, "device_results: nothing has run");
    if (d_unscheduled) *d_unscheduled = c->d_unsched.p;
    if (d_used_cpu) *d_used_cpu = c->d_used_cpu.p;
    if (d_used_mem) *d_used_mem = c->d_used_mem.p;
    return SIMON_OK;
}

}  // extern "C"

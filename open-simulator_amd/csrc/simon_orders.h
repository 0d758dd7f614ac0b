// simon_orders.h -- order rows composed from segments (simon_load_scenarios_composed): every order is the concatenation of one variant
// per segment, so n_orders x P ids are described by a table of sum_g n_variants[g] x len_g ids and n_orders x G choices.  The first
// half is plain C++ without a HIP dependency -- the validation of the caller's table and the host twin of the kernels
// (SIMON_ORDER_STAGE=host) --, so that a stand-alone program can run it under a sanitizer; the launchers follow under __HIPCC__.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace simon {

constexpr int kMaxOrderSegments = 64;        // SIMON_MAX_ORDER_SEGMENTS
constexpr int kMaxOrderVariants = 1 << 24;   // SIMON_MAX_ORDER_VARIANTS: variants of all segments together

// the caller's table (simon_order_segments without struct_size)
struct OrderSegView {
    int32_t n_seg;
    const int32_t *seg_start, *n_variants, *variant_pods, *variant_live, *choice;
};

// why a table is refused; the order is the order of the checks
enum OrderSegError {
    kSegOk = 0,
    kSegCount,        // G outside [1, kMaxOrderSegments]
    kSegNull,         // a required array is missing
    kSegStarts,       // seg_start does not run from 0 to P, non-decreasing
    kSegVariants,     // n_variants[g] < 1, or more than kMaxOrderVariants variants in all
    kSegPodId,        // a variant entry is no pod id
    kSegOverlap,      // a pod id twice in a segment's first row, or in the first rows of two segments
    kSegNotPerm,      // a later variant row is not a permutation of its segment's first row
    kSegLive,         // variant_live outside [0, len_g]
    kSegChoice,       // choice outside [0, n_variants[g])
};

// What validation leaves behind for the device (and the host twin): where a segment's rows start, which segment owns a pod, and the
// inverse of every variant row -- pos[var_off[g] + v * len_g + local[p]] = position of pod p inside variant v of its segment g, with
// local[p] = its position in variant 0.  With it the inverse orders and the presence bits are computed BY POD ID, in coalesced writes.
struct OrderSegTable {
    int G = 0, P = 0;
    std::vector<int32_t> seg_start;          // [G + 1]
    std::vector<int64_t> var_off;            // [G] offset of segment g's rows in variant_pods / pos
    std::vector<int32_t> live_off;           // [G + 1] offset of segment g's variants in variant_live
    std::vector<int32_t> owner, local;       // [P]
    std::vector<int32_t> pos;                // like variant_pods
    size_t n_ids() const { return pos.size(); }
    int n_var() const { return live_off.empty() ? 0 : live_off[G]; }
};

// Validates the table for P pods and n_orders orders in sum_g n_variants[g] x len_g + n_orders x G steps and fills `t`.  *at receives
// the index of the offending entry in its array (segment, variant entry, live entry or choice entry).
inline OrderSegError order_segments_check(const OrderSegView& v, int P, int n_orders, OrderSegTable& t, long long* at) {
    long long dummy;
    long long& where = at ? *at : dummy;
    where = 0;
    const int G = v.n_seg;
    if (G < 1 || G > kMaxOrderSegments) return kSegCount;
    if (!v.seg_start || !v.n_variants || !v.choice || (P > 0 && !v.variant_pods)) return kSegNull;
    if (v.seg_start[0] != 0) return kSegStarts;
    for (int g = 0; g < G; ++g)
        if (v.seg_start[g + 1] < v.seg_start[g]) { where = g + 1; return kSegStarts; }
    if (v.seg_start[G] != P) { where = G; return kSegStarts; }
    // (the sum is bounded before anything is sized from it: live_off is an int32 running sum)
    long long n_var = 0;
    for (int g = 0; g < G; ++g) {
        if (v.n_variants[g] < 1) { where = g; return kSegVariants; }
        if ((n_var += v.n_variants[g]) > kMaxOrderVariants) { where = g; return kSegVariants; }
    }
    t.G = G; t.P = P;
    t.seg_start.assign(v.seg_start, v.seg_start + G + 1);
    t.var_off.assign(G, 0);
    t.live_off.assign(G + 1, 0);
    size_t ids = 0;
    for (int g = 0; g < G; ++g) {
        t.var_off[g] = (int64_t)ids;
        t.live_off[g + 1] = t.live_off[g] + v.n_variants[g];
        ids += (size_t)v.n_variants[g] * (size_t)(v.seg_start[g + 1] - v.seg_start[g]);
    }
    t.owner.assign(P, -1);
    t.local.assign(P, 0);
    t.pos.assign(ids, 0);
    std::vector<int32_t> seen(P, -1);                                 // the last row (by variant index over all segments) that held the pod
    for (int g = 0; g < G; ++g) {
        const int len = v.seg_start[g + 1] - v.seg_start[g];
        for (int w = 0; w < v.n_variants[g]; ++w) {
            const size_t row = (size_t)t.var_off[g] + (size_t)w * len;
            const int32_t stamp = t.live_off[g] + w;
            for (int k = 0; k < len; ++k) {
                const int32_t p = v.variant_pods[row + k];
                where = (long long)(row + k);
                if (p < 0 || p >= P) return kSegPodId;
                if (w == 0) {
                    if (t.owner[p] >= 0) return kSegOverlap;
                    t.owner[p] = g; t.local[p] = k;
                } else if (t.owner[p] != g || seen[p] == stamp) return kSegNotPerm;
                seen[p] = stamp;
                t.pos[row + t.local[p]] = k;
            }
        }
    }
    // (the first rows are disjoint and hold P ids in all: together they are [0, P))
    if (v.variant_live)
        for (int g = 0; g < G; ++g)
            for (int w = 0; w < v.n_variants[g]; ++w) {
                const int32_t l = v.variant_live[t.live_off[g] + w];
                if (l < 0 || l > v.seg_start[g + 1] - v.seg_start[g]) { where = t.live_off[g] + w; return kSegLive; }
            }
    for (long long i = 0; i < (long long)n_orders * G; ++i)
        if (v.choice[i] < 0 || v.choice[i] >= v.n_variants[i % G]) { where = i; return kSegChoice; }
    where = 0;
    return kSegOk;
}

inline const char* order_segments_text(OrderSegError e) {
    switch (e) {
        case kSegOk: return "ok";
        case kSegCount: return "n_seg outside [1, SIMON_MAX_ORDER_SEGMENTS]";
        case kSegNull: return "a required array is NULL";
        case kSegStarts: return "seg_start does not run from 0 to P in ascending order";
        case kSegVariants: return "a segment has no variant, or the segments have more than SIMON_MAX_ORDER_VARIANTS together";
        case kSegPodId: return "a variant entry is not a pod id";
        case kSegOverlap: return "segments overlap (a pod id twice among the first rows)";
        case kSegNotPerm: return "a variant row is not a permutation of its segment's pods";
        case kSegLive: return "a live value outside [0, len]";
        case kSegChoice: return "a choice outside [0, n_variants)";
    }
    return "?";
}

// The host twin of the kernels: orders [n_orders][P]; inv [n_orders][P] (or null); words [n_orders][(P + 31) / 32] by pod id (or null,
// and only with `live`).
inline void order_segments_compose_host(const OrderSegTable& t, const int32_t* variant_pods, const int32_t* live, const int32_t* choice, int n_orders,
                                        int32_t* orders, int32_t* inv, uint32_t* words) {
    const int P = t.P, G = t.G, W = (P + 31) / 32;
    for (int o = 0; o < n_orders; ++o) {
        if (words) for (int w = 0; w < W; ++w) words[(size_t)o * W + w] = 0u;
        for (int g = 0; g < G; ++g) {
            const int start = t.seg_start[g], len = t.seg_start[g + 1] - start, v = choice[(size_t)o * G + g];
            const int32_t* row = variant_pods + t.var_off[g] + (size_t)v * len;
            const int n_live = live ? live[t.live_off[g] + v] : len;
            for (int k = 0; k < len; ++k) {
                const int32_t p = row[k];
                orders[(size_t)o * P + start + k] = p;
                if (inv) inv[(size_t)o * P + p] = start + k;
                if (words && k < n_live) words[(size_t)o * W + (p >> 5)] |= 1u << (p & 31);
            }
        }
    }
}

}  // namespace simon

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace simon {

// the table on the device
struct OrderCompose {
    const int32_t* seg_start;                // [G + 1]
    const int64_t* var_off;                  // [G]
    const int32_t* live_off;                 // [G + 1]
    const int32_t* variant_pods;             // the caller's rows
    const int32_t* pos;                      // OrderSegTable::pos
    const int32_t *owner, *local;            // [P]
    const int32_t* live;                     // [n_var] or nullptr = every row is live throughout
    const int32_t* choice;                   // [n_orders][G]
    int32_t G, P, n_orders;
};

// order_compose_kernel: orders[o][i] over (order o, stream position i)
hipError_t launch_order_compose(const OrderCompose& a, int32_t* orders, hipStream_t st);
// order_by_pod_kernel: over (order o, pod id p), 64 ids per wave -- inv[o][p] (or nullptr) and the presence words [n_orders][(P + 31) / 32]
// of the live entries (or nullptr)
hipError_t launch_order_by_pod(const OrderCompose& a, int32_t* inv, uint32_t* words, hipStream_t st);
// row s of pod_words [S][W] = row scen[s].order_id of order_words (scen [S][2]: n_nodes, order_id)
hipError_t launch_order_rows_expand(const uint32_t* order_words, const int32_t* scen, int S, int W, uint32_t* pod_words, hipStream_t st);

}  // namespace simon
#endif

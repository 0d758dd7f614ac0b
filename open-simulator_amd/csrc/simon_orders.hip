// simon_orders.hip -- the order rows of simon_load_scenarios_composed, built on the device from the segment table (simon_orders.h): the
// host uploads sum_g n_variants[g] x len_g ids and n_orders x G choices instead of n_orders x P ids twice (orders and inverse orders)
// and S x P presence bits.  No atomics, no scattered writes: the orders are written by stream position, the inverse orders and the
// presence words by pod id through the inverse of every variant row (OrderSegTable::pos).  The arrays equal what the host loops of
// order_segments_compose_host build (SIMON_ORDER_STAGE=host).
#include "simon_orders.h"

namespace simon {

namespace {

constexpr int kOrderThreads = 256;

// the segment of stream position i: the g with seg_start[g] <= i < seg_start[g + 1] (empty segments are skipped by the search)
__device__ inline int segment_of(const int32_t* s_start, int G, int i) {
    int lo = 0, hi = G - 1;
    while (lo < hi) {                                    // the first g with seg_start[g + 1] > i
        const int mid = (lo + hi) >> 1;
        if (s_start[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kOrderThreads) void order_compose_kernel(OrderCompose a, int32_t* __restrict__ orders) {
    __shared__ int32_t s_start[kMaxOrderSegments + 1];
    for (int g = threadIdx.x; g <= a.G; g += kOrderThreads) s_start[g] = a.seg_start[g];
    __syncthreads();
    const int o = blockIdx.y, i = blockIdx.x * kOrderThreads + threadIdx.x;
    if (i >= a.P) return;
    const int g = segment_of(s_start, a.G, i);
    const int start = s_start[g], len = s_start[g + 1] - start;
    const int v = a.choice[(size_t)o * a.G + g];
    orders[(size_t)o * a.P + i] = a.variant_pods[a.var_off[g] + (int64_t)v * len + (i - start)];
}

__global__ __launch_bounds__(kOrderThreads) void order_by_pod_kernel(OrderCompose a, int32_t* __restrict__ inv, uint32_t* __restrict__ words) {
    const int o = blockIdx.y, p = blockIdx.x * kOrderThreads + threadIdx.x;
    const int W = (a.P + 31) >> 5;
    bool live = false;
    if (p < a.P) {
        const int g = a.owner[p];
        const int start = a.seg_start[g], len = a.seg_start[g + 1] - start;
        const int v = a.choice[(size_t)o * a.G + g];
        const int k = a.pos[a.var_off[g] + (int64_t)v * len + a.local[p]];     // position of pod p inside its segment's chosen variant
        if (inv) inv[(size_t)o * a.P + p] = start + k;
        live = !a.live || k < a.live[a.live_off[g] + v];
    }
    if (!words) return;                                  // (uniform: every lane of the wave reaches the ballot or none does)
    // 64 pod ids per wave: the ballot is two presence words; the lanes at or beyond P contribute 0, so the tail bits are 0
    const unsigned long long m = __ballot(live);
    const int lane = threadIdx.x & 63;
    const int w = (p - lane) >> 5;                       // the word of the wave's first id (a multiple of 64)
    if (lane == 0 && w < W) words[(size_t)o * W + w] = (uint32_t)m;
    if (lane == 32 && w + 1 < W) words[(size_t)o * W + w + 1] = (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(kOrderThreads) void order_rows_expand_kernel(const uint32_t* __restrict__ order_words, const int32_t* __restrict__ scen, int W,
                                                                          uint32_t* __restrict__ pod_words) {
    const int s = blockIdx.y, w = blockIdx.x * kOrderThreads + threadIdx.x;
    if (w < W) pod_words[(size_t)s * W + w] = order_words[(size_t)scen[2 * s + 1] * W + w];
}

}  // namespace

hipError_t launch_order_compose(const OrderCompose& a, int32_t* orders, hipStream_t st) {
    if (a.P <= 0 || a.n_orders <= 0) return hipSuccess;
    // (blockIdx.y carries the order: at most 65 535 per launch)
    for (int first = 0; first < a.n_orders; first += 65535) {
        OrderCompose b = a;
        b.choice = a.choice + (size_t)first * a.G;
        const int n = a.n_orders - first < 65535 ? a.n_orders - first : 65535;
        hipLaunchKernelGGL(order_compose_kernel, dim3((unsigned)((a.P + kOrderThreads - 1) / kOrderThreads), (unsigned)n), dim3(kOrderThreads), 0, st, b,
                           orders + (size_t)first * a.P);
    }
    return hipGetLastError();
}

hipError_t launch_order_by_pod(const OrderCompose& a, int32_t* inv, uint32_t* words, hipStream_t st) {
    if (a.P <= 0 || a.n_orders <= 0 || (!inv && !words)) return hipSuccess;
    const size_t W = (size_t)(a.P + 31) / 32;
    for (int first = 0; first < a.n_orders; first += 65535) {
        OrderCompose b = a;
        b.choice = a.choice + (size_t)first * a.G;
        const int n = a.n_orders - first < 65535 ? a.n_orders - first : 65535;
        hipLaunchKernelGGL(order_by_pod_kernel, dim3((unsigned)((a.P + kOrderThreads - 1) / kOrderThreads), (unsigned)n), dim3(kOrderThreads), 0, st, b,
                           inv ? inv + (size_t)first * a.P : nullptr, words ? words + (size_t)first * W : nullptr);
    }
    return hipGetLastError();
}

hipError_t launch_order_rows_expand(const uint32_t* order_words, const int32_t* scen, int S, int W, uint32_t* pod_words, hipStream_t st) {
    if (S <= 0 || W <= 0) return hipSuccess;
    for (int first = 0; first < S; first += 65535) {
        const int n = S - first < 65535 ? S - first : 65535;
        hipLaunchKernelGGL(order_rows_expand_kernel, dim3((unsigned)((W + kOrderThreads - 1) / kOrderThreads), (unsigned)n), dim3(kOrderThreads), 0, st,
                           order_words, scen + (size_t)2 * first, W, pod_words + (size_t)first * W);
    }
    return hipGetLastError();
}

}  // namespace simon

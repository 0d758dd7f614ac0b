// simon_subset.hip -- subset_stage_kernel: the per-scenario arrays of a node-subset batch (simon_set_scenario_nodes), built on the
// device from the presence words.  One wave per scenario; every order comes from ballots and prefix counts (no atomics), so the
// arrays are the same on every run and equal to what the host loops of simon_hip.hip build (SIMON_SUBSET_STAGE=host).
//
// The canonical order of a scenario is nodeTree.list() of its own nodes inserted in pool order (V/internal/cache/node_tree.go:119-143):
// zones in first-appearance order, one node per zone per round, exhausted zones skipped.  A present node with index i inside its zone
// (among the scenario's nodes) and zone order q comes after, of the zone of order q', min(cnt, i + 1) nodes for q' < q and min(cnt, i)
// nodes for q' >= q:   rank = sum_z min(cnt_z, i) + #{z' : order(z') < q, cnt_z' > i}.
#include "simon_subset.h"

namespace simon {
namespace {

__global__ __launch_bounds__(64) void subset_stage_kernel(SubsetStage a) {
    extern __shared__ int32_t smem[];
    int32_t* const s_ocnt = smem;            // [64] nodes of the zone with order q
    int32_t* const s_zord = smem + 64;       // [64] order of zone z
    int32_t* const s_fill = smem + 128;      // [Ct] nodes of class d met so far (pass 2)
    const int s = blockIdx.x, lane = threadIdx.x, N = a.N;
    const uint32_t* __restrict__ const row = a.present + (size_t)s * a.W;
    int32_t* const rank = a.rank + (size_t)s * N;
    int32_t* const inv = a.inv + (size_t)s * N;
    const unsigned long long below = (1ull << lane) - 1;

    // ---- pass 0, pool order: index of every present node inside its zone; lane z keeps zone z's count and first node; the totals ----
    int zcnt = 0, zfirst = N;
    long long t_cpu = 0, t_mem = 0, t_vg = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool in = j < N && ((row[j >> 5] >> (j & 31)) & 1u) != 0;
        const int z = (in && a.node_zone) ? a.node_zone[j] : 0;
        if (in) {
            t_cpu += a.prefix_cpu[j + 1] - a.prefix_cpu[j];
            t_mem += a.prefix_mem[j + 1] - a.prefix_mem[j];
            t_vg += a.prefix_vg[j + 1] - a.prefix_vg[j];
        }
        int idx = 0;
        unsigned long long left = __ballot(in);
        while (left) {                                                // one turn per distinct zone among the chunk's present nodes
            const int lead = __ffsll(left) - 1;
            const int zz = __shfl(z, lead, 64);
            const bool mine = in && z == zz;
            const unsigned long long m = __ballot(mine);
            const int before = __shfl(zcnt, zz, 64);
            if (mine) idx = before + __popcll(m & below);
            if (lane == zz) {
                zcnt = before + __popcll(m);
                if (before == 0) zfirst = base + lead;
            }
            left &= ~m;
        }
        if (j < N) rank[j] = in ? idx : N;                            // (the index inside the zone: pass 1 turns it into the rank)
    }
    // zone order = first appearance among the scenario's nodes (the first nodes of two zones differ, so no ties)
    int q = 0, nz = 0, n = 0;
    for (int k = 0; k < 64; ++k) {
        const int ck = __shfl(zcnt, k, 64), fk = __shfl(zfirst, k, 64);
        q += (ck > 0 && fk < zfirst) ? 1 : 0;
        nz += ck > 0 ? 1 : 0;
        n += ck;
    }
    if (zcnt > 0) s_ocnt[q] = zcnt;
    s_zord[lane] = q;
    for (int off = 32; off > 0; off >>= 1) {
        t_cpu += __shfl_xor(t_cpu, off, 64);
        t_mem += __shfl_xor(t_mem, off, 64);
        t_vg += __shfl_xor(t_vg, off, 64);
    }
    if (lane == 0) {
        a.tot[s] = t_cpu;
        a.tot[(size_t)a.S + s] = t_mem;
        a.tot[(size_t)2 * a.S + s] = t_vg;
    }
    __syncthreads();

    // ---- pass 1: ranks from the closed form, and their inverse ----
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        if (j >= N || ((row[j >> 5] >> (j & 31)) & 1u) == 0) continue;
        const int i = rank[j], zq = s_zord[a.node_zone ? a.node_zone[j] : 0];
        int r = 0;
        for (int k = 0; k < nz; ++k) r += min(s_ocnt[k], i + (k < zq ? 1 : 0));
        rank[j] = r;
        if (r < N) inv[r] = j;
    }
    if (!a.ncls) return;

    // ---- pass 2, rank order: per-class node lists, a node's index inside its class, the class counts ----
    const int Ct = a.Ct;
    for (int d = lane; d < Ct; d += 64) s_fill[d] = 0;
    __syncthreads();                                                  // (also: pass 1's inv is visible to the whole wave)
    int32_t* const ids = a.rk_ids + (size_t)s * N;
    int32_t* const pos = a.rk_pos + (size_t)s * N;
    for (int base = 0; base < n; base += 64) {
        const int r = base + lane;
        const bool in = r < n;
        const int j = in ? inv[r] : 0;
        const int d = in ? a.ncls[j] : -1;
        unsigned long long left = __ballot(in);
        while (left) {                                                // one turn per distinct class among the chunk's nodes
            const int lead = __ffsll(left) - 1;
            const int dd = __shfl(d, lead, 64);
            const bool mine = in && d == dd;
            const unsigned long long m = __ballot(mine);
            const int before = s_fill[dd];
            if (mine) {
                const int p = before + __popcll(m & below);
                pos[j] = p;
                if (a.cls_off[dd] + p < N) ids[a.cls_off[dd] + p] = j;
            }
            if (lane == lead) s_fill[dd] = before + __popcll(m);
            left &= ~m;
        }
        __syncthreads();
    }
    for (int d = lane; d < Ct; d += 64) a.scls[(size_t)s * Ct + d] = s_fill[d];
}

// image_states_kernel (simon_subset.h): workgroup t = slot t.  s_cnt[q] = NumNodes of entry q in this slot (written for the entries of
// present nodes only: nothing else is read), s_first[i] = entry of the first present lister of image i, -1 = none present.
__global__ __launch_bounds__(256) void image_states_kernel(ImageStates a) {
    extern __shared__ int32_t smem[];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* const s_cnt = a.scratch ? a.scratch + (size_t)t * ((size_t)a.nnz + a.I) : smem;   // [nnz]
    int32_t* const s_first = s_cnt + a.nnz;                                                     // [I]
    const uint32_t* __restrict__ const row = a.present + (size_t)t * a.W;
    const unsigned long long below = (1ull << lane) - 1;

    // ---- phase A: one wave per image, 64 listers per turn; the count so far is carried from chunk to chunk ----
    for (int i = wave; i < a.I; i += 4) {
        const int lo = a.lis_off[i], hi = a.lis_off[i + 1];
        int carry = 0, first = -1;
        for (int base = lo; base < hi; base += 64) {
            const int k = base + lane;
            const int j = k < hi ? a.lis_node[k] : 0;
            const bool in = k < hi && ((row[j >> 5] >> (j & 31)) & 1u) != 0;
            const int q = in ? a.lis_ent[k] : 0;
            const unsigned long long m = __ballot(in);
            if (in) s_cnt[q] = carry + __popcll(m & below) + 1;           // (the node itself counts: "up to and including")
            if (first < 0 && m) first = __shfl(q, __ffsll(m) - 1, 64);
            carry += __popcll(m);
        }
        if (lane == 0) s_first[i] = first;
    }
    __syncthreads();                                                      // (a barrier orders the workgroup's own global writes too)

    // ---- phase B: one byte per (row, node class) ----
    const int n = a.slot_n[t];
    const long long mb = 1024 * 1024, lo_b = 23 * mb;
    uint8_t* const out = a.out + (size_t)t * a.R * a.Cn;
    for (int x = tid; x < a.R * a.Cn; x += 256) {
        const int r = x / a.Cn, k = x - r * a.Cn;
        const int j = a.rep[k];
        int score = 0;
        if (j >= 0 && ((row[j >> 5] >> (j & 31)) & 1u)) {
            const int cp = a.row_class[r], e0 = a.class_off[cp], e1 = a.class_off[cp + 1];
            const long long hi_b = 1000 * mb * (long long)(e1 - e0);
            const int q0 = a.node_off[j], q1 = a.node_off[j + 1];
            long long sum = 0;
            for (int e = e0; e < e1; ++e) {
                const int im = a.class_image[e];
                if (im < 0) continue;
                for (int q = q0; q < q1; ++q)
                    if (a.node_image[q] == im) {
                        sum += (long long)((double)a.node_size[s_first[im]] * ((double)s_cnt[q] / (double)n));
                        break;
                    }
                if (sum > hi_b) sum = hi_b + 1;                           // (saturates as img_score does)
            }
            sum = sum < lo_b ? lo_b : sum > hi_b ? hi_b : sum;
            score = (int)(100 * (sum - lo_b) / (hi_b - lo_b));
        }
        out[x] = (uint8_t)score;
    }
}

// group_counts_kernel: the placement row and pod_group are read coalesced (8 B per pod: the kernel is HBM-bound), the two histograms live in
// LDS behind LDS atomics and leave as rows of [S][G].
__global__ __launch_bounds__(256) void group_counts_kernel(const int32_t* __restrict__ placement, const int32_t* __restrict__ pod_group, int P, int G,
                                                           int32_t* __restrict__ unscheduled, int32_t* __restrict__ placed) {
    extern __shared__ int32_t smem[];
    int32_t* const h_uns = smem;             // [G] placement == SIMON_UNSCHEDULED
    int32_t* const h_pl = smem + G;          // [G] placement >= 0
    const int s = blockIdx.x, tid = threadIdx.x;
    for (int g = tid; g < 2 * G; g += 256) smem[g] = 0;
    __syncthreads();
    const int32_t* __restrict__ const row = placement + (size_t)s * P;
    for (int p = tid; p < P; p += 256) {
        const int g = pod_group[p], v = row[p];
        if (g < 0 || g >= G || v < -1) continue;                      // not counted; not part of the scenario (SIMON_GATED)
        atomicAdd(v < 0 ? &h_uns[g] : &h_pl[g], 1);
    }
    __syncthreads();
    for (int g = tid; g < G; g += 256) {
        unscheduled[(size_t)s * G + g] = h_uns[g];
        if (placed) placed[(size_t)s * G + g] = h_pl[g];
    }
}

// ---- simon_fetch_node_usage / simon_fetch_headroom / simon_fetch_gpu_usage / simon_fetch_headroom_gpu --------------------------------
// One pod's recorded devices onto its node's eight sums: byte d of the slices word times the pod's GPU memory per slice, one LDS atomic
// per non-zero byte (and 1 onto the device's pod count where kept).  A pod without a GPU request never touches the slices row.
__device__ __forceinline__ void dev_add(const DevUsage& g, const uint64_t* __restrict__ srow, int p, int jj,
                                        unsigned long long* s_dev, int32_t* s_dpods) {
    const long long m = g.gpu_mem[p];
    if (m <= 0) return;
    const uint64_t w = srow[p];
    if (w == 0) return;                                                 // (bound by Spec.NodeName: never reserved)
#pragma unroll
    for (int d = 0; d < kGpuDev; ++d) {
        const unsigned b = (unsigned)(w >> (8 * d)) & 255u;
        if (b == 0) continue;
        atomicAdd(&s_dev[dev_slot(jj, d)], (unsigned long long)b * (unsigned long long)m);
        if (s_dpods) atomicAdd(&s_dpods[dev_slot(jj, d)], 1);
    }
}

// One tile of the node range [t0, t1): s_req[i][j - t0] = request sum of accumulated row i over the pods placed on node j, s_cnt[j - t0]
// their number; DEV: also s_dev[dev_slot(j - t0, d)] = GPU memory the stream booked on device d of node j (srow: the scenario's slices
// row, nullptr = nothing booked).  The placement row is read coalesced; a pod whose node lies outside the tile (SIMON_UNSCHEDULED /
// SIMON_GATED: below 0) adds nothing.  Ends behind a barrier: every thread may read the tile.
template <bool DEV>
__device__ __forceinline__ void usage_accumulate(const UsageCommon& a, const int32_t* __restrict__ row, int t0, int t1,
                                                 unsigned long long* s_req, int32_t* s_cnt, const DevUsage* g = nullptr,
                                                 const uint64_t* __restrict__ srow = nullptr, unsigned long long* s_dev = nullptr) {
    const int tid = threadIdx.x, tile = a.tile;
    for (int i = tid; i < a.nrows * tile; i += 256) s_req[i] = 0;
    for (int i = tid; i < tile; i += 256) s_cnt[i] = 0;
    if (DEV)
        for (int i = tid; i < tile * kGpuDev; i += 256) s_dev[i] = 0;
    __syncthreads();
    for (int p = tid; p < a.P; p += 256) {
        const int v = row[p];
        if (v < t0 || v >= t1) continue;
        atomicAdd(&s_cnt[v - t0], 1);
        for (int i = 0; i < a.nrows; ++i) {
            const long long q = a.pod_req[(size_t)a.row_src[i] * a.P + p];
            if (q != 0) atomicAdd(&s_req[i * tile + (v - t0)], (unsigned long long)q);
        }
        if (DEV && srow) dev_add(*g, srow, p, v - t0, s_dev, nullptr);
    }
    __syncthreads();
}

// The device sums alone (gpu_usage_kernel): as above without the resource rows; s_dpods may be nullptr.
__device__ __forceinline__ void dev_accumulate(const UsageCommon& a, const DevUsage& g, const int32_t* __restrict__ row,
                                               const uint64_t* __restrict__ srow, int t0, int t1, unsigned long long* s_dev, int32_t* s_dpods) {
    const int tid = threadIdx.x, cells = a.tile * kGpuDev;
    for (int i = tid; i < cells; i += 256) s_dev[i] = 0;
    for (int i = tid; s_dpods && i < cells; i += 256) s_dpods[i] = 0;
    __syncthreads();
    for (int p = tid; srow && p < a.P; p += 256) {
        const int v = row[p];
        if (v < t0 || v >= t1) continue;
        dev_add(g, srow, p, v - t0, s_dev, s_dpods);
    }
    __syncthreads();
}

__device__ __forceinline__ bool usage_holds(const UsageCommon& a, int s, int j) {
    return a.rank ? a.rank[(size_t)s * a.N + j] < a.N : j < a.scen[2 * s];
}

// node_usage_kernel: workgroup b = listed scenario b.  Rows leave coalesced; a node the scenario lacks reads 0 / npods -1.
__global__ __launch_bounds__(256) void node_usage_kernel(UsageCommon a, UsageOut o) {
    extern __shared__ unsigned long long usage_smem[];
    unsigned long long* const s_req = usage_smem;                       // [nrows][tile]
    int32_t* const s_cnt = (int32_t*)(usage_smem + (size_t)a.nrows * a.tile);   // [tile]
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int s = o.scen_ids ? o.scen_ids[b] : b;
    const int32_t* __restrict__ const row = a.placement + (size_t)s * a.P;
    for (int t0 = 0; t0 < N; t0 += a.tile) {
        const int t1 = min(t0 + a.tile, N);
        usage_accumulate<false>(a, row, t0, t1, s_req, s_cnt);
        for (int j = t0 + tid; j < t1; j += 256) {
            const bool in = usage_holds(a, s, j);
            for (int i = 0; i < a.nrows; ++i)
                o.rows[i][(size_t)b * o.row_stride[i] + j] = in ? a.node_init[(size_t)a.row_src[i] * N + j] + (long long)s_req[i * a.tile + (j - t0)] : 0;
            o.npods[(size_t)b * N + j] = in ? a.init_npods[j] + s_cnt[j - t0] : -1;
        }
        __syncthreads();                                                // (the next tile zeroes what this one read)
    }
}

// gpu_usage_kernel: workgroup b = listed scenario b.  [n][N][8] leaves coalesced (thread i of a pass = device i & 7 of tile node i >> 3);
// a node the scenario lacks reads 0 / dev_pods -1, a device the node lacks 0 / 0.
__global__ __launch_bounds__(256) void gpu_usage_kernel(UsageCommon a, DevUsage g, GpuUsageOut o) {
    extern __shared__ unsigned long long usage_smem[];
    unsigned long long* const s_dev = usage_smem;                       // [tile][8]
    int32_t* const s_dpods = o.dev_pods ? (int32_t*)(usage_smem + (size_t)a.tile * kGpuDev) : nullptr;   // [tile][8]
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int s = o.scen_ids ? o.scen_ids[b] : b;
    const int32_t* __restrict__ const row = a.placement + (size_t)s * a.P;
    const uint64_t* __restrict__ const srow = g.slices ? g.slices + (size_t)s * a.P : nullptr;
    for (int t0 = 0; t0 < N; t0 += a.tile) {
        const int t1 = min(t0 + a.tile, N);
        dev_accumulate(a, g, row, srow, t0, t1, s_dev, s_dpods);
        for (int i = tid; i < (t1 - t0) * kGpuDev; i += 256) {
            const int jj = i >> 3, d = i & 7, j = t0 + jj;
            const bool in = usage_holds(a, s, j), live = d < g.node_cnt[j];
            const size_t at = ((size_t)b * N + j) * kGpuDev + d;
            o.dev_used[at] = in && live ? g.init_used[(size_t)j * kGpuDev + d] + (long long)s_dev[dev_slot(jj, d)] : 0;
            if (o.dev_pods) o.dev_pods[at] = !in ? -1 : live ? s_dpods[dev_slot(jj, d)] : 0;
        }
        __syncthreads();                                                // (the next tile zeroes what this one read)
    }
}

// The cap of one probe on node j of the tile that starts at t0 (headroom_kernel below): pod slots, the resources fitsRequest compares
// and, DEV, the slices the node's devices still hold.
template <bool DEV>
__device__ __forceinline__ long long node_cap(const UsageCommon& a, const HeadroomArgs& h, const DevUsage& g, const ProbeRow& pr, long long gm, int gc,
                                              const unsigned long long* s_req, const int32_t* s_cnt, const unsigned long long* s_dev, int j, int t0) {
    const int N = a.N;
    long long cap = (long long)h.alloc_pods[j] - a.init_npods[j] - s_cnt[j - t0];      // pod slots
    int ai = 0;                                                         // (the accumulated rows are an ascending subset of the resource rows)
    for (int r = 0; r < kUsageRows && cap > 0; ++r) {
        long long used = a.node_init[(size_t)r * N + j];
        if (ai < a.nrows && a.row_src[ai] == r) used += (long long)s_req[ai++ * a.tile + (j - t0)];
        if (!((pr.checked >> r) & 1u)) continue;
        const long long room = h.node_alloc[(size_t)r * N + j] - used, q = pr.q[r];
        if (room < 0) cap = 0;                                          // over-committed: Allocatable < request + Requested whatever the request
        else if (q > 0) cap = min(cap, room / q);
    }
    if (DEV && gm > 0 && cap > 0) {
        long long T = 0;
        const int cnt = gc > 0 ? g.node_cnt[j] : 0;
        const long long per = g.per_dev[j];
        for (int d = 0; d < cnt; ++d) {
            const long long idle = per - g.init_used[(size_t)j * kGpuDev + d] - (long long)s_dev[dev_slot(j - t0, d)];
            if (idle > 0) T += idle / gm;                               // (an over-booked device holds nothing)
        }
        cap = gc > 0 ? min(cap, T / gc) : 0;
    }
    return cap;
}

// ---- Open-Local: simon_fetch_local_usage / simon_fetch_headroom_local ----------------------------------------------------------------
struct LocalState {
    long long req[kLocalVG];                 // SharedResource.Requested of the node's volume groups
    int alloc;                               // bit d: ExclusiveResource.IsAllocated
};

__device__ __forceinline__ bool same_state(const LocalState& x, const LocalState& y) {
    bool eq = x.alloc == y.alloc;
#pragma unroll
    for (int q = 0; q < kLocalVG; ++q) eq = eq && x.req[q] == y.req[q];
    return eq;
}

// One pod's volumes onto node j: local_allocate + the commit of LocalPlugin.Bind as oracle/simon_oracle.c restates them, which is what
// local_eval<COMMIT> of simon_wide.hip does for the pod it places.  LVM volumes in spec order (a named group by interned name, otherwise
// the smallest free size that fits, ties in annotation order, this pod's earlier volumes counted); then SSD and HDD volumes by
// CheckExclusiveResourceMeetsPVCSize: free devices ascending by (capacity, index), sizes ascending as the spec carries them, two
// pointers, failing only when the LAST device is too small.  True = allocated, st holds the new state; false = st is untouched.
__device__ bool local_apply(const LocalUsage& L, const LocalSpec& sp, int j, LocalState& st) {
    if (!(L.flags[j] & 1)) return false;                                // SIMON_FAIL_LOCAL
    long long req[kLocalVG];
#pragma unroll
    for (int q = 0; q < kLocalVG; ++q) req[q] = st.req[q];
    if (sp.n_lvm > 0) {
        const int nvg = L.vg_cnt[j];
        if (nvg <= 0) return false;
        long long cap[kLocalVG];
        int name[kLocalVG];
#pragma unroll
        for (int q = 0; q < kLocalVG; ++q) {
            cap[q] = L.vg_cap[(size_t)j * kLocalVG + q];
            name[q] = L.vg_name[(size_t)j * kLocalVG + q];
        }
        for (int k = 0; k < sp.n_lvm; ++k) {
            const long long size = sp.lvm_size[k];
            const int want = sp.lvm_vg[k];
            int pick = -1;
            long long pick_free = 0;
#pragma unroll
            for (int q = 0; q < kLocalVG; ++q) {
                if (q >= nvg) continue;
                const long long fr = cap[q] - req[q];
                if (want >= 0) {
                    if (pick < 0 && name[q] == want) { pick = q; pick_free = fr; }
                } else if (fr >= size && (pick < 0 || fr < pick_free)) {
                    pick = q; pick_free = fr;
                }
            }
            if (pick < 0 || pick_free < size) return false;
#pragma unroll
            for (int q = 0; q < kLocalVG; ++q)
                if (q == pick) req[q] += size;
        }
    }
    int newly = 0;
    if (sp.n_ssd + sp.n_hdd > 0) {
        const int cnt = L.dev_cnt[j], media = L.dev_media[j];
        const int64_t* __restrict__ const dcap = L.dev_cap + (size_t)j * kLocalDev;
        for (int m = 1; m <= 2; ++m) {                                  // SSD first, then HDD
            const int n_pvc = m == 1 ? sp.n_ssd : sp.n_hdd;
            const int64_t* const sizes = m == 1 ? sp.ssd_size : sp.hdd_size;
            unsigned free_mask = 0;
            for (int d = 0; d < cnt; ++d)
                if (((media >> (2 * d)) & 3) == m && !((st.alloc >> d) & 1)) free_mask |= 1u << d;
            const int nfree = __popc(free_mask);
            if (nfree < n_pvc) return false;
            int i = 0;
            for (int step = 0; step < nfree && n_pvc > 0; ++step) {
                int d = -1;
                long long c = 0;
                for (int e = 0; e < cnt; ++e)
                    if (((free_mask >> e) & 1u) && (d < 0 || dcap[e] < c)) { d = e; c = dcap[e]; }
                free_mask &= ~(1u << d);
                if (c < sizes[i]) {
                    if (step == nfree - 1) return false;
                    continue;
                }
                newly |= 1 << d;
                if (++i == n_pvc) break;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kLocalVG; ++q) st.req[q] = req[q];
    st.alloc |= newly;
    return true;
}

__device__ __forceinline__ LocalState local_load(const long long* s_vg, const int32_t* s_ldev, int tile, int jj) {
    LocalState st;
#pragma unroll
    for (int q = 0; q < kLocalVG; ++q) st.req[q] = s_vg[q * tile + jj];
    st.alloc = s_ldev[jj];
    return st;
}

// One tile of the node range [t0, t1): s_vg[q][j - t0] / s_ldev[j - t0] = the storage state of node j after the scheduled storage pods
// of the scenario's order (L.list[lo, hi)).  Thread t owns the tile nodes t, t + 256, ...: it sets their state before the stream and
// applies, chunk by chunk and front to back, the staged pods whose placement names one of them -- stream order per node, nothing shared.
// s_stage: [2][kLocalChunk] node and spec of the staged pods.  Ends behind a barrier: every thread may read the tile.
__device__ __forceinline__ void local_replay(const UsageCommon& a, const LocalUsage& L, const int32_t* __restrict__ row, int lo, int hi, int t0,
                                             int t1, long long* s_vg, int32_t* s_ldev, int32_t* s_stage) {
    const int tid = threadIdx.x, tile = a.tile, tw = t1 - t0;
    for (int jj = tid; jj < tw; jj += 256) {
#pragma unroll
        for (int q = 0; q < kLocalVG; ++q) s_vg[q * tile + jj] = L.flags ? L.vg_init[(size_t)(t0 + jj) * kLocalVG + q] : 0;
        s_ldev[jj] = L.flags ? L.dev_init[t0 + jj] : 0;
    }
    for (int c0 = lo; L.flags && c0 < hi; c0 += kLocalChunk) {
        const int cn = min(kLocalChunk, hi - c0);
        __syncthreads();                                                // (the last chunk has been read)
        for (int i = tid; i < cn; i += 256) {
            const int p = L.list[c0 + i];
            s_stage[i] = row[p];
            s_stage[kLocalChunk + i] = L.pod_spec[p];
        }
        __syncthreads();
        for (int i = 0; i < cn; ++i) {
            const int jj = s_stage[i] - t0;                             // (SIMON_UNSCHEDULED / SIMON_GATED: below 0)
            if ((unsigned)jj >= (unsigned)tw || (jj & 255) != tid) continue;
            LocalState st = local_load(s_vg, s_ldev, tile, jj);
            if (!local_apply(L, L.specs[s_stage[kLocalChunk + i]], t0 + jj, st)) continue;   // (a row from another problem: commits nothing)
#pragma unroll
            for (int q = 0; q < kLocalVG; ++q) s_vg[q * tile + jj] = st.req[q];
            s_ldev[jj] = st.alloc;
        }
    }
    __syncthreads();
}

// local_usage_kernel: workgroup b = listed scenario b.  [n][N][4] / [n][N] leave coalesced; a node the scenario lacks reads 0 / -1, a node
// without the storage annotation 0 / 0, a volume group the node lacks 0.
__global__ __launch_bounds__(256) void local_usage_kernel(UsageCommon a, LocalUsage L, LocalUsageOut o) {
    extern __shared__ unsigned long long usage_smem[];
    long long* const s_vg = (long long*)usage_smem;                     // [4][tile]
    int32_t* const s_ldev = (int32_t*)(s_vg + (size_t)kLocalVG * a.tile);   // [tile]
    int32_t* const s_stage = s_ldev + a.tile;                           // [2][kLocalChunk]
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int s = o.scen_ids ? o.scen_ids[b] : b;
    const int32_t* __restrict__ const row = a.placement + (size_t)s * a.P;
    const int order = a.scen[2 * s + 1];
    const int lo = L.flags ? L.list_off[order] : 0, hi = L.flags ? L.list_off[order + 1] : 0;
    for (int t0 = 0; t0 < N; t0 += a.tile) {
        const int t1 = min(t0 + a.tile, N);
        local_replay(a, L, row, lo, hi, t0, t1, s_vg, s_ldev, s_stage);
        for (int i = tid; i < (t1 - t0) * kLocalVG; i += 256) {
            const int jj = i >> 2, q = i & 3, j = t0 + jj;
            const bool live = L.flags && (L.flags[j] & 1) && q < L.vg_cnt[j] && usage_holds(a, s, j);
            o.vg_req[((size_t)b * N + j) * kLocalVG + q] = live ? s_vg[q * a.tile + jj] : 0;
        }
        for (int j = t0 + tid; o.dev_alloc && j < t1; j += 256)
            o.dev_alloc[(size_t)b * N + j] = !usage_holds(a, s, j) ? -1 : L.flags && (L.flags[j] & 1) ? s_ldev[j - t0] : 0;
        __syncthreads();                                                // (the next tile overwrites what this one read)
    }
}

// headroom_kernel: workgroup s = scenario s of the batch.  Per tile the same accumulation; then, per probe, every thread takes the cap
// of its nodes of the tile (node_cap) and the workgroup adds them up in LDS.  Only [S][K] counters leave.  DEV
// (simon_fetch_headroom_gpu): the tile also carries the device sums, and a probe with a GPU request is bounded by the slices the
// node's devices still hold: T = sum over the node's devices of max(per_dev - used, 0) / mem, cap_gpu = T / count
// (GpuNodeInfo.AllocateGpuId accepts such a pod iff T >= count, and every accepted pod lowers T by count).  LOCAL
// (simon_fetch_headroom_local): the storage pods are replayed after the tile's accumulation, and a probe whose class has an Open-Local
// spec is bounded, per node, by the number of consecutive local_apply steps of that spec that succeed on a private copy of the node's
// end state, at most the cap so far; a step that leaves the state unchanged (no volume, no device) ends the count at the cap so far.
// The state after m copies depends only on m and a failed copy changes nothing, so the bound is what the scheduler places.
template <bool DEV, bool LOCAL>
__global__ __launch_bounds__(256) void headroom_kernel(UsageCommon a, HeadroomArgs h, DevUsage g, LocalUsage L) {
    extern __shared__ unsigned long long usage_smem[];
    const HeadroomLds lds{a.nrows, h.K, DEV, LOCAL};
    unsigned long long* const s_req = usage_smem;                       // [nrows][tile]
    unsigned long long* const s_dev = s_req + lds.req(a.tile);          // DEV: [tile][8]
    long long* const s_vg = (long long*)(s_dev + lds.dev(a.tile));      // LOCAL: [4][tile]
    unsigned long long* const s_fit = (unsigned long long*)(s_vg + lds.vg(a.tile));   // [K]
    int32_t* const s_cnt = (int32_t*)(s_fit + lds.fit());               // [tile]
    int32_t* const s_nodes = s_cnt + lds.cnt(a.tile);                   // [K]
    int32_t* const s_ldev = s_nodes + lds.nodes();                      // LOCAL: [tile]
    int32_t* const s_stage = s_ldev + lds.ldev(a.tile);                 // LOCAL: [2][kLocalChunk]
    const int s = blockIdx.x, tid = threadIdx.x, N = a.N, K = h.K, W = (N + 63) >> 6;
    const int32_t* __restrict__ const row = a.placement + (size_t)s * a.P;
    const uint64_t* __restrict__ const srow = DEV && g.slices ? g.slices + (size_t)s * a.P : nullptr;
    const int order = LOCAL ? a.scen[2 * s + 1] : 0;
    const int lo = LOCAL && L.flags ? L.list_off[order] : 0, hi = LOCAL && L.flags ? L.list_off[order + 1] : 0;
    for (int k = tid; k < K; k += 256) { s_fit[k] = 0; s_nodes[k] = 0; }
    for (int t0 = 0; t0 < N; t0 += a.tile) {
        const int t1 = min(t0 + a.tile, N);
        usage_accumulate<DEV>(a, row, t0, t1, s_req, s_cnt, &g, srow, s_dev);   // (its first barrier also covers s_fit / s_nodes)
        if (LOCAL) local_replay(a, L, row, lo, hi, t0, t1, s_vg, s_ldev, s_stage);
        for (int k = 0; k < K; ++k) {
            const ProbeRow& pr = h.probes[k];
            const uint64_t* __restrict__ const mask = h.probe_mask + (size_t)k * W;
            const long long gm = DEV ? g.probe_mem[k] : 0;
            const int gc = DEV ? g.probe_cnt[k] : 0;
            const int spec = LOCAL && L.flags ? L.probe_spec[k] : -1;
            long long fit = 0;
            int nodes = 0;
            for (int j = t0 + tid; j < t1; j += 256) {
                if (!((mask[j >> 6] >> (j & 63)) & 1ull) || !usage_holds(a, s, j)) continue;
                long long cap;
                if (DEV && !LOCAL) {
                    // node_cap<true> in place, for this instantiation only, kept because in place the kernel compiles to the instruction
                    // stream it had (so its time needs no argument), not because the call was shown to be too slow: with the call it
                    // came out in another order and measured 2.790 against 2.778 ms (8 GPU probes, config 5's shape, five rounds: one
                    // round 0.6 us past the parent's spread, profiles/usage_refactor/README.md).  A change there belongs here too.
                    cap = (long long)h.alloc_pods[j] - a.init_npods[j] - s_cnt[j - t0];
                    int ai = 0;
                    for (int r = 0; r < kUsageRows && cap > 0; ++r) {
                        long long used = a.node_init[(size_t)r * N + j];
                        if (ai < a.nrows && a.row_src[ai] == r) used += (long long)s_req[ai++ * a.tile + (j - t0)];
                        if (!((pr.checked >> r) & 1u)) continue;
                        const long long room = h.node_alloc[(size_t)r * N + j] - used, q = pr.q[r];
                        if (room < 0) cap = 0;
                        else if (q > 0) cap = min(cap, room / q);
                    }
                    if (gm > 0 && cap > 0) {
                        long long T = 0;
                        const int cnt = gc > 0 ? g.node_cnt[j] : 0;
                        const long long per = g.per_dev[j];
                        for (int d = 0; d < cnt; ++d) {
                            const long long idle = per - g.init_used[(size_t)j * kGpuDev + d] - (long long)s_dev[dev_slot(j - t0, d)];
                            if (idle > 0) T += idle / gm;
                        }
                        cap = gc > 0 ? min(cap, T / gc) : 0;
                    }
                } else
                    cap = node_cap<DEV>(a, h, g, pr, gm, gc, s_req, s_cnt, s_dev, j, t0);
                if (LOCAL && spec >= 0 && cap > 0) {
                    LocalState st = local_load(s_vg, s_ldev, a.tile, j - t0);
                    long long m = 0;
                    while (m < cap) {
                        const LocalState was = st;
                        if (!local_apply(L, L.specs[spec], j, st)) break;
                        if (same_state(was, st)) { m = cap; break; }
                        ++m;
                    }
                    cap = m;
                }
                if (cap > 0) { fit += cap; ++nodes; }
            }
            for (int off = 32; off > 0; off >>= 1) {
                fit += __shfl_xor(fit, off, 64);
                nodes += __shfl_xor(nodes, off, 64);
            }
            if ((tid & 63) == 0 && nodes) {
                atomicAdd(&s_fit[k], (unsigned long long)fit);
                atomicAdd(&s_nodes[k], nodes);
            }
        }
        __syncthreads();
    }
    for (int k = tid; k < K; k += 256) {
        h.fit[(size_t)s * K + k] = (long long)s_fit[k];
        if (h.fit_nodes) h.fit_nodes[(size_t)s * K + k] = s_nodes[k];
    }
}

}  // namespace

// every array a launch reads is there (`headroom`: the per-probe ones too); a LocalUsage without flags is a problem without Open-Local
static bool complete(const DevUsage& g, bool headroom) {
    return g.gpu_mem && g.node_cnt && g.init_used && (!headroom || (g.per_dev && g.probe_mem && g.probe_cnt));
}
static bool complete(const LocalUsage& l, bool headroom) {
    return !l.flags || (l.specs && l.pod_spec && l.list && l.list_off && l.vg_cnt && l.vg_cap && l.vg_init && l.vg_name && l.dev_cnt && l.dev_cap &&
                        l.dev_media && l.dev_init && (!headroom || l.probe_spec));
}

hipError_t launch_node_usage(const UsageCommon& a, const UsageOut& o, int n, hipStream_t st) {
    if (n <= 0 || a.N <= 0 || a.tile <= 0 || a.nrows < 2 || a.nrows > kUsageRows) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.tile * usage_node_bytes(a.nrows);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(node_usage_kernel, dim3((unsigned)n), dim3(256), lds, st, a, o);
    return hipGetLastError();
}

hipError_t launch_gpu_usage(const UsageCommon& a, const DevUsage& g, const GpuUsageOut& o, int n, hipStream_t st) {
    if (n <= 0 || a.N <= 0 || a.tile <= 0 || !o.dev_used || !complete(g, false)) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.tile * usage_node_bytes(0, kDevBytes + (o.dev_pods ? kDevPodsBytes : 0));
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gpu_usage_kernel, dim3((unsigned)n), dim3(256), lds, st, a, g, o);
    return hipGetLastError();
}

hipError_t launch_local_usage(const UsageCommon& a, const LocalUsage& l, const LocalUsageOut& o, int n, hipStream_t st) {
    if (n <= 0 || a.N <= 0 || a.tile <= 0 || !o.vg_req || !complete(l, false)) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.tile * kLocalBytes + kLocalStageBytes;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(local_usage_kernel, dim3((unsigned)n), dim3(256), lds, st, a, l, o);
    return hipGetLastError();
}

hipError_t launch_headroom(const UsageCommon& a, const HeadroomArgs& h, const DevUsage& g, const LocalUsage& l, bool devices, bool storage, int S,
                           hipStream_t st) {
    if (S <= 0 || a.N <= 0 || a.tile <= 0 || a.nrows < 2 || a.nrows > kUsageRows || h.K < 1 || h.K > kMaxProbes) return hipErrorInvalidValue;
    if ((devices && !complete(g, true)) || (storage && !complete(l, true))) return hipErrorInvalidValue;
    const size_t lds = HeadroomLds{a.nrows, h.K, devices, storage}.bytes(a.tile);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const auto kernel = storage ? (devices ? headroom_kernel<true, true> : headroom_kernel<false, true>)
                                : (devices ? headroom_kernel<true, false> : headroom_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(256), lds, st, a, h, devices ? g : DevUsage{}, storage ? l : LocalUsage{});
    return hipGetLastError();
}

hipError_t launch_group_counts(const int32_t* placement, const int32_t* pod_group, int S, int P, int G, int32_t* unscheduled, int32_t* placed,
                               hipStream_t st) {
    if (S <= 0 || G <= 0 || G > kMaxPodGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_counts_kernel, dim3((unsigned)S), dim3(256), (size_t)2 * G * sizeof(int32_t), st, placement, pod_group, P, G, unscheduled, placed);
    return hipGetLastError();
}

hipError_t launch_image_states(const ImageStates& a, hipStream_t st) {
    if (a.T <= 0 || a.R <= 0 || a.Cn <= 0) return hipSuccess;
    if (a.W <= 0 || a.I < 0 || a.nnz < 0 || !a.out || !a.present || !a.slot_n || !a.rep) return hipErrorInvalidValue;
    const size_t lds = ((size_t)a.nnz + a.I) * sizeof(int32_t);
    if (!a.scratch && lds > kImageLdsBudget) return hipErrorInvalidValue;
    hipLaunchKernelGGL(image_states_kernel, dim3((unsigned)a.T), dim3(256), a.scratch ? 0 : lds, st, a);
    return hipGetLastError();
}

hipError_t launch_subset_stage(const SubsetStage& a, hipStream_t st) {
    if (a.S <= 0 || a.N <= 0) return hipSuccess;
    const size_t lds = (size_t)(128 + (a.ncls ? a.Ct : 0)) * sizeof(int32_t);
    hipLaunchKernelGGL(subset_stage_kernel, dim3((unsigned)a.S), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace simon

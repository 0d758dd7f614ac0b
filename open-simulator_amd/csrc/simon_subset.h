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

// simon_fetch_group_counts: per scenario and pod group, the pods left unscheduled (placement == -1) and the pods placed (>= 0) -- a pod that
// is not part of the scenario (-2) counts in neither.  placement [S][P] by pod id, pod_group [P] in [0, G) or -1 (validated by the caller),
// unscheduled / placed [S][G] (placed may be null).  One workgroup per scenario, two G-entry histograms in LDS.
constexpr int kMaxPodGroups = 1024;          // SIMON_MAX_POD_GROUPS
hipError_t launch_group_counts(const int32_t* placement, const int32_t* pod_group, int S, int P, int G, int32_t* unscheduled, int32_t* placed,
                               hipStream_t st);

}  // namespace simon

// simon_podsets.h -- host-side checks of the pod-subset calls (simon_set_scenario_pods, simon_fetch_group_counts): plain C++ without a
// HIP dependency, so that a stand-alone program can run them under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace simon {

inline int pod_row_words(int P) { return (P + 31) / 32; }

// Presence rows [S][pod_row_words(P)]: pod p of scenario s = bit (p & 31) of word p >> 5.  Returns -1 when no row sets a bit at or
// beyond P, else the first scenario that does (*bit receives the offending pod id).
inline int pod_rows_first_bad(const uint32_t* present, int S, int P, int* bit) {
    const int W = pod_row_words(P), tail = P & 31;
    if (tail == 0) return -1;                                         // every bit of every word names a pod
    const uint32_t beyond = ~0u << tail;
    for (int s = 0; s < S; ++s) {
        const uint32_t w = present[(size_t)s * W + (W - 1)] & beyond;
        if (w) {
            int b = tail;
            while (!((w >> b) & 1u)) ++b;
            if (bit) *bit = (W - 1) * 32 + b;
            return s;
        }
    }
    return -1;
}

// pod_group [P]: ids in [0, G) or -1.  Returns -1 when all are, else the first pod whose id is not.
inline int pod_groups_first_bad(const int32_t* pod_group, int P, int G) {
    for (int p = 0; p < P; ++p)
        if (pod_group[p] < -1 || pod_group[p] >= G) return p;
    return -1;
}

}  // namespace simon

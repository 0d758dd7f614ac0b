// usage_lds_check.hip -- the node tiles and LDS sizes of the usage / headroom launches, printed from the helpers of csrc/simon_subset.h the
// way simon_hip.hip calls them.  Launches nothing and needs no GPU; tests/test_usage_lds.py builds it with hipcc and checks the figures.
//     hipcc --offload-arch=gfx950 -std=c++17 -I open-simulator_amd/csrc tests/cabi/usage_lds_check.hip -o usage_lds_check
#include <stdio.h>

#include "simon_subset.h"

using namespace simon;

static int headroom_tile(int N, const HeadroomLds& lds, int forced) { return usage_tile(N, lds.node_bytes(), lds.reserve_bytes(), forced); }

int main() {
    const int N = 5000, modes[2] = {0, 1 << 30};                       // forced: the LDS budget; one workgroup per CU
    const char* const mode_name[2] = {"budget", "cu"};
    for (int m = 0; m < 2; ++m) {
        const int f = modes[m];
        printf("tile node_usage_2rows %s %d\n", mode_name[m], usage_tile(N, usage_node_bytes(2), kTileReserve, f));
        printf("tile gpu_usage %s %d\n", mode_name[m], usage_tile(N, usage_node_bytes(0, kDevBytes), kTileReserve, f));
        printf("tile gpu_usage_dev_pods %s %d\n", mode_name[m], usage_tile(N, usage_node_bytes(0, kDevBytes + kDevPodsBytes), kTileReserve, f));
        printf("tile local_usage %s %d\n", mode_name[m], usage_tile(N, kLocalBytes, kTileReserve + kLocalStageBytes, f));
        printf("tile headroom_2rows %s %d\n", mode_name[m], headroom_tile(N, HeadroomLds{2, 8, false, false}, f));
        printf("tile headroom_2rows_devices %s %d\n", mode_name[m], headroom_tile(N, HeadroomLds{2, 8, true, false}, f));
        printf("tile headroom_2rows_storage %s %d\n", mode_name[m], headroom_tile(N, HeadroomLds{2, 8, false, true}, f));
        printf("tile headroom_2rows_storage_devices %s %d\n", mode_name[m], headroom_tile(N, HeadroomLds{2, 8, true, true}, f));
        printf("tile headroom_2rows_n1512 %s %d\n", mode_name[m], headroom_tile(1512, HeadroomLds{2, 8, false, false}, f));
    }
    // the launch's LDS at the chosen tile: rows, devices, storage, K, mode -> tile, bytes
    for (int rows = 2; rows <= kUsageRows; ++rows)
        for (int dev = 0; dev < 2; ++dev)
            for (int sto = 0; sto < 2; ++sto)
                for (int K = 1; K <= kMaxProbes; K += kMaxProbes - 1)
                    for (int m = 0; m < 2; ++m) {
                        const HeadroomLds lds{rows, K, dev != 0, sto != 0};
                        const int tile = headroom_tile(N, lds, modes[m]);
                        printf("lds %d %d %d %d %s %d %zu %zu %zu\n", rows, dev, sto, K, mode_name[m], tile, lds.bytes(tile), lds.node_bytes(), lds.fixed_bytes());
                    }
    return 0;
}

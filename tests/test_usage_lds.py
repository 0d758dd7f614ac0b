"""The node tiles and the LDS sizes of the usage / headroom launches (usage_tile and HeadroomLds of csrc/simon_subset.h) against the
documented values: the tiles docs/KERNELS.md and the measurement READMEs (profiles/usage, profiles/gpu_usage, profiles/local_usage) give
for 5 000 and 1 512 nodes, the bytes per node and beside the tile of every headroom layout, and one workgroup's 64 KB as the ceiling
of every launch.  tests/cabi/usage_lds_check.hip prints the figures the way the library computes them; it launches nothing, so this
test needs hipcc and no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (budget = four workgroups per CU share 40 KB each, cu = one workgroup per CU takes what 64 KB hold); None: not documented
TILES = {
    "node_usage_2rows": (2048, 3225),
    "headroom_2rows": (2048, 3225),
    "headroom_2rows_devices": (None, 768),
    "gpu_usage": (None, 1008),
    "gpu_usage_dev_pods": (None, 672),
    "local_usage": (1088, 1678),
    "headroom_2rows_storage": (704, 1078),
    "headroom_2rows_storage_devices": (320, 503),
    "headroom_2rows_n1512": (1512, None),
}


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("usage_lds") / "usage_lds_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "open-simulator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cabi", "usage_lds_check.hip"), "-o", exe], check=True, capture_output=True, timeout=600)
    return [line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]


def test_tiles_are_the_documented_ones(figures):
    got = {(f[1], f[2]): int(f[3]) for f in figures if f[0] == "tile"}
    for case, (budget, cu) in TILES.items():
        for mode, want in (("budget", budget), ("cu", cu)):
            if want is not None:
                assert got[(case, mode)] == want, (case, mode)


def test_every_headroom_launch_fits_one_workgroup_s_lds(figures):
    rows = [f for f in figures if f[0] == "lds"]
    assert len(rows) == 6 * 2 * 2 * 2 * 2                                 # rows 2 .. 7, devices, storage, K in {1, 64}, both modes
    for _, nrows, dev, sto, K, mode, tile, lds, per, fixed in rows:
        nrows, dev, sto, K, tile, lds, per, fixed = map(int, (nrows, dev, sto, K, tile, lds, per, fixed))
        assert per == nrows * 8 + 4 + 64 * dev + 36 * sto and fixed == 12 * K + 4096 * sto, (nrows, dev, sto, K)
        assert lds == tile * per + fixed and 1 <= tile <= 5000 and lds <= 65536, (nrows, dev, sto, K, mode, tile, lds)
        if mode == "cu":                                                  # the largest tile 64 KB hold, the counters of 64 probes kept free
            assert (tile + 1) * per + 1024 + 4096 * sto > 65536 or tile == 5000, (nrows, dev, sto, K, tile)

// grid_plan_driver.cpp -- stand-alone host program around csrc/dpm_grid_plan.hpp, built and run by tests/grid_plan.py
// (tests/test_grid_plan_host.py, tests/test_gpu_large_routes.py).  One case per line of standard input:
//   n u n_cu blocks_per_cu block_threads big_tiles
// one line of "name=value" pairs per case on standard output.
#include <cinttypes>
#include <cstdio>

#include "dpm_grid_plan.hpp"

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    long long n;
    int u, n_cu, blocks_per_cu, block_threads, big_tiles;
    if (std::sscanf(line, "%lld %d %d %d %d %d", &n, &u, &n_cu, &blocks_per_cu, &block_threads, &big_tiles) != 6) continue;
    const StreamGridPlan g = stream_grid_plan(n, u, n_cu, blocks_per_cu, block_threads);
    std::printf("iters=%" PRId64 " threads=%d blocks=%" PRId64 " big=%d scalar_blocks=%" PRId64 " fused=%d aux_vec_blocks=%" PRId64
                " aux_blocks=%" PRId64 "\n",
                g.iters, g.threads, g.blocks, (int)stream_big(n, n_cu), scalar_grid_blocks(n, n_cu),
                (int)lone_takes_fused_shape(n, big_tiles), aux_grid_blocks(n, n_cu, true), aux_grid_blocks(n, n_cu, false));
  }
  return 0;
}

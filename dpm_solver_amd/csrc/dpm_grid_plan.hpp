// dpm_grid_plan.hpp -- the launch-shape arithmetic of the single-request launchers: which grid a launch of n elements gets
// and where a large launch changes route.  stream_grid / scalar_grid / launch_stream (dpm_launch.hpp), dpm_stage_launch_dyn,
// dpm_add_noise_launch and dpm_blend_launch (dpm_kernels.hip) call it and keep their dim3 wrappers.
// Plain C++17: the standard library only, nothing of HIP -- so that a host compiler and a CPU test
// (tests/test_grid_plan_host.py) reach it, and so that the GPU sweep of the large routes (tests/test_gpu_large_routes.py) asks
// the same functions which route a size takes instead of restating a gate.
#pragma once
#include <algorithm>
#include <cstdint>

namespace {

constexpr int64_t GRID_GROUP_ELEMS = 8;   // elements of a lane's access group (EPT)
constexpr int64_t GRID_TILE_GROUPS = 256; // groups of a tile: one per lane of a 256-lane group (2048 elements)
constexpr int GRID_MAX_THREADS = 512;     // the streaming kernels' largest workgroup (STAGE_MAX_THREADS)
constexpr int64_t GRID_SCALAR_PER_CU = 16; // workgroups per CU of the one-element-per-lane and the aux kernels' grid cap

// 2048-element tiles a launch of n elements is counted in (a tile of a ragged n is counted by its whole groups)
inline int64_t grid_tiles(int64_t n) { return (n / GRID_GROUP_ELEMS + GRID_TILE_GROUPS - 1) / GRID_TILE_GROUPS; }

struct StreamGridPlan {
  int64_t iters;   // workgroup iterations of 256 lanes the launch is made of: u tiles each
  int threads;     // per workgroup: 256, or 512 (two 256-lane groups) when that still leaves two workgroups per CU
  int64_t blocks;  // workgroups: one per `threads / 256` iterations, capped per CU (then the kernel loops)
};
// launch shape of the streaming family's vector kernels at u tiles per iteration.  block_threads > 0 (Tuning::block_threads,
// lab build) fixes the workgroup size; blocks_per_cu is Tuning::blocks_per_cu.
inline StreamGridPlan stream_grid_plan(int64_t n, int u, int n_cu, int blocks_per_cu, int block_threads) {
  StreamGridPlan g;
  g.iters = (grid_tiles(n) + u - 1) / u;
  g.threads = 256;
  if (block_threads > 0) g.threads = block_threads;
  else if (g.iters >= 4 * (int64_t)n_cu) g.threads = GRID_MAX_THREADS;
  const int64_t per = g.threads / 256;
  const int64_t blocks = std::min((g.iters + per - 1) / per, std::max<int64_t>(1, (int64_t)n_cu * blocks_per_cu / per));
  g.blocks = blocks < 1 ? 1 : blocks;
  return g;
}

// launch_stream's `big`: the cache-resident hot kernels take two tiles per iteration only when there is work for it
inline bool stream_big(int64_t n, int n_cu) { return grid_tiles(n) >= 4 * (int64_t)n_cu; }

// workgroups (256 threads, grid-stride loop) of the one-element-per-lane catch-all kernels
inline int64_t scalar_grid_blocks(int64_t n, int n_cu) {
  return std::min<int64_t>((n + 255) / 256, (int64_t)n_cu * GRID_SCALAR_PER_CU);
}

// does a lone launch of n elements take the fused kernel's shape as a group of one (Tuning::big_tiles; 0: never)?
inline bool lone_takes_fused_shape(int64_t n, int big_tiles) { return big_tiles > 0 && grid_tiles(n) >= big_tiles; }

// workgroups (256 threads, grid-stride loop) of add_noise_kernel and blend_kernel: `vec` = add_noise_kernel<T, true>, one
// 8-element group per lane; else one element per lane
inline int64_t aux_grid_blocks(int64_t n, int n_cu, bool vec) {
  const int64_t blocks = vec ? grid_tiles(n) : (n + 255) / 256;
  return std::min(blocks, (int64_t)n_cu * GRID_SCALAR_PER_CU);
}

}  // namespace

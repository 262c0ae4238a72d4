// dpm_het_shapes.hpp -- the tile space of a mixed-shape heterogeneous launch (stage_kernel_shapes, dpm_shapes_kernel.hpp):
// requests of DIFFERENT element counts share one launch, so a virtual super-tile index no longer finds its request by a
// division.  The plan concatenates the members' super-tiles -- request r owns [first[r], first[r + 1]) -- and the lookup
// finds (request, local super-tile) of a virtual index in that prefix table.
// Plain C++17: the standard library only, nothing of HIP -- so that a host compiler and a CPU test
// (tests/test_het_shapes_host.py) reach it.  The three functions the kernels call as well are qualified by DPM_SHAPES_HD,
// which dpm_shapes_kernel.hpp defines for the device before it includes this file: the mapping tested on the CPU is the
// mapping that runs.
#pragma once
#include <cstdint>

#ifndef DPM_SHAPES_HD
#define DPM_SHAPES_HD inline
#endif

namespace {

constexpr int HET_SHAPES_MAX = 16;          // members of one launch (HET_MAX: the records travel in the kernel's arguments)
constexpr int64_t HET_TILE_GROUPS = 256;    // 8-element groups of a tile: one per lane of a 256-lane group (2048 elements)
constexpr int64_t HET_GROUP_ELEMS = 8;

// super-tiles (u tiles of 2048 elements) of a request of n elements -- fused_grid's `spr`
inline int64_t het_super_tiles(int64_t n, int u) {
  return ((n / HET_GROUP_ELEMS + HET_TILE_GROUPS - 1) / HET_TILE_GROUPS + u - 1) / u;
}

struct HetShapePlan {
  uint32_t count[HET_SHAPES_MAX];      // super-tiles of member r
  uint32_t first[HET_SHAPES_MAX + 1];  // exclusive prefix of count; the entries past n_req repeat the total
  int64_t total;                       // super-tiles of the launch (first[n_req] when it fits)
  bool mixed;                          // at least two members differ in n
  bool fits;                           // 1 <= n_req <= HET_SHAPES_MAX, every n > 0, total below 2^31
};

// the plan of n_req members of n[r] elements at u tiles per super-tile
inline HetShapePlan het_shape_plan(const int64_t* n, int n_req, int u) {
  HetShapePlan pl = {};
  pl.fits = n_req >= 1 && n_req <= HET_SHAPES_MAX && u >= 1;
  for (int r = 0; pl.fits && r < n_req; ++r) {
    const int64_t c = n[r] > 0 ? het_super_tiles(n[r], u) : 0;
    pl.mixed = pl.mixed || n[r] != n[0];
    pl.total += c;
    pl.fits = c > 0 && pl.total < ((int64_t)1 << 31);
    if (pl.fits) {
      pl.count[r] = (uint32_t)c;
      pl.first[r + 1] = (uint32_t)pl.total;
    }
  }
  for (int r = pl.fits ? n_req : 0; r < HET_SHAPES_MAX; ++r) pl.first[r + 1] = pl.fits ? (uint32_t)pl.total : 0u;
  return pl;
}

// fused_grid's XCD span applied to the total: super-tiles per XCD of the XCD-contiguous remap (0: no remap)
inline uint32_t het_xcd_span(int64_t total, bool remap) { return remap ? (uint32_t)((total + 7) / 8) : 0u; }
// ... and its grid: workgroups of `per` 256-lane groups, one super-tile per group
inline int64_t het_grid_blocks(int64_t total, uint32_t span, int per) {
  return span ? 8 * (((int64_t)span + per - 1) / per) : (total + per - 1) / per;
}

// The virtual super-tile of 256-lane group `sub` of workgroup b (per groups per workgroup), or `total` when that group has
// none.  span != 0: workgroup b runs on XCD b % 8 -- every XCD gets one contiguous eighth of the concatenated tile space.
DPM_SHAPES_HD uint32_t het_virtual_tile(uint32_t b, uint32_t sub, uint32_t per, uint32_t span, uint32_t total) {
  const uint32_t in_xcd = (b >> 3) * per + sub;
  if (span && in_xcd >= span) return total;
  const uint32_t v = span ? (b & 7u) * span + in_xcd : b * per + sub;
  return v < total ? v : total;
}

struct HetSlot {
  uint32_t r, local;  // the member and its super-tile that a virtual index names
};
// (request, local super-tile) of virtual super-tile v < first[n_req]: the last member whose first super-tile is not past
// v.  A fixed run of HET_SHAPES_MAX - 1 wave-uniform compares on a table that is loaded once -- no search whose loads
// depend on each other, and no bound by n_req: the entries past it repeat the total (het_shape_plan), which v never reaches.
DPM_SHAPES_HD HetSlot het_shape_find(const uint32_t* first, uint32_t n_req, uint32_t v) {
  (void)n_req;
  uint32_t r = 0, base = first[0];
#if defined(__clang__)
#pragma unroll
#endif
  for (uint32_t i = 1; i < (uint32_t)HET_SHAPES_MAX; ++i) {
    const bool at = v >= first[i];
    r = at ? i : r;
    base = at ? first[i] : base;
  }
  return HetSlot{r, v - base};
}

}  // namespace

// het_shapes_driver.cpp -- stand-alone host program around the mixed-shape launch's tile space (csrc/dpm_het_shapes.hpp),
// built and run by tests/test_het_shapes_host.py.  One case per line of standard input:
//   u n_req n[0] ... n[n_req - 1]
// one line per case on standard output:
//   fits=F mixed=M total=T first=a,b,... walk=r:l,r:l,...  grid=<per><remap>:<blocks>:<verdict> x 4
// walk: the (request, local super-tile) het_shape_find names for v = 0 .. total - 1, in that order.  grid, for 256 and 512
// threads (per = 1, 2) without and with the XCD remap: every workgroup b and 256-lane group sub of the launch's grid goes
// through het_virtual_tile and het_shape_find; the verdict is 1 when every (request, local super-tile) of the plan was visited
// exactly once and nothing outside it.  Plans of more than 2^20 super-tiles are printed without walk and grid.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dpm_het_shapes.hpp"

int main() {
  static char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    char* s = line;
    const int u = (int)std::strtol(s, &s, 10);
    const int n_req = (int)std::strtol(s, &s, 10);
    if (u < 1 || n_req < 0 || n_req > 64) continue;
    std::vector<int64_t> n((size_t)n_req > 0 ? (size_t)n_req : 1, 0);
    for (int r = 0; r < n_req; ++r) n[(size_t)r] = std::strtoll(s, &s, 10);
    const HetShapePlan pl = het_shape_plan(n.data(), n_req, u);
    std::printf("fits=%d mixed=%d total=%" PRId64 " first=", (int)pl.fits, (int)pl.mixed, pl.fits ? pl.total : 0);
    for (int r = 0; r <= HET_SHAPES_MAX; ++r) std::printf("%s%u", r ? "," : "", pl.first[r]);
    std::printf(" walk=");
    if (!pl.fits || pl.total > (1 << 20)) {  // no plan, or a plan too large to walk here
      std::printf("- grid=-\n");
      continue;
    }
    const uint32_t total = (uint32_t)pl.total;
    for (uint32_t v = 0; v < total; ++v) {
      const HetSlot t = het_shape_find(pl.first, (uint32_t)n_req, v);
      std::printf("%s%u:%u", v ? "," : "", t.r, t.local);
    }
    std::printf(" grid=");
    for (int per = 1; per <= 2; ++per)
      for (int remap = 0; remap <= 1; ++remap) {
        const uint32_t span = het_xcd_span(pl.total, remap != 0);
        const int64_t blocks = het_grid_blocks(pl.total, span, per);
        std::vector<std::vector<int>> seen((size_t)n_req);
        for (int r = 0; r < n_req; ++r) seen[(size_t)r].assign(pl.count[r], 0);
        bool ok = true;
        for (int64_t b = 0; b < blocks; ++b)
          for (int sub = 0; sub < per; ++sub) {
            const uint32_t v = het_virtual_tile((uint32_t)b, (uint32_t)sub, (uint32_t)per, span, total);
            if (v >= total) {
              ok = ok && v == total;
              continue;
            }
            const HetSlot t = het_shape_find(pl.first, (uint32_t)n_req, v);
            if (t.r >= (uint32_t)n_req || t.local >= pl.count[t.r]) {
              ok = false;
              continue;
            }
            seen[t.r][t.local] += 1;
          }
        for (int r = 0; r < n_req; ++r)
          for (int c : seen[(size_t)r]) ok = ok && c == 1;
        std::printf("%s%d%d:%" PRId64 ":%d", per + remap > 1 ? "," : "", per, remap, blocks, (int)ok);
      }
    std::printf("\n");
  }
  return 0;
}

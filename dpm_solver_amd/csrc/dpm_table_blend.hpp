// dpm_table_blend.hpp -- mask-blend rows of the table-driven launch (DPM_TABLE_BLEND): stage_kernel_table_blend, its record
// and its launcher (part of dpm_device.hpp; include that)
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// An inpainting / DiffEdit request carries DPM_F_BLEND on every stage that emits a state, and fusable_request turns the blend
// away: in a pool such a request was its own dpm_stage_launch per tick.  The kernarg records have no room for three more
// pointers and two scalars per request; a table has -- a third record kind behind the rows (after the noise records of a
// DPM_TABLE_NOISE call), record i beside row i, reached through a second const __restrict__ kernel-argument pointer with the
// same wave-uniform r: scalar loads, like the row and like stage_kernel_table_noise's KNoiseTab.  The kernel is
// stage_kernel_table over the form set {LIN1, TWO, MS3} with EXT = true: the tile body's own blend epilogue, the bits of the
// request's dpm_stage_launch.
// The record's pointers are declared in the global address space, as TableRow's are and for the same reason: KExt's are plain
// `const void*`, and a plain pointer loaded from global memory would make the mask / known-image / noise loads flat_load.
// The cast to KExt's type happens in the kernel, where the optimiser sees the address space behind it.
// The tile layout is the row's: stage_tiles takes the split layout (4-byte states) when the mask period is a whole number
// of 2048-element tiles (can_split) -- computed from the record's period, wave-uniform, so one launch holds rows that split
// next to rows that do not.
// ------------------------------------------------------------------------------------------------
struct alignas(16) KBlendTab {
  const DPM_GLOBAL_PTR void* mask;
  const DPM_GLOBAL_PTR void* ba;
  const DPM_GLOBAL_PTR void* bb;  // null: ba is blended in as it is
  int64_t mask_period;            // elements
  float alpha, sigma;             // dpm_stage.blend_alpha / blend_sigma
  uint32_t pad[2];                // (zero)
};
static_assert(sizeof(KBlendTab) == DPM_TABLE_BLEND_BYTES && alignof(KBlendTab) == 16,
              "include/dpm_hip.h publishes the blend record's size: 3 pointers, the period, 2 scalars, 2 zero words");

template <typename TS, typename TE, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_table_blend(const TableRow* __restrict__ rows,
                                                                              const KBlendTab* __restrict__ bls, int64_t n,
                                                                              uint32_t nreq, uint32_t spr, uint32_t xcd_span) {
  static_assert(GUIDE != DPM_GUIDE_CLASSIFIER, "a table row: no classifier guidance");
  const int64_t ngroups = n / EPT;
  const uint32_t total = nreq * spr;
  const uint32_t per = blockDim.x >> 8;
  const uint32_t sub = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const uint32_t b = blockIdx.x;
  const uint32_t in_xcd = (b >> 3) * per + sub;
  if (xcd_span && in_xcd >= xcd_span) return;
  const uint32_t v = xcd_span ? (b & 7u) * xcd_span + in_xcd : b * per + sub;
  if (v >= total) return;
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v / spr));
  const int64_t t0 = (int64_t)(v - r * spr) * U;
  const TableRow& row = rows[r];
  const KBlendTab& bl = bls[r];
  const KParams& p = row.p;
  KExt ext = {};
  if constexpr (GUIDE == DPM_GUIDE_CFG) ext.xo2 = (void*)row.xo2;
  ext.mask = (const void*)bl.mask;
  ext.ba = (const void*)bl.ba;
  ext.bb = (const void*)bl.bb;
  ext.mask_period = bl.mask_period;
  ext.blend_alpha = bl.alpha;
  ext.blend_sigma = bl.sigma;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
#define DPM_TABLE_TILES(F_) \
  stage_tiles<TS, TE, F_, GUIDE, false, SPEC, U, NT, true>(x, nullptr, e0, e1, nullptr, h1, h2, xo, mo, ngroups, t0, p, ext)
  switch (p.form) {
    case DPM_FORM_LIN1: DPM_TABLE_TILES(DPM_FORM_LIN1); break;
    case DPM_FORM_TWO: DPM_TABLE_TILES(DPM_FORM_TWO); break;
    case DPM_FORM_MS3: DPM_TABLE_TILES(DPM_FORM_MS3); break;
    default: break;  // (the host groups LIN1 / TWO / MS3 only)
  }
#undef DPM_TABLE_TILES
}

// may a DPM_F_BLEND request own a table row (DPM_TABLE_BLEND)?  fusable_request on the stage without the blend bit (guidance
// none or CFG, a plain dense request of whole 8-element groups, aligned buffers, x_out2 only under CFG; the caller's pair_of:
// 2- and 4-byte pairs), one of the kernel's three forms, no noise behind the blend and no thresholding (neither epilogue is in
// this kernel), the three blend tensors aligned for 16-byte accesses, and a mask period of whole 8-element groups that divides n
// -- the vector path's index is gi % (mask_period / 8).
inline bool blend_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_BLEND) || (st.flags & (DPM_F_NOISE | DPM_F_THRESH))) return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3) return false;
  dpm_stage plain = st;
  plain.flags &= ~(uint32_t)DPM_F_BLEND;
  if (!fusable_request(plain, b)) return false;
  if (!b.mask || !b.blend_a || !aligned(b.mask, 16) || !aligned(b.blend_a, 16) || !aligned(b.blend_b, 16)) return false;
  return b.mask_period >= EPT && b.mask_period % EPT == 0 && b.n % b.mask_period == 0;
}

// ---- DPM_TABLE_FILL | DPM_TABLE_BLEND: the blend records of one group of blend rows, beside its rows (same order).  Host memory,
// no HIP call.
inline void table_fill_blend(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* recs) {
  KBlendTab* out = static_cast<KBlendTab*>(recs);
  for (int r = 0; r < n_req; ++r) {
    KBlendTab bl;
    std::memset(&bl, 0, sizeof bl);
    const void* const ptrs[3] = {bs[r].mask, bs[r].blend_a, bs[r].blend_b};
    static_assert(offsetof(KBlendTab, mask_period) == sizeof ptrs, "a blend record starts with its 3 pointers");
    std::memcpy(&bl, ptrs, sizeof ptrs);
    bl.mask_period = bs[r].mask_period;
    bl.alpha = st[r].blend_alpha;
    bl.sigma = st[r].blend_sigma;
    std::memcpy(&out[r], &bl, sizeof bl);
  }
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_BLEND: ONE launch over a group of blend rows and their records (device memory)
template <typename TS, typename TE>
int launch_table_blend_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs,
                             const LaunchCtx& c) {
  constexpr int U = TableShape<TS, TE>::U, NT = TableShape<TS, TE>::NT;
  const TableRow* tab = static_cast<const TableRow*>(rows);
  const KBlendTab* bls = static_cast<const KBlendTab*>(recs);
  const int64_t n = bs[0].n;
  const uint32_t nreq = (uint32_t)n_req;
  return launch_table_rows<TS, TE>(
      st, bs, n_req, "stage_launch_multi: a stage that is no blend row of this group in a table blend launch",
      "table blend stage kernel launch failed", [&](int r) { return blend_row_ok(st[r], bs[r]) && bs[r].n == bs[0].n; },
      [&](auto x0_, auto cfg_, const FusedShape& sh) {
        launch(stage_kernel_table_blend<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, tab, bls, n, nreq,
               sh.spr, sh.xcd_span);
      });
}

}  // namespace

// dpm_shapes_kernel.hpp -- the mixed-shape heterogeneous fused stage (dpm_launch_opts.fuse_shapes): the siblings of
// stage_kernel_het / _het_noise / _het_unipc for groups whose members differ in element count, and their launcher
// (part of dpm_device.hpp; include that)
#pragma once

#define DPM_SHAPES_HD __host__ __device__ __forceinline__
#include "dpm_het_shapes.hpp"

namespace {

static_assert(HET_SHAPES_MAX == HET_MAX && HET_GROUP_ELEMS == EPT, "dpm_het_shapes.hpp restates the het launch's constants");

// ------------------------------------------------------------------------------------------------
// A server's requests differ in latent size and images per prompt; the heterogeneous kernels find a request by v / spr, one
// element count for the whole launch.  Here the virtual super-tile index runs over the CONCATENATED super-tiles of the
// members (dpm_het_shapes.hpp: request r owns [first[r], first[r + 1])), and request r brings its own ngroups.  Everything
// else is stage_kernel_het's: whole KParams records read in place through the kernarg segment pointer (scalar loads with
// the wave-uniform r), one super-tile per 256-lane group, no loop, MultiShape's tiles and cache policy, the XCD-contiguous
// remap -- applied to the concatenated space, so an XCD's eighth may span several requests.  The tile body is stage_tiles,
// called with the request's own ngroups and local tile: every request gets the bits of its own single launch, and the
// noise contract (z from seed, stage index and element index) holds as it stands.
// A struct of its own (see HetNoiseArgs on why HetArgs gains no field).
// ------------------------------------------------------------------------------------------------
struct HetShapeArgs {
  const void* x[HET_MAX];
  const void* e0[HET_MAX];
  const void* e1[HET_MAX];
  const void* h1[HET_MAX];
  const void* h2[HET_MAX];
  void* xo[HET_MAX];
  void* mo[HET_MAX];
  void* xo2[HET_MAX];
  KParams p[HET_MAX];
  int64_t ngroups[HET_MAX];     // request r's 8-element groups (n / 8)
  uint32_t first[HET_MAX + 1];  // request r's first virtual super-tile; the entries past nreq repeat the total
  uint32_t nreq, total;         // total = first[nreq]
  uint32_t xcd_span;            // != 0: XCD-contiguous remap of the concatenated tile space
};
struct HetShapeNoiseArgs {
  HetShapeArgs h;
  KNoise nz[HET_MAX];
};
static_assert(sizeof(HetShapeNoiseArgs) <= 4096, "the mixed-shape launch's argument block must fit HIP's 4 KiB");
constexpr unsigned HET_FORMS_UNIPC = HET_FORMS_2 | (1u << DPM_FORM_UNIPC);
// stage_tiles reads bits 0-3 of its nt mask.  Bit 4 means nothing to it and gives these kernels instantiations of the tile
// body of their own: sharing stage_kernel_het's, the 4-byte-state stage_kernel_het / _het_noise / _het_unipc kernels came out
// with other listings (the force-inlined body is placed differently once it has more callers), and a uniform pool is to keep
// the code it was measured with.
constexpr int NT_SHAPES = 16;

// the body of the three kernels: `a` and `nzs` point into the kernarg segment
template <typename TS, typename TE, unsigned FORMS, int GUIDE, int SPEC, int U, int NT, bool NOISE>
__device__ __forceinline__ void shapes_body(const HetShapeArgs& a, const KNoise* nzs) {
  const uint32_t per = blockDim.x >> 8;
  const uint32_t sub = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const uint32_t v = het_virtual_tile(blockIdx.x, sub, per, a.xcd_span, a.total);
  if (v >= a.total) return;
  const HetSlot slot = het_shape_find(a.first, a.nreq, v);
  const uint32_t r = slot.r;
  const int64_t t0 = (int64_t)slot.local * U;
  const int64_t ngroups = a.ngroups[r];
  const KParams& p = a.p[r];
  const KNoise* nz = NOISE ? nzs + r : nullptr;
  constexpr bool DUP = GUIDE == DPM_GUIDE_CFG;
  KExt ext = {};
  if constexpr (DUP) ext.xo2 = a.xo2[r];
  const TS* x = static_cast<const TS*>(a.x[r]);
  const TE* e0 = static_cast<const TE*>(a.e0[r]);
  const TE* e1 = static_cast<const TE*>(a.e1[r]);
  const TS* h1 = static_cast<const TS*>(a.h1[r]);
  const TS* h2 = static_cast<const TS*>(a.h2[r]);
  TS* xo = static_cast<TS*>(a.xo[r]);
  TS* mo = static_cast<TS*>(a.mo[r]);
#define DPM_SHAPES_TILES(F_)                                                                                                  \
  stage_tiles<TS, TE, F_, GUIDE, false, SPEC, U, NT, DUP, false, NOISE>(x, nullptr, e0, e1, nullptr, h1, h2, xo, mo, ngroups, t0, \
                                                                        p, ext, nullptr, nz)
  switch (p.form) {
    case DPM_FORM_LIN1: DPM_SHAPES_TILES(DPM_FORM_LIN1); break;
    case DPM_FORM_TWO: DPM_SHAPES_TILES(DPM_FORM_TWO); break;
    case DPM_FORM_MS3:
      if constexpr ((FORMS >> DPM_FORM_MS3) & 1u) DPM_SHAPES_TILES(DPM_FORM_MS3);
      break;
    case DPM_FORM_UNIPC:
      if constexpr ((FORMS >> DPM_FORM_UNIPC) & 1u) DPM_SHAPES_TILES(DPM_FORM_UNIPC);
      break;
    default: break;  // (the host groups only forms of FORMS)
  }
#undef DPM_SHAPES_TILES
}

// ODE stages: FORMS = HET_FORMS_2 or HET_FORMS_3, as stage_kernel_het
template <typename TS, typename TE, unsigned FORMS, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_shapes(const HetShapeArgs args) {
  (void)args;
  shapes_body<TS, TE, FORMS, GUIDE, SPEC, U, NT, false>(*(const HetShapeArgs*)__builtin_amdgcn_kernarg_segment_ptr(), nullptr);
}

// SDE stages (DPM_F_NOISE; LIN1 / TWO): a whole KNoise per request, as stage_kernel_het_noise
template <typename TS, typename TE, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_shapes_noise(const HetShapeNoiseArgs args) {
  static_assert(GUIDE != DPM_GUIDE_CLASSIFIER, "noise: no classifier guidance");
  (void)args;
  const HetShapeNoiseArgs& an = *(const HetShapeNoiseArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  shapes_body<TS, TE, HET_FORMS_2, GUIDE, SPEC, U, NT, true>(an.h, an.nz);
}

// UniPC stages next to first- and second-order ones: {LIN1, TWO, UNIPC}, as stage_kernel_het_unipc
template <typename TS, typename TE, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_shapes_unipc(const HetShapeArgs args) {
  static_assert(GUIDE != DPM_GUIDE_CLASSIFIER, "unipc: no classifier guidance");
  (void)args;
  shapes_body<TS, TE, HET_FORMS_UNIPC, GUIDE, SPEC, U, NT, false>(*(const HetShapeArgs*)__builtin_amdgcn_kernarg_segment_ptr(),
                                                                  nullptr);
}

// ---- the launcher.  The caller (dpm_kernels.hip, under dpm_launch_opts.fuse_shapes) has grouped the requests as for
// launch_het_typed, except that they need not agree on n and batch, and sends only groups with at least two different n.
// MULTI_NOT_BUILT (no error set): the group's super-tile total does not fit 31 bits -- the caller launches its members one
// by one.
template <typename TS, typename TE>
int launch_het_shapes_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const LaunchCtx& c) {
  if (n_req < 1 || n_req > HET_MAX)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one fused launch", n_req);
  const Tuning tn = tuning_for(bs[0].opts);
  constexpr int U = MultiShape<TS, TE>::U, NT = MultiShape<TS, TE>::NT | NT_SHAPES;
  int64_t ns[HET_MAX];
  for (int r = 0; r < n_req; ++r) ns[r] = bs[r].n;
  const HetShapePlan pl = het_shape_plan(ns, n_req, U);
  if (!pl.fits) return MULTI_NOT_BUILT;
  HetShapeNoiseArgs an;  // (the ODE kernels take its first member)
  std::memset(&an, 0, sizeof an);
  HetShapeArgs& a = an.h;
  bool ms3 = false, unipc = false;
  const bool sde = (st[0].flags & DPM_F_NOISE) != 0;
  bool x0 = !tn.force_generic;
  for (int r = 0; r < n_req; ++r) {
    fill_request(a, r, bs[r]);
    a.xo2[r] = bs[r].x_out2;
    a.p[r] = make_params(&st[r]);
    a.ngroups[r] = bs[r].n / EPT;
    if (sde) an.nz[r] = noise_of(st[r], bs[r]);
    ms3 = ms3 || st[r].form == DPM_FORM_MS3;
    unipc = unipc || st[r].form == DPM_FORM_UNIPC;
    x0 = x0 && x0_prologue_ok(st[r]);
  }
  if (unipc && (ms3 || sde))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a UniPC stage grouped with a third-order or an SDE stage");
  std::memcpy(a.first, pl.first, sizeof a.first);
  a.nreq = (uint32_t)n_req;
  a.total = (uint32_t)pl.total;
  // fused_grid's shape on the concatenated tile space
  const int bt = tn.block_threads > 0 ? tn.block_threads : MultiShape<TS, TE>::THREADS;
  const bool remap = tn.multi_xcd_remap < 0 ? sizeof(TS) == 2 : tn.multi_xcd_remap != 0;
  a.xcd_span = het_xcd_span(pl.total, remap);
  const dim3 grid((unsigned)het_grid_blocks(pl.total, a.xcd_span, bt / 256)), block((unsigned)bt);
  const bool cfg = st[0].guidance == DPM_GUIDE_CFG;
  if (sde) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_shapes_noise<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, grid, block, 0, c, an);
    });
  } else if (unipc) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_shapes_unipc<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, grid, block, 0, c, a);
    });
  } else if (ms3) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_shapes<TS, TE, HET_FORMS_3, guide_of(cfg_), spec_of(x0_), U, NT>, grid, block, 0, c, a);
    });
  } else {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_shapes<TS, TE, HET_FORMS_2, guide_of(cfg_), spec_of(x0_), U, NT>, grid, block, 0, c, a);
    });
  }
  return launch_status("fused mixed-shape stage kernel launch failed");
}

}  // namespace

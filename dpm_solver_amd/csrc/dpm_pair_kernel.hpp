// dpm_pair_kernel.hpp -- guidance over TWO conditions (DPM_GUIDE_CFG2, include/dpm_hip.h): stage_pair_kernel, a streaming stage
// kernel that blends THREE network outputs -- e0 under the first condition, e1 unconditional, g under the second condition --
// and its launcher.  Included by unit H of dpm_stage_unit.hip behind dpm_device.hpp and by nothing else, so that every other
// unit compiles to the code it compiled to.
//
//   n_k = noise prediction of the raw output o_k;  d0 = n0 - n1;  d2 = n2 - n1;  eps = (n1 + s1 * d0) + s2 * d2
// in fp32 on the exactly widened outputs, one rounding per operation (s1 = cfg_scale, s2 = cg_scale), then the stage proper --
// eps -> x0, the update form, the stores -- as under any other guidance.  Nothing is rounded to the network's dtype and the
// model values are never half: combine() runs with hm = false.
// Form, model type and prologue are read from the stage record at run time (FORM_RT, PM_RT): one instantiation per dtype pair.
//   16-byte route  2048-element tiles, one 8-element group per lane (load_pack / store_pack), the tile walk and the grid of the
//                  streaming family (stream_grid_plan at one tile per iteration): n a multiple of 8, every operand 16-byte aligned
//   scalar route   one element per lane, a grid-stride loop over the catch-all kernels' grid (scalar_grid_blocks)
// The three outputs are read once and by nothing else: non-temporal loads.  The state, the evaluation state and the cached model
// values are loaded non-temporally too: that is the streaming family's own policy -- stage_tiles gives EVERY read stream bit 0 of
// its nt mask, and the mask of a lone launch whose inputs come from HBM sets it (dpm_launch.hpp, DefNT: a network ran since the
// previous stage wrote them, so they are no longer cached; [256,4,64,64] 8.4 against 9.3 us fp16, 15.3 against 16.3-16.5 us
// fp32).  Every launch of this kernel follows a network call on three copies of the state.  The stores follow the family per state
// width: a 2-byte state leaves written through, a 4-byte state's 32 bytes per lane are two instructions that each fill every
// other 16 bytes and stay cached stores that L2 merges (dpm_access.hpp: store_pack).
#pragma once

namespace {

// the guided noise prediction of one element's three raw outputs, then eps -> x0 where the stage converts
__device__ __forceinline__ float pair_model(float o0, float o1, float o2, float xev, const KParams& p) {
  const float n0 = to_noise<PM_RT>(o0, xev, p), n1 = to_noise<PM_RT>(o1, xev, p), n2 = to_noise<PM_RT>(o2, xev, p);
  const float d0 = n0 - n1;
  const float d2 = n2 - n1;
  const float eps = (n1 + p.cfg_scale * d0) + p.cg_scale * d2;
  if (p.flags & DPM_F_TO_X0) return div_uniform(xev - p.sigma_e * eps, p.alpha_e, p.inv_alpha, (p.fastdiv & 1u) != 0u);
  return eps;
}

// x: the state the update starts from (the evaluation state where the form reads none), xe: the state the network saw (= x when
// there is no separate one); h1 / h2 / mo may be null where the stage does not name them.  `vec`: the 16-byte route.
template <typename TS, typename TE>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_pair_kernel(const TS* __restrict__ x, const TS* __restrict__ xe,
                                                                       const TE* __restrict__ e0, const TE* __restrict__ e1,
                                                                       const TE* __restrict__ e2, const TS* __restrict__ h1,
                                                                       const TS* __restrict__ h2, TS* __restrict__ xo,
                                                                       TS* __restrict__ mo, int64_t n, const KParams p, int vec) {
  const bool need_xe = (p.flags & DPM_F_TO_X0) || p.model_type == DPM_MODEL_X_START || p.model_type == DPM_MODEL_V;
  const bool nx = form_needs_x<FORM_RT>(p), nh1 = form_needs_h1<FORM_RT>(p), nh2 = form_needs_h2<FORM_RT>(p);
  const bool sep = xe != x;  // a separate evaluation state (singlestep mid-stages)
  const bool store_m = (p.flags & DPM_F_STORE_M) != 0;
  if (vec) {
    const int64_t ngroups = n / EPT;
    const int64_t ntiles = (ngroups + 255) / 256;
    const uint32_t per = blockDim.x >> 8;                                                    // 256-lane groups per workgroup
    const uint32_t sub = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));  // this wavefront's (wave-uniform)
    for (int64_t t = (int64_t)blockIdx.x * per + sub; t < ntiles; t += (int64_t)gridDim.x * per) {
      // lanes past the end of the last tile load a clamped (valid) group and only skip the stores
      const int64_t gr = t * 256 + tile_lane();
      const int64_t gi = gr < ngroups ? gr : ngroups - 1;
      float vx[EPT], vxe[EPT], v0[EPT], v1[EPT], v2[EPT], vh1[EPT], vh2[EPT], ox[EPT], om[EPT];
      // (The conditional loads convert where they load, so each is followed by a wait before the next is issued.  Two other
      // bodies were built and timed on an MI355X -- raw loads converted after the last one is issued, and the mode and form
      // switches once per tile instead of once per element -- and neither was faster: profiles/r30_cfg_pair.md, section 2.)
      const bool ld_x = nx || (need_xe && !sep);
      if (ld_x) load_pack<true>(x, gi, vx);
      if (need_xe && sep) load_pack<true>(xe, gi, vxe);
      load_pack<true>(e0, gi, v0);
      load_pack<true>(e1, gi, v1);
      load_pack<true>(e2, gi, v2);
      if (nh1) load_pack<true>(h1, gi, vh1);
      if (nh2) load_pack<true>(h2, gi, vh2);
#pragma unroll
      for (int j = 0; j < EPT; ++j) {
        const float xv = ld_x ? vx[j] : 0.f;
        const float xev = need_xe ? (sep ? vxe[j] : xv) : 0.f;
        const float mn = pair_model(v0[j], v1[j], v2[j], xev, p);
        om[j] = mn;
        ox[j] = combine_any<FORM_RT, float, TE>(nx ? xv : 0.f, mn, nh1 ? vh1[j] : 0.f, nh2 ? vh2[j] : 0.f, p, false);
      }
      if (gr < ngroups) {
        store_pack<false, true>(xo, gi, ox);
        if (store_m) store_pack<false, true>(mo, gi, om);
      }
    }
  } else {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float xv = (nx || (need_xe && !sep)) ? to_f32(x[i]) : 0.f;
      const float xev = need_xe ? (sep ? to_f32(xe[i]) : xv) : 0.f;
      const float mn = pair_model(to_f32(e0[i]), to_f32(e1[i]), to_f32(e2[i]), xev, p);
      xo[i] = from_f32<TS>(combine_any<FORM_RT, float, TE>(nx ? xv : 0.f, mn, nh1 ? to_f32(h1[i]) : 0.f,
                                                            nh2 ? to_f32(h2[i]) : 0.f, p, false));
      if (store_m) mo[i] = from_f32<TS>(mn);
    }
  }
}

// this unit's launch of one DPM_GUIDE_CFG2 stage (checked by dpm_stage_launch: check_pair_guidance, dpm_kernels.hip)
template <typename TS, typename TE>
int launch_pair_typed(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& c) {
  const Operands<TS, TE> op(st, b);
  const bool vec = b->n % EPT == 0 && op.aligned_to(16, 16);
  if (vec) {
    const Shape sh = stream_grid(b->n, 1, op.n_cu, tuning_for(b->opts));
    launch(stage_pair_kernel<TS, TE>, sh.grid, sh.block, 0, c, op.x, op.xe ? op.xe : op.x, op.e0, op.e1, op.g, op.h1, op.h2, op.xo,
           op.mo, b->n, op.p, 1);
  } else {
    launch(stage_pair_kernel<TS, TE>, scalar_grid(b->n, op.n_cu), dim3(256), 0, c, op.x, op.xe ? op.xe : op.x, op.e0, op.e1, op.g,
           op.h1, op.h2, op.xo, op.mo, b->n, op.p, 0);
  }
  return launch_status("two-condition stage kernel launch failed");
}

}  // namespace

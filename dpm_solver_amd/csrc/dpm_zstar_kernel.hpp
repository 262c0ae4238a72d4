// dpm_zstar_kernel.hpp -- classifier-free guidance with the CFG-Zero* projection (DPM_F_CFG_ZSTAR, include/dpm_hip.h; Fan et al.
// 2025, "CFG-Zero*: Improved Classifier-Free Guidance for Flow Matching Models"): stage_zstar_kernel, a stage kernel that owns
// a whole SAMPLE, and its launcher.  Included by unit G of dpm_stage_unit.hip behind dpm_sample_frame.hpp -- the workgroup, the
// lane-to-element map, the masked loads and stores, the reduction, the two access paths -- and by nothing else, so that every
// other unit compiles to the code it compiled to.
//
// Before the blend the unconditional output is scaled by its least-squares fit to the conditional one over the sample.  One
// workgroup per sample, grid = batch:
//   pass 1   the sample's two raw outputs -> two sums in double per thread, <o_c, o_u> and <o_u, o_u> (products of fp32 values
//            are exact in double), reduced (sf_reduce); every thread then forms the same a = S_cu / (S_uu + 1e-8)
//   pass 2   u = a * o_u, g = u + s * (o_c - u), then the stage proper -- conversion, eps -> x0, update form, stores -- on the
//            sample
// Form, model type and prologue are read from the stage record (FORM_RT, PM_RT): one instantiation per dtype pair.
//   register path  the two outputs stay in registers between the passes (non-temporal loads: nothing reads them again)
//   re-read path   pass 2 reads the outputs again, so pass 1 loads them with the default cache policy and the second read
//                  comes from L2
// The kernel carries no parameter of its own (cfg_scale is the flag-less blend's) and no state from stage to stage.
#pragma once

namespace {

// the two sums of one iteration's elements: S_cu (acc[0]) and S_uu (acc[1]).  A masked element adds an exact zero.
template <bool VEC>
__device__ __forceinline__ void zstar_accumulate(const float (&vc)[EPT], const float (&vu)[EPT], int64_t k, int64_t per,
                                                 double (&acc)[2]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const bool valid = sf_index<VEC>(k, j) < per;
    const double c = valid ? (double)vc[j] : 0.0;
    const double u = valid ? (double)vu[j] : 0.0;
    acc[0] += c * u;
    acc[1] += u * u;
  }
}

// pass 2 on one iteration: the guided raw output, the conversion, eps -> x0, the update form, the stores
template <bool VEC, typename TS, typename TE>
__device__ __forceinline__ void zstar_update(const float (&vc)[EPT], const float (&vu)[EPT], const TS* __restrict__ x,
                                             const TS* __restrict__ xe, const TS* __restrict__ h1, const TS* __restrict__ h2,
                                             TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__ xo2, int64_t k, int64_t per,
                                             float a, const KParams& p) {
  const bool need_xe = (p.flags & DPM_F_TO_X0) || p.model_type == DPM_MODEL_X_START || p.model_type == DPM_MODEL_V;
  const bool nx = form_needs_x<FORM_RT>(p), nh1 = form_needs_h1<FORM_RT>(p), nh2 = form_needs_h2<FORM_RT>(p);
  const bool sep = xe != x;  // a separate evaluation state (singlestep mid-stages)
  float vx[EPT], vxe[EPT], vh1[EPT], vh2[EPT], ox[EPT], om[EPT];
  if (nx || (need_xe && !sep)) sf_load<VEC, true>(x, k, per, vx);
  if (need_xe && sep) sf_load<VEC, true>(xe, k, per, vxe);
  if (nh1) sf_load<VEC, true>(h1, k, per, vh1);
  if (nh2) sf_load<VEC, true>(h2, k, per, vh2);
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const float xv = (nx || (need_xe && !sep)) ? vx[j] : 0.f;
    const float xev = need_xe ? (sep ? vxe[j] : xv) : 0.f;
    // (the guided output is an fp32 tensor whatever the network's dtype: nothing here is a half operation)
    const float u = a * vu[j];
    const float g = u + p.cfg_scale * (vc[j] - u);
    const float eps = to_noise<PM_RT>(g, xev, p);
    const float mn = (p.flags & DPM_F_TO_X0) ? div_uniform(xev - p.sigma_e * eps, p.alpha_e, p.inv_alpha, (p.fastdiv & 1u) != 0u) : eps;
    om[j] = mn;
    ox[j] = combine_any<FORM_RT, float, TE>(nx ? xv : 0.f, mn, nh1 ? vh1[j] : 0.f, nh2 ? vh2[j] : 0.f, p, false);
  }
  sf_store<VEC>(xo, k, per, ox);
  if (xo2) sf_store<VEC>(xo2, k, per, ox);
  if (p.flags & DPM_F_STORE_M) sf_store<VEC>(mo, k, per, om);
}

// one sample, both passes.  KEEP: the register path (per <= SF_KEEP_MAX).  Called by every thread of the workgroup with
// workgroup-uniform template arguments: the barrier inside is reached by all of them.
template <bool VEC, bool KEEP, typename TS, typename TE>
__device__ __forceinline__ void zstar_sample(const TS* __restrict__ x, const TS* __restrict__ xe, const TE* __restrict__ e0,
                                             const TE* __restrict__ e1, const TS* __restrict__ h1, const TS* __restrict__ h2,
                                             TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__ xo2, int64_t per,
                                             const KParams& p, double* red) {
  const int64_t nchunks = (per + SF_CHUNK - 1) / SF_CHUNK;
  double acc[2] = {0.0, 0.0};
  float kc[KEEP ? SF_KEEP_CHUNKS : 1][EPT], ku[KEEP ? SF_KEEP_CHUNKS : 1][EPT];
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k) {  // every load of the sample's outputs in flight before the first use
      sf_load<VEC, true>(e0, k, per, kc[k]);
      sf_load<VEC, true>(e1, k, per, ku[k]);
    }
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k) zstar_accumulate<VEC>(kc[k], ku[k], k, per, acc);
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, false>(e0, k, per, kc[0]);  // default cache policy: pass 2 reads these lines again
      sf_load<VEC, false>(e1, k, per, ku[0]);
      zstar_accumulate<VEC>(kc[0], ku[0], k, per, acc);
    }
  }
  double s[2];  // every thread holds the same sums, hence the same a
  sf_reduce(acc, red, s);
  // (S_uu == 0: every o_u is zero, so is S_cu, and a = 0 / 1e-8 = 0 -- g = s * o_c)
  const float a = (float)(s[0] / (s[1] + 1e-8));
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k)
      if ((int64_t)k < nchunks) zstar_update<VEC, TS, TE>(kc[k], ku[k], x, xe, h1, h2, xo, mo, xo2, k, per, a, p);
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, true>(e0, k, per, kc[0]);
      sf_load<VEC, true>(e1, k, per, ku[0]);
      zstar_update<VEC, TS, TE>(kc[0], ku[0], x, xe, h1, h2, xo, mo, xo2, k, per, a, p);
    }
  }
}

// x: the state the update starts from (the evaluation state where the form reads none), xe: the state the network saw (= x when
// there is no separate one); h1 / h2 / mo / xo2 may be null where the stage does not name them.  `vec`: 16-byte accesses.
template <typename TS, typename TE>
__global__ __launch_bounds__(SF_THREADS) void stage_zstar_kernel(const TS* __restrict__ x, const TS* __restrict__ xe,
                                                                 const TE* __restrict__ e0, const TE* __restrict__ e1,
                                                                 const TS* __restrict__ h1, const TS* __restrict__ h2,
                                                                 TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__ xo2,
                                                                 int64_t per, const KParams p, int vec) {
  __shared__ double red[SF_WAVES * 2];
  const int64_t base = (int64_t)blockIdx.x * per;  // this workgroup's sample
  if (x) x += base;
  if (xe) xe += base;
  e0 += base;
  e1 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  if (xo2) xo2 += base;
  const bool keep = per <= SF_KEEP_MAX;
  if (vec) {
    if (keep) zstar_sample<true, true>(x, xe, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
    else zstar_sample<true, false>(x, xe, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
  } else {
    if (keep) zstar_sample<false, true>(x, xe, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
    else zstar_sample<false, false>(x, xe, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
  }
}

// this unit's launch of one flagged stage (checked by dpm_stage_launch: kSampleGuidance, dpm_kernels.hip)
template <typename TS, typename TE>
int launch_sample_typed(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& c) {
  return launch_sample_stage<TS, TE>(stage_zstar_kernel<TS, TE>, "DPM_F_CFG_ZSTAR", "CFG-Zero* stage kernel launch failed", st, b, c,
                                     nullptr);
}

}  // namespace

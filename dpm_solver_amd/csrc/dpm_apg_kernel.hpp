// dpm_apg_kernel.hpp -- classifier-free guidance with adaptive projected guidance (DPM_F_CFG_APG, include/dpm_hip.h; Sadat et
// al. 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models"): stage_apg_kernel, a stage
// kernel that owns a whole SAMPLE, and its launcher.  Included by unit F of dpm_stage_unit.hip behind dpm_sample_frame.hpp --
// the workgroup, the lane-to-element map, the masked loads and stores, the reduction, the two access paths -- and by nothing
// else, so that every other unit compiles to the code it compiled to.
//
// APG works on the DATA predictions: c, u = x0 of the conditional / unconditional output, d = c - u the guidance direction.
// One workgroup per sample, grid = batch:
//   pass 1   the sample's two raw outputs and the state the network saw -> c and d; with a momentum the running average of d is
//            read, updated and stored in place and takes d's place; three sums in double per thread (d.d, d.c, c.c), reduced
//            (sf_reduce); every thread then forms the same two scalars: sc, the norm clamp of d, and q, its projection
//            coefficient on c
//   pass 2   dn = sc*d, par = q*c, upd = (dn - par) + eta*par, mn = c + (s - 1)*upd, then the update form and the stores
// Form and model type are read from the stage record (FORM_RT, PM_RT): one instantiation per dtype pair.
//   register path  c and d -- 32 elements per thread each -- stay in registers between the passes; pass 2 loads x, h1 and
//                  h2 only
//   re-read path   pass 2 recomputes c and d from the operands read again (L2), or, with a momentum, c from the conditional
//                  output and the state and d from the average pass 1 stored (the same thread wrote it)
#pragma once

namespace {

struct ApgScalars {
  float eta, r, beta;  // dpm_stage.cg_scale / thr_ratio / thr_max under DPM_F_CFG_APG
};

// x0 of one raw output on the evaluation state: operation for operation the model value of a flag-less data-prediction stage
__device__ __forceinline__ float apg_x0(float o, float xev, const KParams& p) {
  const float eps = to_noise<PM_RT>(o, xev, p);
  return div_uniform(xev - p.sigma_e * eps, p.alpha_e, p.inv_alpha, (p.fastdiv & 1u) != 0u);
}

// c and d of one iteration from its operands; MOM: `va` is the running average, updated in place and taking d's place
template <bool MOM>
__device__ __forceinline__ void apg_direction(const float (&vc)[EPT], const float (&vu)[EPT], const float (&vxe)[EPT],
                                              float (&va)[EPT], const KParams& p, float beta, float (&c)[EPT], float (&d)[EPT]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    c[j] = apg_x0(vc[j], vxe[j], p);
    d[j] = c[j] - apg_x0(vu[j], vxe[j], p);
    if constexpr (MOM) {
      va[j] = d[j] + beta * va[j];
      d[j] = va[j];
    }
  }
}

// the three sums of one iteration's elements.  Products of fp32 values are exact in double.
template <bool VEC>
__device__ __forceinline__ void apg_accumulate(const float (&c)[EPT], const float (&d)[EPT], int64_t k, int64_t per,
                                               double (&acc)[3]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const bool valid = sf_index<VEC>(k, j) < per;
    const double dd = valid ? (double)d[j] : 0.0, cc = valid ? (double)c[j] : 0.0;
    acc[0] += dd * dd;
    acc[1] += dd * cc;
    acc[2] += cc * cc;
  }
}

// pass 2 on one iteration: the guided data prediction, the update form, the stores
template <bool VEC, typename TS, typename TE>
__device__ __forceinline__ void apg_update(const float (&c)[EPT], const float (&d)[EPT], const TS* __restrict__ x,
                                           const TS* __restrict__ h1, const TS* __restrict__ h2, TS* __restrict__ xo,
                                           TS* __restrict__ mo, TS* __restrict__ xo2, int64_t k, int64_t per, float sc, float q,
                                           float eta, const KParams& p) {
  const bool nx = form_needs_x<FORM_RT>(p), nh1 = form_needs_h1<FORM_RT>(p), nh2 = form_needs_h2<FORM_RT>(p);
  const float s1 = p.cfg_scale - 1.f;
  float vx[EPT], vh1[EPT], vh2[EPT], ox[EPT], om[EPT];
  if (nx) sf_load<VEC, true>(x, k, per, vx);
  if (nh1) sf_load<VEC, true>(h1, k, per, vh1);
  if (nh2) sf_load<VEC, true>(h2, k, per, vh2);
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const float dn = sc * d[j], par = q * c[j];
    const float upd = (dn - par) + eta * par;
    const float mn = c[j] + s1 * upd;
    om[j] = mn;
    ox[j] = combine_any<FORM_RT, float, TE>(nx ? vx[j] : 0.f, mn, nh1 ? vh1[j] : 0.f, nh2 ? vh2[j] : 0.f, p, false);
  }
  sf_store<VEC>(xo, k, per, ox);
  if (xo2) sf_store<VEC>(xo2, k, per, ox);
  if (p.flags & DPM_F_STORE_M) sf_store<VEC>(mo, k, per, om);
}

// one sample, both passes.  KEEP: the register path (per <= SF_KEEP_MAX); MOM: beta != 0.  Called by every thread of the
// workgroup with workgroup-uniform template arguments: the barrier inside is reached by all of them.
template <bool VEC, bool KEEP, bool MOM, typename TS, typename TE>
__device__ __forceinline__ void apg_sample(const TS* __restrict__ x, const TS* __restrict__ xe, const TE* __restrict__ e0,
                                           const TE* __restrict__ e1, const TS* __restrict__ h1, const TS* __restrict__ h2,
                                           TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__ xo2, float* __restrict__ avg,
                                           int64_t per, const KParams& p, const ApgScalars a, double* red) {
  const int64_t nchunks = (per + SF_CHUNK - 1) / SF_CHUNK;
  double acc[3] = {0.0, 0.0, 0.0};
  float kc[KEEP ? SF_KEEP_CHUNKS : 1][EPT], kd[KEEP ? SF_KEEP_CHUNKS : 1][EPT];
  float vc[EPT], vu[EPT], vxe[EPT], va[EPT];
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k) {
      sf_load<VEC, true>(e0, k, per, vc);  // non-temporal: nothing reads the outputs again
      sf_load<VEC, true>(e1, k, per, vu);
      sf_load<VEC, false>(xe, k, per, vxe);  // (the state: pass 2 reads it again where it is the form's x)
      if constexpr (MOM) sf_load<VEC, true>(avg, k, per, va);
      apg_direction<MOM>(vc, vu, vxe, va, p, a.beta, kc[k], kd[k]);
      if constexpr (MOM) sf_store<VEC>(avg, k, per, va);
      apg_accumulate<VEC>(kc[k], kd[k], k, per, acc);
    }
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, false>(e0, k, per, vc);  // default cache policy: pass 2 reads these lines again
      if constexpr (!MOM) sf_load<VEC, false>(e1, k, per, vu);
      else sf_load<VEC, true>(e1, k, per, vu);
      sf_load<VEC, false>(xe, k, per, vxe);
      if constexpr (MOM) sf_load<VEC, true>(avg, k, per, va);
      apg_direction<MOM>(vc, vu, vxe, va, p, a.beta, kc[0], kd[0]);
      if constexpr (MOM) sf_store<VEC>(avg, k, per, va);
      apg_accumulate<VEC>(kc[0], kd[0], k, per, acc);
    }
  }
  double s[3];  // every thread holds the same sums, hence the same sc and q
  sf_reduce(acc, red, s);
  double sc64 = 1.0;
  if (a.r > 0.f) {
    const double t = (double)a.r / sqrt(s[0]);
    sc64 = t < 1.0 ? t : 1.0;
  }
  const float sc = (float)sc64, q = (float)(sc64 * s[1] / s[2]);
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k)
      if ((int64_t)k < nchunks) apg_update<VEC, TS, TE>(kc[k], kd[k], x, h1, h2, xo, mo, xo2, k, per, sc, q, a.eta, p);
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, true>(e0, k, per, vc);
      sf_load<VEC, true>(xe, k, per, vxe);
      if constexpr (MOM) {
        sf_load<VEC, false>(avg, k, per, kd[0]);  // what this thread stored in pass 1
#pragma unroll
        for (int j = 0; j < EPT; ++j) kc[0][j] = apg_x0(vc[j], vxe[j], p);
      } else {
        sf_load<VEC, true>(e1, k, per, vu);
        apg_direction<false>(vc, vu, vxe, va, p, 0.f, kc[0], kd[0]);
      }
      apg_update<VEC, TS, TE>(kc[0], kd[0], x, h1, h2, xo, mo, xo2, k, per, sc, q, a.eta, p);
    }
  }
}

// x: the state the update starts from (the evaluation state where the form reads none), xe: the state the network saw (= x when
// there is no separate one); h1 / h2 / mo / xo2 may be null where the stage does not name them; avg: the running average of the
// direction, fp32, null without a momentum.  `vec`: 16-byte accesses.
template <typename TS, typename TE>
__global__ __launch_bounds__(SF_THREADS) void stage_apg_kernel(const TS* __restrict__ x, const TS* __restrict__ xe,
                                                               const TE* __restrict__ e0, const TE* __restrict__ e1,
                                                               const TS* __restrict__ h1, const TS* __restrict__ h2,
                                                               TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__ xo2,
                                                               int64_t per, const KParams p, int vec, float* __restrict__ avg,
                                                               const ApgScalars a) {
  __shared__ double red[SF_WAVES * 3];
  const int64_t base = (int64_t)blockIdx.x * per;  // this workgroup's sample
  if (x) x += base;
  xe += base;
  e0 += base;
  e1 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  if (xo2) xo2 += base;
  if (avg) avg += base;
  const bool keep = per <= SF_KEEP_MAX;
#define DPM_APG_PATH(V, K)                                                                           \
  do {                                                                                               \
    if (avg) apg_sample<V, K, true>(x, xe, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);        \
    else apg_sample<V, K, false>(x, xe, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);           \
  } while (0)
  if (vec) {
    if (keep) DPM_APG_PATH(true, true);
    else DPM_APG_PATH(true, false);
  } else {
    if (keep) DPM_APG_PATH(false, true);
    else DPM_APG_PATH(false, false);
  }
#undef DPM_APG_PATH
}

// this unit's launch of one flagged stage (checked by dpm_stage_launch: kSampleGuidance, dpm_kernels.hip)
template <typename TS, typename TE>
int launch_sample_typed(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& c) {
  const ApgScalars a{st->cg_scale, st->thr_ratio, st->thr_max};
  float* const avg = a.beta != 0.f ? static_cast<float*>(b->workspace) : nullptr;
  return launch_sample_stage<TS, TE>(stage_apg_kernel<TS, TE>, "DPM_F_CFG_APG", "adaptive projected guidance stage kernel launch failed",
                                     st, b, c, avg, avg, a);
}

}  // namespace

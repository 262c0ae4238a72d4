// dpm_perp_kernel.hpp -- Perp-Neg guidance (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 stage, include/dpm_hip.h; Armandpour et al.
// 2023, "Re-imagine the Negative Prompt Algorithm"; ComfyUI's PerpNeg): stage_perp_kernel, a stage kernel that owns a whole
// SAMPLE and reads THREE network outputs, and its launcher (its table sibling, stage_perp_kernel_table, is dpm_table_perp.hpp's,
// on perp_sample below, in unit J).  Included by units I and J of dpm_stage_unit.hip behind
// dpm_sample_frame.hpp -- the workgroup, the lane-to-element map, the masked loads and stores, the reduction, the two access
// paths -- and by nothing else, so that every other unit compiles to the code it compiled to.
//
// The negative direction d2 = o_n - o_u loses its component along the positive one d0 = o_c - o_u, per sample, before it is
// subtracted.  One workgroup per sample, grid = batch:
//   pass 1   the sample's three raw outputs -> d0, d2 in fp32 and two sums in double per thread, <d2, d0> and <d0, d0> (products
//            of fp32 values are exact in double), reduced (sf_reduce); every thread then forms the same a = S_nd / S_dd
//   pass 2   perp = d2 - a * d0, gd = o_u + s * (d0 - w * perp), then the stage proper -- conversion, eps -> x0, update form,
//            stores -- on the sample
// Form, model type and prologue are read from the stage record (FORM_RT, PM_RT): one instantiation per dtype pair.
//   register path  o_c and o_u stay in registers between the passes (64 values per lane, as in stage_zstar_kernel, which leaves
//                  13-28 of the 256 VGPRs of a 512-thread workgroup: a third kept output does not fit).  The third operand
//                  crosses the barrier as d2, one of two ways (PARK):
//                    true   parked in LDS, 32 fp32 values per lane = 64 KiB per workgroup whatever the network's dtype; a lane
//                           reads back the 16-byte words it wrote itself, so the frame's one barrier is all there is
//                    false  not kept: pass 1 loads o_n with the default cache policy, pass 2 reads it again (L2) and takes the
//                           difference a second time
//                  The product instantiates PERP_PARK alone; the lab build carries both (DPM_TUNE_PERP_REREAD) so that one
//                  process times them over the same slabs -- tools/perp_in_loop.py, profiles/r32_cfg_perp_neg.md.
//   re-read path   samples above SF_KEEP_MAX: pass 2 reads all three outputs again, so pass 1 loads them with the default cache
//                  policy and the second read comes from L2
// The kernel carries s = cfg_scale and w = cg_scale and no state from stage to stage.
#pragma once

namespace {

constexpr bool PERP_PARK = true;  // the shipped register path (the faster of the two: profiles/r32_cfg_perp_neg.md)

typedef float perp_f4 __attribute__((ext_vector_type(4)));

// this lane's two 16-byte words of iteration k in the parked d2 (lane stride 16 bytes: a wavefront's access is 1 KiB dense)
__device__ __forceinline__ void perp_park(perp_f4* park, int k, const float (&d2)[EPT]) {
  park[(2 * k) * SF_THREADS + threadIdx.x] = perp_f4{d2[0], d2[1], d2[2], d2[3]};
  park[(2 * k + 1) * SF_THREADS + threadIdx.x] = perp_f4{d2[4], d2[5], d2[6], d2[7]};
}
__device__ __forceinline__ void perp_unpark(const perp_f4* park, int k, float (&d2)[EPT]) {
  const perp_f4 a = park[(2 * k) * SF_THREADS + threadIdx.x], b = park[(2 * k + 1) * SF_THREADS + threadIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    d2[j] = a[j];
    d2[4 + j] = b[j];
  }
}

// d2 of one iteration's elements and their share of the two sums: S_nd (acc[0]) and S_dd (acc[1]).  A masked element adds an
// exact zero.
template <bool VEC>
__device__ __forceinline__ void perp_accumulate(const float (&vc)[EPT], const float (&vu)[EPT], const float (&vn)[EPT], int64_t k,
                                                int64_t per, double (&acc)[2], float (&d2)[EPT]) {
#pragma unroll
  for (int j = 0; j < EPT; ++j) {
    const bool valid = sf_index<VEC>(k, j) < per;
    const float d0 = vc[j] - vu[j];
    d2[j] = vn[j] - vu[j];
    const double p = valid ? (double)d0 : 0.0;
    const double q = valid ? (double)d2[j] : 0.0;
    acc[0] += q * p;
    acc[1] += p * p;
  }
}

// The copies of the state a table row may name (stage_perp_kernel_table, dpm_table_perp.hpp): where xo2 is not null
// (workgroup-uniform) the state is stored to xo2 and xo3 as well, by x_out's own store -- the other two thirds of the network's
// next [3S, ...] input.  The lone kernel has no second store: its instantiation passes no pointers and takes the empty overload.
template <bool VEC, typename TS>
__device__ __forceinline__ void perp_store_copies(int64_t, int64_t, const float (&)[EPT]) {}
template <bool VEC, typename TS>
__device__ __forceinline__ void perp_store_copies(int64_t k, int64_t per, const float (&ox)[EPT], TS* xo2, TS* xo3) {
  if (xo2) {
    sf_store<VEC>(xo2, k, per, ox);
    sf_store<VEC>(xo3, k, per, ox);
  }
}

// pass 2 on one iteration: the guided raw output, the conversion, eps -> x0, the update form, the stores.  COPIES: a compile-time
// pack, empty (the lone kernel: the function is what it was) or the two copies' pointers (perp_store_copies).
template <bool VEC, typename TS, typename TE, typename... COPIES>
__device__ __forceinline__ void perp_update(const float (&vc)[EPT], const float (&vu)[EPT], const float (&d2)[EPT],
                                            const TS* __restrict__ x, const TS* __restrict__ xe, const TS* __restrict__ h1,
                                            const TS* __restrict__ h2, TS* __restrict__ xo, TS* __restrict__ mo, int64_t k,
                                            int64_t per, float a, const KParams& p, COPIES... copies) {
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
    const float d0 = vc[j] - vu[j];
    const float perp = d2[j] - a * d0;
    const float gd = vu[j] + p.cfg_scale * (d0 - p.cg_scale * perp);
    const float eps = to_noise<PM_RT>(gd, xev, p);
    const float mn = (p.flags & DPM_F_TO_X0) ? div_uniform(xev - p.sigma_e * eps, p.alpha_e, p.inv_alpha, (p.fastdiv & 1u) != 0u) : eps;
    om[j] = mn;
    ox[j] = combine_any<FORM_RT, float, TE>(nx ? xv : 0.f, mn, nh1 ? vh1[j] : 0.f, nh2 ? vh2[j] : 0.f, p, false);
  }
  sf_store<VEC>(xo, k, per, ox);
  perp_store_copies<VEC, TS>(k, per, ox, copies...);
  if (p.flags & DPM_F_STORE_M) sf_store<VEC>(mo, k, per, om);
}

// one sample, both passes.  KEEP: the register path (per <= SF_KEEP_MAX), PARK: its d2 crosses the barrier in LDS.  Called by
// every thread of the workgroup with workgroup-uniform template arguments: the barrier inside is reached by all of them.
// COPIES: perp_update's.
template <bool VEC, bool KEEP, bool PARK, typename TS, typename TE, typename... COPIES>
__device__ __forceinline__ void perp_sample(const TS* __restrict__ x, const TS* __restrict__ xe, const TE* __restrict__ e0,
                                            const TE* __restrict__ e1, const TE* __restrict__ e2, const TS* __restrict__ h1,
                                            const TS* __restrict__ h2, TS* __restrict__ xo, TS* __restrict__ mo, int64_t per,
                                            const KParams& p, double* red, perp_f4* park, COPIES... copies) {
  const int64_t nchunks = (per + SF_CHUNK - 1) / SF_CHUNK;
  double acc[2] = {0.0, 0.0};
  float kc[KEEP ? SF_KEEP_CHUNKS : 1][EPT], ku[KEEP ? SF_KEEP_CHUNKS : 1][EPT], vn[EPT], d2[EPT];
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k) {  // every load of the two kept outputs in flight before the first use
      sf_load<VEC, true>(e0, k, per, kc[k]);
      sf_load<VEC, true>(e1, k, per, ku[k]);
    }
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k) {
      sf_load<VEC, PARK>(e2, k, per, vn);  // (not parked: pass 2 reads these lines again -- default cache policy)
      perp_accumulate<VEC>(kc[k], ku[k], vn, k, per, acc, d2);
      if constexpr (PARK) perp_park(park, k, d2);
    }
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, false>(e0, k, per, kc[0]);  // default cache policy: pass 2 reads these lines again
      sf_load<VEC, false>(e1, k, per, ku[0]);
      sf_load<VEC, false>(e2, k, per, vn);
      perp_accumulate<VEC>(kc[0], ku[0], vn, k, per, acc, d2);
    }
  }
  double s[2];  // every thread holds the same sums, hence the same a
  sf_reduce(acc, red, s);
  // (S_dd == 0: every d0 is zero -- the positive prompt does not move the output -- and a = 0, defined; a NaN S_dd likewise)
  const float a = s[1] > 0.0 ? (float)(s[0] / s[1]) : 0.f;
  if constexpr (KEEP) {
#pragma unroll
    for (int k = 0; k < SF_KEEP_CHUNKS; ++k)
      if ((int64_t)k < nchunks) {
        if constexpr (PARK) {
          perp_unpark(park, k, d2);
        } else {
          sf_load<VEC, true>(e2, k, per, vn);
#pragma unroll
          for (int j = 0; j < EPT; ++j) d2[j] = vn[j] - ku[k][j];
        }
        perp_update<VEC, TS, TE>(kc[k], ku[k], d2, x, xe, h1, h2, xo, mo, k, per, a, p, copies...);
      }
  } else {
    for (int64_t k = 0; k < nchunks; ++k) {
      sf_load<VEC, true>(e0, k, per, kc[0]);
      sf_load<VEC, true>(e1, k, per, ku[0]);
      sf_load<VEC, true>(e2, k, per, vn);
#pragma unroll
      for (int j = 0; j < EPT; ++j) d2[j] = vn[j] - ku[0][j];
      perp_update<VEC, TS, TE>(kc[0], ku[0], d2, x, xe, h1, h2, xo, mo, k, per, a, p, copies...);
    }
  }
}

// x: the state the update starts from (the evaluation state where the form reads none), xe: the state the network saw (= x when
// there is no separate one); h1 / h2 / mo may be null where the stage does not name them; the guidance has no second store
// (the ninth pointer of the frame's launch is null).  `vec`: 16-byte accesses.  e2: dpm_buffers.g, the output under the negative
// condition.
template <typename TS, typename TE, bool PARK>
__global__ __launch_bounds__(SF_THREADS) void stage_perp_kernel(const TS* __restrict__ x, const TS* __restrict__ xe,
                                                                const TE* __restrict__ e0, const TE* __restrict__ e1,
                                                                const TS* __restrict__ h1, const TS* __restrict__ h2,
                                                                TS* __restrict__ xo, TS* __restrict__ mo, TS* __restrict__,
                                                                int64_t per, const KParams p, int vec, const TE* __restrict__ e2) {
  __shared__ double red[SF_WAVES * 2];
  __shared__ perp_f4 park[PARK ? SF_KEEP_CHUNKS * 2 * SF_THREADS : 1];
  const int64_t base = (int64_t)blockIdx.x * per;  // this workgroup's sample
  if (x) x += base;
  if (xe) xe += base;
  e0 += base;
  e1 += base;
  e2 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  const bool keep = per <= SF_KEEP_MAX;
  if (vec) {
    if (keep) perp_sample<true, true, PARK>(x, xe, e0, e1, e2, h1, h2, xo, mo, per, p, red, park);
    else perp_sample<true, false, PARK>(x, xe, e0, e1, e2, h1, h2, xo, mo, per, p, red, park);
  } else {
    if (keep) perp_sample<false, true, PARK>(x, xe, e0, e1, e2, h1, h2, xo, mo, per, p, red, park);
    else perp_sample<false, false, PARK>(x, xe, e0, e1, e2, h1, h2, xo, mo, per, p, red, park);
  }
}

// this unit's launch of one flagged DPM_GUIDE_CFG2 stage (checked by dpm_stage_launch: check_pair_guidance, check_perp_flag,
// dpm_kernels.hip); g counts among the operands the 16-byte path needs aligned
template <typename TS, typename TE>
int launch_perp_typed(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& c) {
  const TE* const e2 = static_cast<const TE*>(b->g);
#if DPM_LAB
  const int rr = tuning_for(b->opts).perp_reread;  // -1: the shipped body
  if (rr >= 0 && (rr == 0) != PERP_PARK)
    return launch_sample_stage<TS, TE>(stage_perp_kernel<TS, TE, !PERP_PARK>, "DPM_F_CFG2_PERP", "Perp-Neg stage kernel launch failed",
                                       st, b, c, e2, e2);
#endif
  return launch_sample_stage<TS, TE>(stage_perp_kernel<TS, TE, PERP_PARK>, "DPM_F_CFG2_PERP", "Perp-Neg stage kernel launch failed", st,
                                     b, c, e2, e2);
}

}  // namespace

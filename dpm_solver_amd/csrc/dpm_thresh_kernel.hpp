// dpm_thresh_kernel.hpp -- dynamic thresholding (ref :416-425), part 3 of 3: stage_thresh_kernel -- x0 of a sample's chunk
// computed once into LDS, the order statistics (dpm_thresh_select.hpp), clamp / divide / combine / store from LDS.
// Part of dpm_device.hpp (include that).
#pragma once

namespace {

// HOT != 0: the usual configuration fixed at compile time -- 16-byte accesses legal, no mask blend, form and guidance kind
// known -- so that the load and store loops are straight-line code without the wave-uniform branches of the run-time form
// and guidance and their operands (the kernel is as sensitive to its instruction count as to HBM):
//   HOT = 1  noise-prediction network with the division by the invariant alpha, top-K front end of the select;
//   HOT = 2  the same with the full level-0 histogram (quantiles far from 1; not instantiated since round 5: the catch-all
//            kernel serves them);
//   HOT = 3  like 1, the prologue chosen per sample at run time: x_start / v / score networks and divisors that fail the
//            guard of the division by an invariant (round 4: those ran the catch-all kernel, 14-19 % slower).
// Everything else runs the same source with HOT = 0 (run-time form, guidance, evaluation state, mask blend).
//
// The body lives in dpm_thresh_stage_body.inc, so that stage_thresh_kernel_table (dpm_table_thresh.hpp) is the same source: there
// TABLE = true, the cluster-free shape of ONE sample (s_only) -- k is the constant 1, so every cluster barrier, workspace access
// and hint word is dead code --, with the prologue chosen from the stage record itself (row_prologue_ok: what x0_prologue_ok
// says on the host) instead of ThrParams.fastdiv, which is one value per launch.  (Textual, not a __device__ function: with this
// body hoisted into a __forceinline__ function taking the operands by reference, the existing instantiations of the f16 pair
// compiled to 8 % more instructions in the HOT = 3 kernels and 27 % more in the catch-all one; included, they compile to the
// instructions they had before.)
__device__ __forceinline__ bool row_prologue_ok(const KParams& p) {
  return p.model_type == DPM_MODEL_NOISE && (p.flags & DPM_F_TO_X0) && (p.fastdiv & 1u);
}
template <typename TS, typename TE, int FORM, int GUIDE, bool XE, int T, int HOT>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(HOT != 0 ? 4 : DPM_THR_CATCHALL_WAVES, 4))) void stage_thresh_kernel(
    const TS* __restrict__ x_1, const TS* __restrict__ xe_1, const TE* __restrict__ e0_1, const TE* __restrict__ e1_1,
    const TE* __restrict__ g, const TS* __restrict__ h1_1, const TS* __restrict__ h2_1, TS* __restrict__ xo_1,
    TS* __restrict__ mo_1, KParams p, ThrParams tp, KExt ext, const ThrTab tab) {
  // the body's names besides the parameters (dpm_thresh_stage_body.inc lists and checks them): no table, no single sample
  constexpr bool TABLE = false;
  constexpr int s_only = 0;
#include "dpm_thresh_stage_body.inc"
}

}  // namespace

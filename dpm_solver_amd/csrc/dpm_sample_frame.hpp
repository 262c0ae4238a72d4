// dpm_sample_frame.hpp -- the frame of the stage kernels that own a whole SAMPLE (stage_rescale_kernel and its table sibling,
// dpm_rescale_kernel.hpp / dpm_table_rescale.hpp; stage_apg_kernel, dpm_apg_kernel.hpp): device helpers and the launcher
// skeleton, no kernel.  Included by units E and F of dpm_stage_unit.hip behind dpm_device.hpp, in front of their kernels.
//
// One workgroup of SF_THREADS = 512 threads per sample and two passes over it: pass 1 accumulates N sums in double per thread,
// sf_reduce makes them the sample's behind ONE barrier, pass 2 uses them.  A workgroup depends on nothing outside itself: no
// cluster, no workspace, no wait.  Every thread reaches the barrier; a ragged tail masks loads and stores, never control flow
// around it.
//   register path  a sample of at most SF_KEEP_MAX = 16384 elements (SD's [4,64,64]): 32 elements per thread and tensor stay in
//                  registers between the passes
//   re-read path   larger samples: pass 2 reads its operands again (L2)
// Access: 8 consecutive elements per lane and 16-byte accesses where the sample is whole 8-element groups and every operand is
// 16-byte aligned (`vec`), else one element per lane (ragged samples, views with offsets).  2-byte states leave by the
// write-through stores of the streaming kernels; a 4-byte state's 32 bytes per lane are two instructions that each fill every
// other 16 bytes, which stay cached stores as in the extended streaming kernels (dpm_access.hpp: store_pack).
#pragma once

namespace {

constexpr int SF_THREADS = 512, SF_WAVES = SF_THREADS / 64;
constexpr int SF_CHUNK = SF_THREADS * EPT;         // elements of one workgroup iteration
constexpr int SF_KEEP_CHUNKS = 4;                  // iterations whose operands the register path holds
constexpr int64_t SF_KEEP_MAX = (int64_t)SF_CHUNK * SF_KEEP_CHUNKS;

// element j of this lane in iteration k, relative to the sample
template <bool VEC>
__device__ __forceinline__ int64_t sf_index(int64_t k, int j) {
  return VEC ? k * SF_CHUNK + (int64_t)threadIdx.x * EPT + j : k * SF_CHUNK + (int64_t)j * SF_THREADS + threadIdx.x;
}
// the lane's 8 elements of iteration k; elements past the sample read a clamped (valid) address and are masked by the caller
template <bool VEC, bool NT, typename T>
__device__ __forceinline__ void sf_load(const T* __restrict__ s, int64_t k, int64_t per, float (&out)[EPT]) {
  if constexpr (VEC) {
    const int64_t gi = k * SF_THREADS + threadIdx.x, ng = per / EPT;
    load_pack<NT>(s, gi < ng ? gi : ng - 1, out);
  } else {
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const int64_t i = sf_index<false>(k, j);
      out[j] = to_f32(s[i < per ? i : per - 1]);
    }
  }
}
template <bool VEC, typename T>
__device__ __forceinline__ void sf_store(T* __restrict__ s, int64_t k, int64_t per, const float (&in)[EPT]) {
  if constexpr (VEC) {
    const int64_t gi = k * SF_THREADS + threadIdx.x;
    if (gi < per / EPT) store_pack<false, true>(s, gi, in);
  } else {
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const int64_t i = sf_index<false>(k, j);
      if (i < per) s[i] = from_f32<T>(in[j]);
    }
  }
}

// The per-thread sums `acc` -> the sample's sums `s`, the same in every thread: across the wavefront by cross-lane exchange
// (xor offsets 32 down to 1), across the wavefronts through `red` (SF_WAVES * N doubles of LDS) behind the frame's one
// barrier, the eight partial sums added in wave order.  Called by every thread of the workgroup.
template <int N>
__device__ __forceinline__ void sf_reduce(double (&acc)[N], double* red, double (&s)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
  const int wave = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int q = 0; q < N; ++q) red[wave * N + q] = acc[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = 0.0;
#pragma unroll
  for (int w = 0; w < SF_WAVES; ++w)
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] += red[w * N + q];
}

// (Each kernel advances its own operands to the workgroup's sample and spells its own ladder from the run-time vec / keep
// [/ momentum] to the compile-time path: a helper that takes the kernels' __restrict__ pointer parameters by reference, or a
// lambda that captures them, costs the lone kernels SGPR spills -- profiles/r24_sample_frame.md.)

// The launch of one flagged stage, `flag` its name (checked by dpm_stage_launch: check_stage_buffers): one workgroup per
// sample, the 16-byte path where every operand -- `extra` too, an operand of the kernel's own or null -- allows it.  `kern`
// takes the sample's nine pointers, per, the stage scalars and vec, then `tail`.
template <typename TS, typename TE, typename K, typename... Tail>
int launch_sample_stage(K kern, const char* flag, const char* failed, const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& c,
                        const void* extra, Tail... tail) {
  const Operands<TS, TE> op(st, b);
  const int64_t per = b->n / b->batch;
  if (b->batch > (int64_t)0x7fffffff)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: %s with a batch of %lld (one workgroup per sample)", flag,
                         (long long)b->batch);
  TS* const xo2 = static_cast<TS*>(b->x_out2);
  const bool vec = per % EPT == 0 && aligned(op.x, 16) && aligned(op.xe, 16) && aligned(op.h1, 16) && aligned(op.h2, 16) &&
                   aligned(op.xo, 16) && aligned(op.mo, 16) && aligned(xo2, 16) && aligned(op.e0, 16) && aligned(op.e1, 16) &&
                   aligned(extra, 16);
  launch(kern, dim3((unsigned)b->batch), dim3(SF_THREADS), 0, c, op.x, op.xe ? op.xe : op.x, op.e0, op.e1, op.h1, op.h2, op.xo,
         op.mo, xo2, per, op.p, vec ? 1 : 0, tail...);
  return launch_status(failed);
}

}  // namespace

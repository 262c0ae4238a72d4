// dpm_launch.hpp -- launch plumbing of the stage kernels: device info, cluster shape, tuning, variant dispatch,
// the fused multi-request launcher, the catch-all kernel handles (part of dpm_device.hpp; include that)
#pragma once
#include "dpm_grid_plan.hpp"

namespace {
static_assert(GRID_GROUP_ELEMS == EPT && GRID_MAX_THREADS == STAGE_MAX_THREADS, "dpm_grid_plan.hpp restates the kernels' constants");

// ------------------------------------------------------------------------------------------------
// launch plumbing
// ------------------------------------------------------------------------------------------------
struct DeviceInfo {
  int n_cu = 0;
  int lds = 0;
  char arch[64] = {0};
  bool ok = false;
};

inline const DeviceInfo& device_info() {
  static thread_local int cached_dev = -1;
  static thread_local DeviceInfo info;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return info;
  if (dev != cached_dev || !info.ok) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
      info.n_cu = prop.multiProcessorCount;
      info.lds = (int)prop.maxSharedMemoryPerMultiProcessor;
      std::strncpy(info.arch, prop.gcnArchName, sizeof(info.arch) - 1);
      info.ok = true;
      cached_dev = dev;
    }
  }
  return info;
}

inline bool aligned(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }
// the tensors of a plain request (plain_request: no separate evaluation state; the fused launches take no classifier
// gradient): state pointers aligned to a_s bytes, network outputs to a_e.  Operands::aligned_to is the single-request twin.
inline bool buffers_aligned(const dpm_buffers& b, size_t a_s, size_t a_e) {
  return aligned(b.x, a_s) && aligned(b.h1, a_s) && aligned(b.h2, a_s) && aligned(b.x_out, a_s) && aligned(b.m_out, a_s) &&
         aligned(b.e0, a_e) && aligned(b.e1, a_e);
}

// Two run-time booleans -> template arguments: calls f(std::bool_constant<a>{}, std::bool_constant<b>{}).  Every launcher
// with a compile-time x0 prologue (SPEC_NOISE_X0 against SPEC_GENERIC: spec_of) and a second binary axis -- classifier-free
// guidance for the fused launchers (guide_of), the KExt extension for the single-request ones -- selects its kernel through it.
// The instantiations are made in the order (1,1) (1,0) (0,1) (0,0), and a code object lays its kernels out in the order
// they were first named in: the callers pass their booleans in the order that keeps that layout (profiles/r14_launchers.md).
template <typename F>
auto with_flags(bool a, bool b, F&& f) {
  if (a) return b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  return b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}
template <typename X0>
constexpr int spec_of(X0) { return X0::value ? SPEC_NOISE_X0 : SPEC_GENERIC; }
template <typename Cfg>
constexpr int guide_of(Cfg) { return Cfg::value ? DPM_GUIDE_CFG : DPM_GUIDE_NONE; }

// the division-by-invariant of the specialised prologue is exact unless alpha's significand is all ones (or alpha is
// not a normal number): then the generic prologue, with a true division, runs instead
inline bool div_invariant_ok(float alpha) {
  uint32_t u;
  std::memcpy(&u, &alpha, 4);
  const uint32_t ex = (u >> 23) & 0xffu;
  return ex != 0u && ex != 0xffu && (u & 0x7fffffu) != 0x7fffffu && ex > 32u && ex < 222u;
}

inline KParams make_params(const dpm_stage* st) {
  KParams p;
  p.alpha_e = st->alpha_e;
  p.inv_alpha = 1.0f / st->alpha_e;
  p.sigma_e = st->sigma_e;
  p.cfg_scale = st->cfg_scale;
  p.cg_scale = st->cg_scale;
  p.cx = st->cx;
  p.c0 = st->c0;
  p.c1 = st->c1;
  p.c2 = st->c2;
  p.k0 = st->k[0];
  p.k1 = st->k[1];
  p.k2 = st->k[2];
  p.k3 = st->k[3];
  p.k4 = st->k[4];
  p.flags = st->flags;
  p.model_type = st->model_type;
  p.form = st->form;
  p.guidance = st->guidance;
  p.inv_sigma = 1.0f / st->sigma_e;
  p.fastdiv = (div_invariant_ok(st->alpha_e) ? 1u : 0u) | (div_invariant_ok(st->sigma_e) ? 2u : 0u);
  return p;
}

// may this stage run a compile-time data-prediction prologue (SPEC_NOISE_X0, thresholding HOT 1)?  Only the data-prediction
// form of a noise network (dpmsolver++: eps -> x0 by the invariant alpha) has one: x_start / v / score networks and an
// alpha the division guard rejects take the general prologue.  The eps form (algorithm_type "dpmsolver") had one too until
// round 5: with inputs from HBM the run-time prologue measures equal or faster on every eps-form launch (2M at cfg2 size
// fp16 / fp32, the unconditional and the CFG singlestep-3 sampler at [64,3,256,256]; profiles/r05_kernel_budget.md).
// Callers that honour Tuning::force_generic test it themselves.
inline bool x0_prologue_ok(const dpm_stage& st) {
  return st.model_type == DPM_MODEL_NOISE && (st.flags & DPM_F_TO_X0) && div_invariant_ok(st.alpha_e);
}

// launch-shape defaults (measured on MI355X: profiles/r01_tuning.md, r01_tuning_v3.txt, and r01_tuning_v4.txt with the
// write-through stores) and the run-time tuning hooks.  nt mask: bit 0 = nt loads; bits 1, 2 = nt x_out / m_out store,
// which only matter in a -DDPM_STORE_WRITE_THROUGH=0 build.  Two situations, two optima:
//   * a network ran since the inputs were written (every real sampling loop): the streams come from HBM and streaming
//     (nt) loads win -- [256,4,64,64] HBM-cold: fp16 8.4 vs 9.3 us, fp32 15.3 vs 16.3-16.5 us against the default cache
//     policy.  This is the default (DefNT = 5).
//   * the previous launch wrote the inputs (dpm_buffers.inputs_resident: frozen-model loops such as dpm_plan_run
//     without a model callback): they sit in the Infinity Cache and the default policy wins, with two tiles per
//     workgroup iteration when there is work for it -- fp16 5.5 vs 7.4-7.6 us, fp32 12.35 vs 12.9 us.  Variants exist for
//     the 2M / first-order kernels (HotCombo).
constexpr int DEF_U = 1;
// LAB build only: the lone-launch north-star kernels (2-byte state, 2M / first-order, inputs from HBM) with their read streams
// on the LDS-DMA path (stage_kernel_dma, DPM_TUNE_LDS_DMA).  Measured by rocprofv3 rows inside a network loop
// (profiles/r05_lone_floor.md): 8.32 us against 8.28 us through registers -- the no-arithmetic floor kernel gains 3-4 % from
// that path, the stage kernel nothing -- so the product keeps the register path and does not carry the variant.
#ifndef DPM_LDS_DMA_DEFAULT
#define DPM_LDS_DMA_DEFAULT 0
#endif
template <typename TS>
struct DefNT {
  static constexpr int value = 5;
};

template <int FORM, int GUIDE, bool XE>
struct HotCombo {
  static constexpr bool value = (FORM == DPM_FORM_TWO || FORM == DPM_FORM_LIN1) && GUIDE == DPM_GUIDE_NONE && !XE;
};

struct LaunchCtx {
  hipStream_t stream;
  hipEvent_t start, stop;  // both null: plain launch; else hipExtLaunchKernelGGL brackets the kernel itself
  // device-resident coefficients (the adaptive solver's on-device controller, dpm_kernels.hip): the float fields of
  // the stage record are read from `dyn` (device memory) by the kernel instead of from its arguments, and the launch
  // is a no-op when *skip != 0.  Honoured by the general-prologue kernels only.
  const dpm_stage* dyn = nullptr;
  const int32_t* skip = nullptr;
  // thresholded stage of n_multi requests fused into ONE launch (dpm_stage_launch_multi): `multi` = their buffer
  // records, all of the shape and dtypes of multi[0] (which is also the `b` the launcher is called with)
  const dpm_buffers* multi = nullptr;
  int n_multi = 0;
};

template <typename K, typename... Args>
void launch(K kern, dim3 grid, dim3 block, size_t lds, const LaunchCtx& c, Args... args) {
  if (c.start || c.stop)
    hipExtLaunchKernelGGL(kern, grid, block, lds, c.stream, c.start, c.stop, 0, args...);
  else
    hipLaunchKernelGGL(kern, grid, block, lds, c.stream, args...);
}

// the status of the kernels just launched: DPM_OK, or the launch error as "<what>: <HIP's text>"
inline int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DPM_OK : dpm_set_error((int)e, "%s: %s", what, hipGetErrorString(e));
}

// what a fused multi-request launcher returns -- without setting an error text -- when this stage (form, guidance,
// prologue, buffers) has no fused variant: the caller then launches the requests one by one
constexpr int MULTI_NOT_BUILT = -1000;

// ---- the requests of a fused launch (stage_kernel_multi, stage_kernel_het, the multi-request stage_thresh_kernel)
// a request the pointer tables can serve: the update starts from the state itself (x set, no separate evaluation state)
// and the network output is dense (no channel slice)
inline bool plain_request(const dpm_buffers& b) {
  return b.x && (!b.xe || b.xe == b.x) && (!b.eps_stride || b.eps_stride == b.n / b.batch);
}

// May this request join a fused streaming launch?  A streaming stage of a fused form (no thresholding / blend, no
// classifier guidance, no device-resident coefficients: the fused launchers take none), a plain request of whole 8-element
// groups, every buffer 16-byte aligned, a duplicate store only under classifier-free guidance.  The element sizes come from
// the dtype codes: only 4- and 2-byte pairs fuse.  SDE stages (DPM_F_NOISE) fuse too, with kernels of their own
// (stage_kernel_multi_noise, stage_kernel_het_noise: LIN1 / TWO); the callers keep them apart from the ODE stages.
// UniPC stages (DPM_FORM_UNIPC) fuse in lockstep (stage_kernel_multi) and at any position (the heterogeneous launch,
// stage_kernel_het_unipc), never with DPM_F_STORE_XC (x_out2 is then the corrected state, which the fused kernels'
// duplicate store does not write).
// Grouping of a per-request-stage call (stage_launch_multi_het, dpm_kernels.hip) is deterministic -- first come, first
// grouped: the first request not yet launched opens a group, and every later fusable request that agrees with it on dtypes,
// n, batch, model type, guidance kind, DPM_F_TO_X0 and DPM_F_NOISE joins, in call order, up to HET_MAX.  LIN1 and TWO records
// join any ODE group; MS3 and UNIPC records never share one (no kernel dispatches both): the first record of either form
// to join decides which of the two the group takes, records of the other form wait for a later group.
inline bool fusable_request(const dpm_stage& st, const dpm_buffers& b) {
  // (rescale, adaptive projected guidance, CFG-Zero*: a kernel per sample, never fused)
  if (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_CFG_RESCALE | DPM_F_CFG_APG | DPM_F_CFG_ZSTAR)) return false;
  if (st.guidance != DPM_GUIDE_NONE && st.guidance != DPM_GUIDE_CFG) return false;
  const bool ms3_ok = !(st.flags & DPM_F_NOISE);
  const bool unipc_ok = !(st.flags & (DPM_F_NOISE | DPM_F_STORE_XC));
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && !(ms3_ok && st.form == DPM_FORM_MS3) &&
      !(unipc_ok && st.form == DPM_FORM_UNIPC))
    return false;
  if (b.n <= 0 || b.n % EPT != 0 || !plain_request(b)) return false;
  const size_t as = (b.state_dtype == DPM_DTYPE_F32 ? 4 : 2) * EPT, ae = (b.eps_dtype == DPM_DTYPE_F32 ? 4 : 2) * EPT;
  if (b.x_out2 && (st.guidance != DPM_GUIDE_CFG || !aligned(b.x_out2, as))) return false;
  return buffers_aligned(b, as, ae);
}

// May a guidance-rescale request own a table row (DPM_TABLE_RESCALE; stage_rescale_kernel_table, dpm_table_rescale.hpp)?
// What dpm_stage_launch asks of the flag (check_stage_buffers: classifier-free guidance, a sample of at least 2 elements,
// phi in (0, 1], no thresholding / blend / noise / UniPC, 2- and 4-byte dtypes, a dense network output) and what a row asks:
// form LIN1 / TWO / MS3 / DENOISE (the last stage of denoise_to_zero, its buffers as LIN1's: the state is the evaluation
// state), a plain request, a SAMPLE (n / batch) of whole 8-element groups -- 16 bytes or a multiple in either dtype: the
// kernel works per sample and takes the 16-byte accesses only --, every buffer 16-byte aligned, x_out2 too.  For a request
// with batch >= 1 and n a multiple of it.
inline bool rescale_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_CFG_RESCALE) || (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE))) return false;
  if (st.guidance != DPM_GUIDE_CFG || !(st.cg_scale > 0.f && st.cg_scale <= 1.f)) return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  if (b.state_dtype == DPM_DTYPE_F64 || b.eps_dtype == DPM_DTYPE_F64) return false;
  if (b.n <= 0 || !plain_request(b) || !b.e0 || !b.e1 || !b.x_out) return false;
  const int64_t per = b.n / b.batch;
  const int64_t bs = per * (b.state_dtype == DPM_DTYPE_F32 ? 4 : 2), be = per * (b.eps_dtype == DPM_DTYPE_F32 ? 4 : 2);
  if (per < 2 || per % EPT != 0 || bs % 16 != 0 || be % 16 != 0) return false;
  return buffers_aligned(b, 16, 16) && aligned(b.x_out2, 16);
}

// May an adaptive-projected-guidance request own a table row (DPM_TABLE_APG; stage_apg_kernel_table, dpm_table_apg.hpp)?  What
// dpm_stage_launch asks of the flag (check_stage_buffers: classifier-free guidance on the data prediction, eta in [0, 1],
// r >= 0, beta in (-1, 1), no thresholding / blend / noise / rescale / UniPC, 2- and 4-byte dtypes, a dense network output)
// and what a row asks: form LIN1 / TWO / MS3 / DENOISE, a plain request, a SAMPLE (n / batch) of whole 8-element groups -- 16
// bytes or a multiple in either dtype: the kernel works per sample and takes the 16-byte accesses only --, every buffer
// 16-byte aligned, x_out2 too, and with a momentum the running average too: in a DPM_TABLE_APG call that is thr_hint.  For a
// request with batch >= 1 and n a multiple of it.
inline bool apg_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_CFG_APG) || (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_CFG_RESCALE))) return false;
  if (st.guidance != DPM_GUIDE_CFG || !(st.flags & DPM_F_TO_X0)) return false;
  if (!(st.cg_scale >= 0.f && st.cg_scale <= 1.f) || !(st.thr_ratio >= 0.f) || !(st.thr_max > -1.f && st.thr_max < 1.f)) return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  if (b.state_dtype == DPM_DTYPE_F64 || b.eps_dtype == DPM_DTYPE_F64) return false;
  if (b.n <= 0 || !plain_request(b) || !b.e0 || !b.e1 || !b.x_out) return false;
  const int64_t per = b.n / b.batch;
  const int64_t bs = per * (b.state_dtype == DPM_DTYPE_F32 ? 4 : 2), be = per * (b.eps_dtype == DPM_DTYPE_F32 ? 4 : 2);
  if (per < EPT || per % EPT != 0 || bs % 16 != 0 || be % 16 != 0) return false;
  if (st.thr_max != 0.f && (!b.thr_hint || !aligned(b.thr_hint, 16))) return false;
  return buffers_aligned(b, 16, 16) && aligned(b.x_out2, 16);
}

// May a CFG-Zero* request own a table row (DPM_TABLE_ZSTAR; stage_zstar_kernel_table, dpm_table_zstar.hpp)?  What
// dpm_stage_launch asks of the flag (check_stage_buffers: classifier-free guidance, no thresholding / blend / noise / rescale /
// adaptive projected guidance / UniPC, 2- and 4-byte dtypes, a dense network output; the flag has no field of its own) and what
// a row asks: form LIN1 / TWO / MS3 / DENOISE, a plain request, a SAMPLE (n / batch) of whole 8-element groups -- 16 bytes or a
// multiple in either dtype: the kernel works per sample and takes the 16-byte accesses only --, every buffer 16-byte aligned,
// x_out2 too.  For a request with batch >= 1 and n a multiple of it.
inline bool zstar_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_CFG_ZSTAR)) return false;
  if (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_CFG_RESCALE | DPM_F_CFG_APG)) return false;
  if (st.guidance != DPM_GUIDE_CFG) return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  if (b.state_dtype == DPM_DTYPE_F64 || b.eps_dtype == DPM_DTYPE_F64) return false;
  if (b.n <= 0 || !plain_request(b) || !b.e0 || !b.e1 || !b.x_out) return false;
  const int64_t per = b.n / b.batch;
  const int64_t bs = per * (b.state_dtype == DPM_DTYPE_F32 ? 4 : 2), be = per * (b.eps_dtype == DPM_DTYPE_F32 ? 4 : 2);
  if (per < EPT || per % EPT != 0 || bs % 16 != 0 || be % 16 != 0) return false;
  return buffers_aligned(b, 16, 16) && aligned(b.x_out2, 16);
}

// May a request under guidance over two conditions own a table row (DPM_TABLE_PAIR; stage_pair_kernel_table,
// dpm_table_pair.hpp)?  What dpm_stage_launch asks of the guidance (check_pair_guidance: finite scales, no thresholding / blend /
// noise / split stage, no UniPC form or flag, 2- and 4-byte dtypes, a dense network output) and what a row asks: form LIN1 / TWO /
// MS3 / DENOISE, a plain request, n a positive multiple of 8 (the kernel takes the 16-byte accesses only), e0, e1, g and x_out
// set, every buffer 16-byte aligned -- x_out2 and, in such a call, the third copy (thr_hint) too.  (Whether the two copies come
// together is the call's check, check_pair_copies, not the row's.)  A DPM_F_CFG2_PERP request is no such row: its blend is not
// the linear one (in a call that carries DPM_TABLE_PERP too it owns a Perp-Neg row, perp_row_ok, or goes on its own).
inline bool pair_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (st.guidance != DPM_GUIDE_CFG2 || !std::isfinite(st.cfg_scale) || !std::isfinite(st.cg_scale)) return false;
  if (st.flags & DPM_F_CFG2_PERP) return false;
  if (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_USER_X0 | DPM_F_UNIPC_DP | DPM_F_UNIPC_P2 | DPM_F_STORE_XC |
                  DPM_F_CFG_RESCALE | DPM_F_CFG_APG | DPM_F_CFG_ZSTAR))
    return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  if (b.state_dtype == DPM_DTYPE_F64 || b.eps_dtype == DPM_DTYPE_F64) return false;
  if (b.n <= 0 || b.n % EPT != 0 || !plain_request(b) || !b.e0 || !b.e1 || !b.g || !b.x_out) return false;
  return buffers_aligned(b, 16, 16) && aligned(b.g, 16) && aligned(b.x_out2, 16) && aligned(b.thr_hint, 16);
}

// May a Perp-Neg request own a table row (DPM_TABLE_PERP; stage_perp_kernel_table, dpm_table_perp.hpp)?  DPM_F_CFG2_PERP set,
// what a two-condition row asks (pair_row_ok's conditions) and what a kernel that owns a sample asks: a SAMPLE (n / batch) of
// whole 8-element groups -- 16 bytes or a multiple in either dtype: the kernel works per sample and takes the 16-byte accesses
// only --, every buffer 16-byte aligned, x_out2 and the third copy (thr_hint) too.  For a request with batch >= 1 and n a
// multiple of it.
inline bool perp_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_CFG2_PERP)) return false;
  if (st.guidance != DPM_GUIDE_CFG2 || !std::isfinite(st.cfg_scale) || !std::isfinite(st.cg_scale)) return false;
  if (st.flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_USER_X0 | DPM_F_UNIPC_DP | DPM_F_UNIPC_P2 | DPM_F_STORE_XC |
                  DPM_F_CFG_RESCALE | DPM_F_CFG_APG | DPM_F_CFG_ZSTAR))
    return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  if (b.state_dtype == DPM_DTYPE_F64 || b.eps_dtype == DPM_DTYPE_F64) return false;
  if (b.n <= 0 || !plain_request(b) || !b.e0 || !b.e1 || !b.g || !b.x_out) return false;
  const int64_t per = b.n / b.batch;
  const int64_t bs = per * (b.state_dtype == DPM_DTYPE_F32 ? 4 : 2), be = per * (b.eps_dtype == DPM_DTYPE_F32 ? 4 : 2);
  if (per < EPT || per % EPT != 0 || bs % 16 != 0 || be % 16 != 0) return false;
  return buffers_aligned(b, 16, 16) && aligned(b.g, 16) && aligned(b.x_out2, 16) && aligned(b.thr_hint, 16);
}

// the generator's parameters of one request's SDE stage: the seed from the request's own dpm_launch_opts (none: seed 0),
// the Philox counter word = the stage index, the scale = the stage's c2
inline KNoise noise_of(const dpm_stage& st, const dpm_buffers& b) {
  KNoise nz;
  nz.key0 = b.opts ? b.opts->noise_seed_lo : 0u;
  nz.key1 = b.opts ? b.opts->noise_seed_hi : 0u;
  nz.ctr = (uint32_t)st.index;
  nz.scale = st.c2;
  return nz;
}

// request r's entry in a fused pointer table (MultiTab, HetArgs, ThrTab); the caller sets the rest (xo2, ws)
template <typename Tab>
void fill_request(Tab& t, int r, const dpm_buffers& b) {
  t.x[r] = b.x;
  t.e0[r] = b.e0;
  t.e1[r] = b.e1;
  t.h1[r] = b.h1;
  t.h2[r] = b.h2;
  t.xo[r] = b.x_out;
  t.mo[r] = b.m_out;
}

// the operands of one single-request launch, typed: what both kernel families (streaming, thresholding) start from
template <typename TS, typename TE>
struct Operands {
  KParams p;
  const TS *x, *xe, *h1, *h2;
  const TE *e0, *e1, *g;
  TS *xo, *mo;
  KExt ext;       // duplicate output, mask blend, channel-sliced network output
  bool use_ext;
  int n_cu;
  Operands(const dpm_stage* st, const dpm_buffers* b)
      : p(make_params(st)),
        x(static_cast<const TS*>(b->x)),
        xe(static_cast<const TS*>(b->xe)),
        h1(static_cast<const TS*>(b->h1)),
        h2(static_cast<const TS*>(b->h2)),
        e0(static_cast<const TE*>(b->e0)),
        e1(static_cast<const TE*>(b->e1)),
        g(static_cast<const TE*>(b->g)),
        xo(static_cast<TS*>(b->x_out)),
        mo(static_cast<TS*>(b->m_out)) {
    const DeviceInfo& di = device_info();
    n_cu = di.n_cu > 0 ? di.n_cu : 256;
    std::memset(&ext, 0, sizeof ext);
    const bool blend = (st->flags & DPM_F_BLEND) != 0;
    ext.xo2 = b->x_out2;
    ext.mask = blend ? b->mask : nullptr;
    ext.ba = blend ? b->blend_a : nullptr;
    ext.bb = blend ? b->blend_b : nullptr;
    ext.mask_period = blend ? b->mask_period : 0;
    ext.per_sample = b->n / b->batch;
    ext.eps_stride = (b->eps_stride == ext.per_sample) ? 0 : b->eps_stride;
    ext.blend_alpha = st->blend_alpha;
    ext.blend_sigma = st->blend_sigma;
    use_ext = ext.xo2 || ext.mask || ext.eps_stride;
  }
  // every state pointer aligned to a_s bytes, every network-output pointer to a_e (null pointers are).  The full list for
  // every launcher: a pointer a kernel does not read is either null or one of the library's own allocations (the callers
  // bind h2 only to stages with an h2 slot and rebind g with the network outputs of every call).
  bool aligned_to(size_t a_s, size_t a_e) const {
    return aligned(x, a_s) && aligned(xe, a_s) && aligned(h1, a_s) && aligned(h2, a_s) && aligned(xo, a_s) &&
           aligned(mo, a_s) && aligned(e0, a_e) && aligned(e1, a_e) && aligned(g, a_e);
  }
};

// the KExt half of the vector kernels' 16-byte test: the extended vector kernel has no ragged tail and indexes whole
// 8-element groups
template <typename TS, typename TE>
bool ext_vec_ok(const Operands<TS, TE>& op, const dpm_buffers* b) {
  const size_t as = sizeof(TS) * EPT;
  const KExt& ext = op.ext;
  return !op.use_ext ||
         (aligned(ext.xo2, as) && aligned(ext.mask, as) && aligned(ext.ba, as) && aligned(ext.bb, as) && b->n % EPT == 0 &&
          ext.mask_period % EPT == 0 && (!ext.eps_stride || (ext.per_sample % EPT == 0 && ext.eps_stride % EPT == 0)));
}

// grid of the one-element-per-lane catch-all kernels (256 threads per workgroup, grid-stride loop)
inline dim3 scalar_grid(int64_t n, int n_cu) { return dim3((unsigned)scalar_grid_blocks(n, n_cu)); }

struct Shape {
  dim3 grid, block;
};
// launch shape of the streaming family's vector kernels (stage_kernel, stage_kernel_noise) at u tiles per iteration: one
// 256-lane group per u tiles, capped per CU; two groups per workgroup (stage_kernel) when that still leaves two workgroups
// per CU: what larger workgroups save is dispatches ([256,4,64,64]: 2048 -> 1024), and a small launch needs every CU more
// than it needs that.  (One step below -- 512 tiles, SD's [64,4,64,64] -- 512 threads measure neutral inside the loop:
// CFG + duplicate store 6.87-6.98 us against 7.00-7.02, the plain fp16 kernel 4.81-4.86 against 4.66-4.84;
// profiles/r04_block_threads.md.)
inline Shape stream_grid(int64_t n, int u, int n_cu, const Tuning& tn) {
  const StreamGridPlan g = stream_grid_plan(n, u, n_cu, tn.blocks_per_cu, tn.block_threads);
  return Shape{dim3((unsigned)g.blocks), dim3((unsigned)g.threads)};
}

// ---- a thresholded stage (stage_thresh_kernel): the plan (thr_launch_plan, dpm_thresh_plan.hpp: cluster shape, select
// parameters), the kernel flavour, the launch
template <typename TS, typename TE, int FORM, int GUIDE, bool XE>
int launch_thresh(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& stream, const Operands<TS, TE>& op) {
  const KExt& ext = op.ext;
  const int n_cu = op.n_cu;
  const Tuning tn = tuning_for(b->opts);
  if (stream.dyn) return dpm_set_error(DPM_ERR_UNSUPPORTED, "dynamic thresholding with device-resident coefficients");
  const int64_t per_sample = b->n / b->batch;
  // several requests in one launch: one batch of n_multi * batch samples -- more samples per launch, smaller (or no)
  // clusters -- whose sample s lives in the tensors of request s / batch (ThrTab)
  const bool multi = stream.multi != nullptr;
  const int64_t batch = multi ? (int64_t)stream.n_multi * b->batch : b->batch;
  hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream.stream, &cap_status);
  const bool capturing = cap_status != hipStreamCaptureStatusNone;
  const size_t a4s = sizeof(TS) * 4, a4e = sizeof(TE) * 4;
  bool vec = per_sample % 4 == 0 && ext.eps_stride % 4 == 0 && ext.mask_period % 4 == 0 && op.aligned_to(a4s, a4e) &&
             aligned(ext.xo2, a4s) && aligned(ext.mask, a4s) && aligned(ext.ba, a4s) && aligned(ext.bb, a4s);
  for (int r = 0; multi && r < stream.n_multi; ++r) vec = vec && buffers_aligned(stream.multi[r], a4s, a4e);
  ThrLaunchPlan lp = thr_launch_plan(*st, batch, per_sample, n_cu, ThrKnobs{tn.cluster_in_graph, tn.cluster_one_hop},
                                     capturing, vec, x0_prologue_ok(*st));
  if (lp.err) return dpm_set_error(DPM_ERR_UNSUPPORTED, "thresholding: batch / sample size out of range");
  ThrParams& tp = lp.tp;
  static const ThrTab no_tab = {};
  ThrTab tab_multi;
  if (multi) {
    // the fused launch serves plain requests: no extensions, the evaluation state is the state, distinct workspaces
    // (clusters of different requests run side by side); anything else is launched request by request
    if (XE || GUIDE == DPM_GUIDE_CLASSIFIER || stream.n_multi > MULTI_MAX) return MULTI_NOT_BUILT;
    std::memset(&tab_multi, 0, sizeof tab_multi);
    tp.bpr = (int32_t)b->batch;
    for (int r = 0; r < stream.n_multi; ++r) {
      const dpm_buffers& q = stream.multi[r];
      if (!plain_request(q) || q.x_out2) return MULTI_NOT_BUILT;
      if (lp.k > 1) {
        if (!q.workspace) return MULTI_NOT_BUILT;
        for (int r2 = 0; r2 < r; ++r2)
          if (stream.multi[r2].workspace == q.workspace) return MULTI_NOT_BUILT;
      }
      fill_request(tab_multi, r, q);
      tab_multi.ws[r] = static_cast<uint32_t*>(q.workspace);
    }
  }
  const ThrTab& tab = multi ? tab_multi : no_tab;
#ifdef DPM_THR_TIMING
  static_assert(DPM_LAB, "DPM_THR_TIMING instruments the lab build only");
  // debug build only: the DPM_THR_TIMING_LAUNCH-th thresholding launch of the process (default 40) is synchronised
  // and its stamps are written to $DPM_THR_TIMING_FILE, one line of 16 values per workgroup
  static uint64_t* t_dev = nullptr;
  static int t_launches = 0;
  if (!t_dev) (void)hipMalloc(&t_dev, 4096 * 16 * sizeof(uint64_t));
  tp.tdbg = t_dev;
  auto t_dump = [&](int64_t wgs) {
    const char* path = getenv("DPM_THR_TIMING_FILE");
    const char* at = getenv("DPM_THR_TIMING_LAUNCH");
    if (!path || ++t_launches != (at ? atoi(at) : 40) || wgs > 4096) return;
    (void)hipStreamSynchronize(stream.stream);
    std::vector<uint64_t> h((size_t)wgs * 16);
    (void)hipMemcpy(h.data(), t_dev, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (FILE* f = fopen(path, "w")) {
      for (int64_t i = 0; i < wgs; ++i) {
        for (int j = 0; j < 16; ++j) fprintf(f, "%llu ", (unsigned long long)h[(size_t)i * 16 + j]);
        fprintf(f, "\n");
      }
      fclose(f);
    }
  };
#else
  auto t_dump = [](int64_t) {};
#endif
  // the compile-time specialisation exists for the forms / guidance kinds samplers combine with thresholding
  // (classifier guidance -- the reference's own ImageNet-256 example samples with it AND thresholding, sample.sh:40-50 --
  // has the HOT = 3 flavour only: its two load loops cover the noise fast path and everything else)
  constexpr bool HOT_BUILT = (FORM == DPM_FORM_LIN1 || FORM == DPM_FORM_TWO || FORM == DPM_FORM_MS3) && !XE;
  constexpr bool HOT12_BUILT = HOT_BUILT && (GUIDE == DPM_GUIDE_NONE || GUIDE == DPM_GUIDE_CFG);
  const bool hot = HOT_BUILT && tp.vec && !ext.mask;
  const bool front = tp.topk > 0 || tp.quota > 0;  // the select starts from the per-thread maxima (quantile close to 1)
  // the general kernel reads form / guidance from the stage record and always takes the evaluation state through xe
  using ThrKernel = decltype(&stage_thresh_kernel<TS, TE, FORM_RT, GUIDE_RT, true, THR_THREADS, 0>);
  auto kern = reinterpret_cast<ThrKernel>(const_cast<void*>(dpm_catchall_thresh<TS, TE>()));
  if constexpr (HOT_BUILT) {
    // noise-prediction network + division by the invariant alpha: the compile-time prologue (HOT 1 / 2); any other
    // parameterisation with the usual near-1 quantile: the run-time prologue (HOT 3); the rest: the catch-all kernel
    bool chosen = false;
    if constexpr (HOT12_BUILT) {
      // (HOT 2 -- the same without the front end, for quantiles far from 1 -- was instantiated until round 5: no BASELINE
      // configuration and no reference example samples with such a ratio; those launches take the catch-all kernel)
      if (hot && front && tp.fastdiv && !tn.force_generic) {
        kern = stage_thresh_kernel<TS, TE, FORM, GUIDE, XE, THR_THREADS, 1>;
        chosen = true;
      }
    }
    if (!chosen && hot && front) kern = stage_thresh_kernel<TS, TE, FORM, GUIDE, XE, THR_THREADS, 3>;
  }
  int64_t grid = batch;
  tp.groups = (int32_t)batch;
  DeviceContext* chain = nullptr;  // != null: an eager clustered launch, chained device-wide (below)
  if (lp.k > 1) {
    // clusters synchronise through spin barriers: every workgroup of the grid must be resident at once
    // (cached per thread for the last (device, kernel, LDS size): kernels of different flavours may differ in occupancy)
    static thread_local int occ_dev = -1, occ = 0;
    static thread_local size_t occ_lds = 0;
    static thread_local const void* occ_kern = nullptr;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev != occ_dev || lp.lds_bytes != occ_lds || occ_kern != reinterpret_cast<const void*>(kern)) {
      int nb = 0;
      hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(kern), THR_THREADS,
                                                                  lp.lds_bytes);
      if (e != hipSuccess) return dpm_set_error((int)e, "hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e));
      occ_dev = dev;
      occ_lds = lp.lds_bytes;
      occ_kern = reinterpret_cast<const void*>(kern);
      occ = nb;
    }
    const int64_t cap = (int64_t)n_cu * (occ < 1 ? 1 : (occ > 2 ? 2 : occ));
    if (lp.k > cap)
      return dpm_set_error(DPM_ERR_UNSUPPORTED, "dynamic thresholding: a sample of %lld elements needs %lld co-resident "
                           "workgroups, the device holds %lld", (long long)per_sample, (long long)lp.k, (long long)cap);
    if (!b->workspace)
      return dpm_set_error(DPM_ERR_ARG,
                           "dynamic thresholding of %lld samples x %lld elements needs a workspace of "
                           "dpm_threshold_workspace_bytes() = %lld bytes",
                           (long long)b->batch, (long long)per_sample, (long long)thr_ws_bytes(b->batch, per_sample, n_cu));
    const int64_t groups = std::min<int64_t>(batch, cap / lp.k);
    tp.groups = (int32_t)groups;
    tp.ws = static_cast<uint32_t*>(b->workspace);
    grid = groups * lp.k;
    // No clearing of the workspace here: the caller hands it over zero-filled once, the kernel leaves it zero-filled
    // (dpm_threshold_workspace_bytes).  A wait on a peer that times out is recovered from inside the kernel (solo_select:
    // same results, no error); the host-mapped word only records that it happened (dpm_cluster_timeout_poll).
    tp.fault = cluster_fault_word(dev, !capturing);
    tp.spin_limit = (uint32_t)tn.thr_spin_limit;
#if DPM_LAB
    if (tn.thr_debug_fault == 1) tp.spin_limit = 0u;
    tp.debug_fault = tn.thr_debug_fault;
    tp.elect = tn.thr_elect > 0 && tp.quota > 0;
    tp.stagger = tn.thr_stagger;
#endif
    // the select bound predicted from the previous stages (dpm_buffers.thr_hint): single requests on the one-exchange route
    // -- where it pays: a small K (the wanted rank from the top), so that the predicted union (~1.3-1.9 K entries instead
    // of k * quota) is finished by rank counting.  Measured (tools/thr_routes.py): [32,3,64,64] (K = 63) 11.3 -> 10.7 us per
    // stage, union 236 -> 116 entries, every stage from the third on predicted; [64,3,256,256] (K = 983) 53 -> 59 us -- a
    // 10-step trajectory changes the statistic by 2.5x per stage, the extrapolation lands low and the union GROWS.
    if (!multi && tp.quota > 0 && b->thr_hint && tp.kbig <= 128) {
      tp.hint = b->thr_hint;
      tp.hint_reset = st->index <= 0;
      tp.hint_predict = tn.thr_predict;
    }
    // Two clustered launches on different streams could each hold part of the CUs with spinning workgroups and
    // starve the other's missing peers.  Within this process they are therefore chained device-wide: wait for the
    // previous clustered launch (whatever its stream), record after this one.  (Not under stream capture, where an
    // event recorded outside the capture cannot be waited on; see thr_launch_plan.)
    if (!capturing) chain = &device_context(dev);
  }
  std::unique_lock<std::mutex> lk;
  if (chain) {
    lk = std::unique_lock<std::mutex>(chain->mu);
    if (!chain->ev && hipEventCreateWithFlags(&chain->ev, hipEventDisableTiming) != hipSuccess) chain->ev = nullptr;
    if (chain->ev && chain->recorded) (void)hipStreamWaitEvent(stream.stream, chain->ev, 0);
  }
  launch(kern, dim3((unsigned)grid), dim3(THR_THREADS), lp.lds_bytes, stream, op.x, op.xe ? op.xe : op.x, op.e0, op.e1, op.g,
         op.h1, op.h2, op.xo, op.mo, op.p, tp, ext, tab);
  if (chain && chain->ev && hipEventRecord(chain->ev, stream.stream) == hipSuccess) chain->recorded = true;
  t_dump(grid);
  return launch_status("stage kernel launch failed");
}

// ---- a stage of the streaming family (stage_kernel / the one-element-per-lane catch-all): variant and launch shape
template <typename TS, typename TE, int FORM, int GUIDE, bool XE>
int launch_stream(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& stream, const Operands<TS, TE>& op) {
  const KParams& p = op.p;
  const TS *x = op.x, *xe = op.xe, *h1 = op.h1, *h2 = op.h2;
  const TE *e0 = op.e0, *e1 = op.e1, *g = op.g;
  TS *xo = op.xo, *mo = op.mo;
  const KExt& ext = op.ext;
  const int n_cu = op.n_cu;
  const bool use_ext = op.use_ext;
  const bool vec = op.aligned_to(sizeof(TS) * EPT, sizeof(TE) * EPT) && ext_vec_ok(op, b);
  // what the streaming family instantiates (binary size, build time and first-call cost: one kernel per combination and
  // dtype pair).  Round 5 measured what a compile-time prologue is worth against the run-time one (SPEC_GENERIC: the mode is
  // chosen once per workgroup iteration, the same straight-line code) -- 0-7 % per launch, profiles/r05_kernel_budget.md --
  // and keeps it where samplers spend their time:
  //   * a separate evaluation state (xe != x) occurs in the singlestep mid / final stages -- forms TWO and SS3T -- and
  //     in the FIRST stage of a multistep run with a corrector on x_t (mask blend, any correcting_xt_fn): the network saw
  //     the raw x_T, the update starts from the corrected state (ref :1179-1183) -- form LIN1, unguided or CFG;
  //   * the compile-time prologues (noise-prediction network) for the forms samplers spend their time in -- LIN1, TWO,
  //     MS3 -- unguided and under classifier-free guidance; classifier guidance (an autograd pass through the classifier
  //     per step dwarfs 3 % of a stage kernel) and that one first stage take SPEC_GENERIC; SS3T and DENOISE run the general
  //     prologue anyway (true division: the same bits);
  //   everything else goes through the one-element-per-lane kernel.
  constexpr bool COMBO_BUILT = ((!XE && !(FORM == DPM_FORM_DENOISE && GUIDE == DPM_GUIDE_CLASSIFIER)) || FORM == DPM_FORM_TWO ||
                                FORM == DPM_FORM_SS3T || (FORM == DPM_FORM_LIN1 && GUIDE != DPM_GUIDE_CLASSIFIER)) &&
                               !(FORM == DPM_FORM_SS3T && GUIDE == DPM_GUIDE_CLASSIFIER) &&  // singlestep-3 'taylor' under classifier guidance: scalar kernel
                               !(FORM == DPM_FORM_SS3T && !XE);  // the samplers always hand SS3T its evaluation state (the rocprofv3 name
                                                                 // set of the suite, profiles/r05_kernels_launched_suite.md, has no launch without)
  // the one denoise_to_zero launch of a trajectory with a KExt extension (mask blend, strided network output): scalar kernel
  constexpr bool EXT_BUILT = FORM != DPM_FORM_DENOISE;
  constexpr bool SPEC_BUILT = (FORM == DPM_FORM_LIN1 || FORM == DPM_FORM_TWO || FORM == DPM_FORM_MS3) &&
                              GUIDE != DPM_GUIDE_CLASSIFIER && !(XE && FORM == DPM_FORM_LIN1);
  // device-resident coefficients (adaptive solver): DYN kernels exist for the forms it launches -- first-order,
  // second-order and the singlestep-3 'taylor' combination -- with a 4-byte state (the reference's adaptive solver keeps
  // fp32 with a discrete schedule), unguided or CFG, without the KExt extensions; anything else takes the
  // one-element-per-lane kernel
  constexpr bool DYN_BUILT = COMBO_BUILT && sizeof(TS) == 4 && GUIDE != DPM_GUIDE_CLASSIFIER &&
                             ((FORM == DPM_FORM_LIN1 && !XE) || (FORM == DPM_FORM_TWO && (XE || GUIDE == DPM_GUIDE_NONE)) ||
                              (FORM == DPM_FORM_SS3T && XE));  // the launches of the adaptive solver's device-side controller
  const bool dyn_vec = stream.dyn && DYN_BUILT && !use_ext;
  if (!vec || !COMBO_BUILT || (stream.dyn && !dyn_vec) || (use_ext && !EXT_BUILT)) {
    using ScalarKernel = decltype(&stage_kernel_scalar<TS, TE, false>);  // the DYN = true variant has the same signature
    const void* k = stream.dyn ? dpm_catchall_scalar<TS, TE, true>() : dpm_catchall_scalar<TS, TE, false>();
    launch(reinterpret_cast<ScalarKernel>(const_cast<void*>(k)), scalar_grid(b->n, n_cu), dim3(256), 0, stream, x,
           xe ? xe : x, e0, e1, g, h1, h2, xo, mo, b->n, p, ext, stream.dyn, stream.skip);
  } else if constexpr (COMBO_BUILT) {
    const Tuning tn = tuning_for(b->opts);
    const bool noise = SPEC_BUILT && !stream.dyn && !tn.force_generic && x0_prologue_ok(*st);
    const int spec = noise ? SPEC_NOISE_X0 : SPEC_GENERIC;
    const bool big = stream_big(b->n, n_cu);  // two tiles per iteration only when there is work for it
#define DPM_LAUNCH(SPEC_, U_, NT_, EXT_)                                                                               \
  do {                                                                                                                 \
    const Shape sh_ = stream_grid(b->n, U_, n_cu, tn);                                                                 \
    launch(stage_kernel<TS, TE, FORM, GUIDE, XE, SPEC_, U_, NT_, EXT_>, sh_.grid, sh_.block, 0, stream, x, xe, e0, e1, \
           g, h1, h2, xo, mo, b->n, p, ext, stream.dyn, stream.skip);                                                  \
  } while (0)
    if (dyn_vec) {
      if constexpr (DYN_BUILT) {
        const Shape sh = stream_grid(b->n, 1, n_cu, tn);
        launch(stage_kernel<TS, TE, FORM, GUIDE, XE, SPEC_GENERIC, 1, DefNT<TS>::value, false, true>, sh.grid, sh.block, 0,
               stream, x, xe, e0, e1, g, h1, h2, xo, mo, b->n, p, ext, stream.dyn, stream.skip);
      }
    } else if (use_ext) {
      // one tile per workgroup (round 2 launched two for an fp32 state with 2-byte outputs: CFG + duplicate store at
      // [256,4,64,64] 18.1 / 20.3 us back-to-back / evicted against 17.3 / 19.3 with one, tools/stage_bench.py); nt mask of
      // the inputs-from-HBM situation
      constexpr int ENT = sizeof(TS) == 2 ? 1 : (sizeof(TE) == 4 ? 5 : 1);
      if constexpr (EXT_BUILT) {
        if (spec == SPEC_GENERIC) {
          DPM_LAUNCH(SPEC_GENERIC, 1, ENT, true);
        } else if constexpr (SPEC_BUILT) {
          DPM_LAUNCH(SPEC_NOISE_X0, 1, ENT, true);
        }
      }
    } else if (spec == SPEC_GENERIC) {
      DPM_LAUNCH(SPEC_GENERIC, 1, DefNT<TS>::value, false);
    } else if constexpr (SPEC_BUILT) {
      if constexpr (HotCombo<FORM, GUIDE, XE>::value) {
        // the north-star kernels (2M / 1st-order update, no guidance): (tiles per iteration, nt mask) by situation and
        // dtypes, from profiles/r01_tuning_v3.txt / r01_tuning_v4.txt:
        //   inputs cache-resident: default policy, two tiles per iteration when there is work for it
        //   inputs from HBM:       one tile per iteration, nt loads (+ nt m store for fp32 + fp32), see below
        const bool resident = b->inputs_resident != 0 || tn.assume_resident != 0;
        constexpr int CNT = sizeof(TS) == 2 ? 1 : (sizeof(TE) == 4 ? 5 : 1);  // nt mask of the HBM situation
#ifdef DPM_TUNING_VARIANTS  // tools/tune.py single: every (tiles per iteration, nt mask)
        if (tn.unroll > 0 && tn.nontemporal >= 0) {
          switch (tn.unroll * 8 + (tn.nontemporal & 7)) {
            case 8 + 0: DPM_LAUNCH(SPEC_NOISE_X0, 1, 0, false); break;
            case 8 + 1: DPM_LAUNCH(SPEC_NOISE_X0, 1, 1, false); break;
            case 8 + 5: DPM_LAUNCH(SPEC_NOISE_X0, 1, 5, false); break;
            case 16 + 0: DPM_LAUNCH(SPEC_NOISE_X0, 2, 0, false); break;
            case 16 + 1: DPM_LAUNCH(SPEC_NOISE_X0, 2, 1, false); break;
            case 16 + 5: DPM_LAUNCH(SPEC_NOISE_X0, 2, 5, false); break;
            case 32 + 0: DPM_LAUNCH(SPEC_NOISE_X0, 4, 0, false); break;
            case 32 + 1: DPM_LAUNCH(SPEC_NOISE_X0, 4, 1, false); break;
            case 32 + 5: DPM_LAUNCH(SPEC_NOISE_X0, 4, 5, false); break;
            case 64 + 0: DPM_LAUNCH(SPEC_NOISE_X0, 8, 0, false); break;
            case 64 + 1: DPM_LAUNCH(SPEC_NOISE_X0, 8, 1, false); break;
            case 64 + 5: DPM_LAUNCH(SPEC_NOISE_X0, 8, 5, false); break;
            default: DPM_LAUNCH(SPEC_NOISE_X0, DEF_U, DefNT<TS>::value, false); break;
          }
        } else
#endif
        if (resident) {
          if (big) DPM_LAUNCH(SPEC_NOISE_X0, 2, 0, false); else DPM_LAUNCH(SPEC_NOISE_X0, 1, 0, false);
        } else {
          // from HBM: ONE tile per workgroup for every dtype pair.  Round 1 picked two tiles for 4-byte states from the
          // interleaved-requests emulation (15.4 vs 15.6 us); INSIDE a torch network loop (profiles/r03_in_loop.md,
          // rocprofv3 rows, 342 launches each) one tile is 15.0 us against 16.3, and four / eight tiles -- fewer, fatter
          // wavefronts with every load issued up front, the emulation's favourite at 14.4 us -- are 15.2 / 23.8 us.
          bool dma = false;
#if DPM_LAB  // the LDS-DMA variant (2-byte state and network output, no ragged tail): an experiment of the lab build
          if constexpr (sizeof(TS) == 2 && sizeof(TE) == 2) dma = (tn.lds_dma < 0 ? DPM_LDS_DMA_DEFAULT : tn.lds_dma) != 0 && b->n % EPT == 0;
          if (dma) {
            if constexpr (sizeof(TS) == 2 && sizeof(TE) == 2) {
              const Shape sh = stream_grid(b->n, 1, n_cu, tn);
              launch(stage_kernel_dma<TS, TE, FORM, CNT>, sh.grid, sh.block, (size_t)(sh.block.x / 64) * 3072, stream, x, e0, h1, xo, mo,
                     b->n, p);
            }
          }
#endif
          if (!dma) DPM_LAUNCH(SPEC_NOISE_X0, 1, CNT, false);
        }
      } else {
        DPM_LAUNCH(SPEC_NOISE_X0, DEF_U, DefNT<TS>::value, false);
      }
    }
#undef DPM_LAUNCH
  }
  return launch_status("stage kernel launch failed");
}

// ---- an SDE stage (DPM_F_NOISE; checked by the caller: LIN1 / TWO, no thresholding, no device-resident coefficients) or
// a UniPC stage (DPM_FORM_UNIPC; checked by the caller: no thresholding / blend / noise / device-resident coefficients):
// the family's vector kernel where the streaming family's vector conditions hold -- one tile per iteration at stage_kernel's
// launch shape, unguided or classifier-free, the evaluation state is the state --, the pair's one-element-per-lane kernel
// of the family otherwise.
//   SDE:   stage_kernel_noise (whole 8-element groups only) / stage_kernel_scalar_noise.  The seed comes from the call's
//          dpm_launch_opts, the Philox counter is the stage index, the scale the stage's c2.
//   UniPC: stage_kernel with the nt mask of the inputs-from-HBM situation / stage_kernel_scalar_unipc.  DPM_F_STORE_XC
//          rides on the KExt flavour (x_out2).
template <typename TS, typename TE, int FORM, int GUIDE, bool XE>
int launch_noise_unipc(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& stream, const Operands<TS, TE>& op) {
  constexpr bool UNIPC = FORM == DPM_FORM_UNIPC;
  constexpr bool BUILT = (FORM == DPM_FORM_LIN1 || FORM == DPM_FORM_TWO || UNIPC) && GUIDE != DPM_GUIDE_CLASSIFIER && !XE;
  const KParams& p = op.p;
  const KExt& ext = op.ext;
  const bool vec = BUILT && (UNIPC || b->n % EPT == 0) && op.aligned_to(sizeof(TS) * EPT, sizeof(TE) * EPT) && ext_vec_ok(op, b);
  if (!vec) {
    const dim3 grid = scalar_grid(b->n, op.n_cu);
    const TS* xe = op.xe ? op.xe : op.x;
    if constexpr (UNIPC) {
      using ScalarUnipc = decltype(&stage_kernel_scalar_unipc<TS, TE>);
      launch(reinterpret_cast<ScalarUnipc>(const_cast<void*>(dpm_catchall_scalar_unipc<TS, TE>())), grid, dim3(256), 0, stream,
             op.x, xe, op.e0, op.e1, op.g, op.h1, op.h2, op.xo, op.mo, b->n, p, ext);
    } else {
      using ScalarNoise = decltype(&stage_kernel_scalar_noise<TS, TE>);
      launch(reinterpret_cast<ScalarNoise>(const_cast<void*>(dpm_catchall_scalar_noise<TS, TE>())), grid, dim3(256), 0, stream,
             op.x, xe, op.e0, op.e1, op.g, op.h1, op.h2, op.xo, op.mo, b->n, p, ext, noise_of(*st, *b));
    }
  } else if constexpr (BUILT) {
    const Tuning tn = tuning_for(b->opts);
    const Shape sh = stream_grid(b->n, 1, op.n_cu, tn);
    with_flags(op.use_ext, !tn.force_generic && x0_prologue_ok(*st), [&](auto use_ext, auto x0) {
      constexpr bool EXT = decltype(use_ext)::value;
      constexpr int SPEC = spec_of(x0);
      if constexpr (UNIPC) {
        constexpr int NT = sizeof(TS) == 2 ? 1 : (sizeof(TE) == 4 ? 5 : 1);
        launch(stage_kernel<TS, TE, DPM_FORM_UNIPC, GUIDE, false, SPEC, 1, NT, EXT>, sh.grid, sh.block, 0, stream, op.x, op.xe,
               op.e0, op.e1, op.g, op.h1, op.h2, op.xo, op.mo, b->n, p, ext, stream.dyn, stream.skip);
      } else {
        launch(stage_kernel_noise<TS, TE, FORM, GUIDE, SPEC, EXT>, sh.grid, sh.block, 0, stream, op.x, op.e0, op.e1, op.h1,
               op.xo, op.mo, b->n, p, ext, noise_of(*st, *b));
      }
    });
  }
  return launch_status(UNIPC ? "unipc stage kernel launch failed" : "noise stage kernel launch failed");
}

template <typename TS, typename TE, int FORM, int GUIDE, bool XE>
int launch_typed(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& stream) {
  const Operands<TS, TE> op(st, b);
  if constexpr (FORM == DPM_FORM_UNIPC) {
    return launch_noise_unipc<TS, TE, FORM, GUIDE, XE>(st, b, stream, op);
  } else {
    if (st->flags & DPM_F_NOISE) return launch_noise_unipc<TS, TE, FORM, GUIDE, XE>(st, b, stream, op);
    return (st->flags & DPM_F_THRESH) ? launch_thresh<TS, TE, FORM, GUIDE, XE>(st, b, stream, op)
                                      : launch_stream<TS, TE, FORM, GUIDE, XE>(st, b, stream, op);
  }
}

// Launch shape of the fused kernel (profiles/r02_tune_multi.txt, 32 x [256,4,64,64], kernel-only per request-stage):
// the inputs of a fused launch always come from HBM (R x 42 MB of other requests' traffic passed since they were
// written) -> streaming loads; one super-tile per workgroup -- a grid of all R x tiles workgroups, no grid-stride loop:
// fp16 7.95 us with the grid capped at 8 workgroups per CU, 7.7 / 7.5 at 16 / 32 per CU, 6.93 uncapped (0.757 of the
// HBM peak; fp32 15.4 -> 13.9, fp32 state + fp16 output 13.3 -> 12.6); two tiles per workgroup for 4-byte states.
// Store policy of 2-byte states (profiles/r07_fused_floor.md, rocprofv3 rows, 32 x [256,4,64,64] fp16 back to back): the
// new state written through and the model value by a non-temporal store (nt mask bit 3) -- the no-arithmetic floor of
// the five streams 211.5 -> 189.9 us, both stores written through or both nt 211.5 / 212.7; LDS-DMA reads, two tiles of
// loads in flight and resident grids were no faster.  4-byte states keep both stores written through (not measured).
template <typename TS, typename TE>
struct MultiShape {
  static constexpr int U = (sizeof(TS) == 4) ? 2 : 1;
  static constexpr int NT = (sizeof(TS) == 2) ? 1 | 8 : 1;
  static constexpr int THREADS = 256;  // per workgroup (256 / 512: stage_kernel_multi)
};

struct FusedShape {
  dim3 grid, block;
  uint32_t spr;       // super-tiles (u tiles of one request) per request
  uint32_t xcd_span;  // != 0: super-tiles per XCD of the XCD-contiguous remap (stage_kernel_multi)
};
// the fused kernels' launch shape for n_req requests of n elements at u tiles per super-tile: one super-tile per 256-lane
// group, XCD-contiguous super-tiles for 2-byte states (Tuning::multi_xcd_remap).  `capped`: the kernel loops over its
// super-tiles (stage_kernel_multi), so the multi_blocks_per_cu tuning hook may cap the grid; stage_kernel_het has no such
// loop and always gets the whole grid.
template <typename TS, typename TE>
FusedShape fused_grid(int64_t n, int n_req, int u, const Tuning& tn, bool capped) {
  const int64_t spr = ((n / EPT + 255) / 256 + u - 1) / u;
  const int64_t groups = spr * n_req;  // 256-lane groups of work: one super-tile each
  const int bt = tn.block_threads > 0 ? tn.block_threads : MultiShape<TS, TE>::THREADS;
  const int64_t per = bt / 256;
  const bool remap = tn.multi_xcd_remap < 0 ? sizeof(TS) == 2 : tn.multi_xcd_remap != 0;
  const uint32_t span = remap ? (uint32_t)((groups + 7) / 8) : 0u;
  int64_t blocks = span ? 8 * (((int64_t)span + per - 1) / per) : (groups + per - 1) / per;
  if (capped && tn.multi_blocks_per_cu > 0) {
    const DeviceInfo& di = device_info();
    blocks = std::min(blocks, (int64_t)(di.n_cu > 0 ? di.n_cu : 256) * tn.multi_blocks_per_cu);
  }
  return FusedShape{dim3((unsigned)blocks), dim3((unsigned)bt), (uint32_t)spr, span};
}

// ---- fused multi-request launch of the streaming family (stage_kernel_multi); thresholded stages fuse inside
// launch_typed (LaunchCtx::multi)
template <typename TS, typename TE, int FORM, int GUIDE, int SPEC>
int launch_multi_spec(const dpm_stage* st, const dpm_buffers* bs, int n_req, const LaunchCtx& c) {
  const Tuning tn = tuning_for(bs[0].opts);
  MultiTab tab;
  std::memset(&tab, 0, sizeof tab);
  for (int r = 0; r < n_req; ++r) {
    fill_request(tab, r, bs[r]);
    tab.xo2[r] = bs[r].x_out2;
  }
  const KParams p = make_params(st);
  const int64_t n = bs[0].n;
  auto go = [&](auto kern, int u) {
    const FusedShape sh = fused_grid<TS, TE>(n, n_req, u, tn, true);
    launch(kern, sh.grid, sh.block, 0, c, tab, n, (uint32_t)n_req, sh.spr, p, sh.xcd_span);
  };
  constexpr int DU = MultiShape<TS, TE>::U, DN = MultiShape<TS, TE>::NT;
#ifdef DPM_TUNING_VARIANTS  // tools/tune.py multi: every (tiles per iteration, nt mask) of the 2M kernel
  if constexpr (FORM == DPM_FORM_TWO && GUIDE == DPM_GUIDE_NONE && SPEC == SPEC_NOISE_X0) {
    if (tn.unroll > 0 && tn.nontemporal >= 0) {
      switch (tn.unroll * 8 + (tn.nontemporal & 7) + ((tn.nontemporal & 8) ? 64 : 0)) {  // nt mask 9: MultiShape's
        case 8 + 0: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 1, 0>, 1); break;
        case 8 + 1: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 1, 1>, 1); break;
        case 8 + 5: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 1, 5>, 1); break;
        case 64 + 8 + 1: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 1, 9>, 1); break;
        case 16 + 0: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 2, 0>, 2); break;
        case 16 + 1: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 2, 1>, 2); break;
        case 16 + 5: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, 2, 5>, 2); break;
        default: go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, DU, DN>, DU); break;
      }
      return launch_status("fused stage kernel launch failed");
    }
  }
#endif
  go(stage_kernel_multi<TS, TE, FORM, GUIDE, SPEC, DU, DN>, DU);
  return launch_status("fused stage kernel launch failed");
}

// ---- the same for an SDE stage (stage_kernel_multi_noise): MultiShape's tiles and cache policy, the whole grid (the
// kernel has no loop over super-tiles), every request's Philox key from its own bs[r].opts
template <typename TS, typename TE, int FORM, int GUIDE, int SPEC>
int launch_multi_noise_spec(const dpm_stage* st, const dpm_buffers* bs, int n_req, const LaunchCtx& c) {
  const Tuning tn = tuning_for(bs[0].opts);
  MultiTab tab;
  MultiKeys keys;
  std::memset(&tab, 0, sizeof tab);
  std::memset(&keys, 0, sizeof keys);
  for (int r = 0; r < n_req; ++r) {
    fill_request(tab, r, bs[r]);
    tab.xo2[r] = bs[r].x_out2;
    const KNoise nz = noise_of(*st, bs[r]);
    keys.k0[r] = nz.key0;
    keys.k1[r] = nz.key1;
  }
  constexpr int U = MultiShape<TS, TE>::U;
  const FusedShape sh = fused_grid<TS, TE>(bs[0].n, n_req, U, tn, false);
  launch(stage_kernel_multi_noise<TS, TE, FORM, GUIDE, SPEC, U, MultiShape<TS, TE>::NT>, sh.grid, sh.block, 0, c, tab, keys,
         bs[0].n, (uint32_t)n_req, sh.spr, make_params(st), sh.xcd_span, (uint32_t)st->index, st->c2);
  return launch_status("fused noise stage kernel launch failed");
}

// every request of the group: same stage, n, batch, dtypes (checked by the caller); here: does every request pass
// fusable_request, and which prologue runs
template <typename TS, typename TE>
int launch_multi_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const LaunchCtx& c) {
  for (int r = 0; r < n_req; ++r)
    if (!fusable_request(*st, bs[r])) return MULTI_NOT_BUILT;
  const bool cfg = st->guidance == DPM_GUIDE_CFG;
  const bool generic = !x0_prologue_ok(*st) || tuning_for(bs[0].opts).force_generic != 0;
  using Lin1 = std::integral_constant<int, DPM_FORM_LIN1>;
  using Two = std::integral_constant<int, DPM_FORM_TWO>;
  if (st->flags & DPM_F_NOISE) {
    auto go = [&](auto form) {
      return with_flags(generic, cfg, [&](auto gen, auto cfg_) {
        return launch_multi_noise_spec<TS, TE, decltype(form)::value, guide_of(cfg_), spec_of(std::bool_constant<!gen>{})>(st, bs, n_req, c);
      });
    };
    return st->form == DPM_FORM_LIN1 ? go(Lin1{}) : go(Two{});
  }
  auto go = [&](auto form) {
    return with_flags(generic, cfg, [&](auto gen, auto cfg_) {
      return launch_multi_spec<TS, TE, decltype(form)::value, guide_of(cfg_), spec_of(std::bool_constant<!gen>{})>(st, bs, n_req, c);
    });
  };
  switch (st->form) {
    case DPM_FORM_LIN1: return go(Lin1{});
    case DPM_FORM_TWO: return go(Two{});
    case DPM_FORM_UNIPC: return go(std::integral_constant<int, DPM_FORM_UNIPC>{});
    default: return go(std::integral_constant<int, DPM_FORM_MS3>{});
  }
}

// ---- heterogeneous fused launch (stage_kernel_het): request r advanced by st[r].  The caller (dpm_kernels.hip) has
// grouped the requests: every one passes fusable_request, and they agree on dtypes, n, batch, model type, guidance kind,
// DPM_F_TO_X0 and DPM_F_NOISE (a group of SDE stages takes stage_kernel_het_noise, each request with its own KNoise), and holds
// MS3 or UNIPC records, never both (a group with a UNIPC record takes stage_kernel_het_unipc).  Here: the prologue
// (compile-time only when every request may run it), the smallest form set that covers the group, the launch shape of the
// lockstep kernel (MultiShape, XCD-contiguous remap).
template <typename TS, typename TE>
int launch_het_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const LaunchCtx& c) {
  if (n_req < 1 || n_req > HET_MAX)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one fused launch", n_req);
  const Tuning tn = tuning_for(bs[0].opts);
  HetNoiseArgs an;  // (the ODE kernels take its first member)
  std::memset(&an, 0, sizeof an);
  HetArgs& a = an.h;
  bool ms3 = false, unipc = false;
  const bool sde = (st[0].flags & DPM_F_NOISE) != 0;
  bool x0 = !tn.force_generic;
  for (int r = 0; r < n_req; ++r) {
    fill_request(a, r, bs[r]);
    a.xo2[r] = bs[r].x_out2;
    a.p[r] = make_params(&st[r]);
    if (sde) an.nz[r] = noise_of(st[r], bs[r]);
    ms3 = ms3 || st[r].form == DPM_FORM_MS3;
    unipc = unipc || st[r].form == DPM_FORM_UNIPC;
    x0 = x0 && x0_prologue_ok(st[r]);
  }
  if (unipc && (ms3 || sde))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a UniPC stage grouped with a third-order or an SDE stage");
  const FusedShape sh = fused_grid<TS, TE>(bs[0].n, n_req, MultiShape<TS, TE>::U, tn, false);
  a.n = bs[0].n;
  a.nreq = (uint32_t)n_req;
  a.spr = sh.spr;
  a.xcd_span = sh.xcd_span;
  const bool cfg = st[0].guidance == DPM_GUIDE_CFG;
  constexpr int U = MultiShape<TS, TE>::U, NT = MultiShape<TS, TE>::NT;
  if (sde) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_het_noise<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, an);
    });
  } else if (unipc) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_het_unipc<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, a);
    });
  } else if (ms3) {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_het<TS, TE, HET_FORMS_3, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, a);
    });
  } else {
    with_flags(x0, cfg, [&](auto x0_, auto cfg_) {
      launch(stage_kernel_het<TS, TE, HET_FORMS_2, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, a);
    });
  }
  return launch_status("fused stage kernel launch failed");
}

template <typename TS, typename TE, int FORM, int GUIDE>
int launch_xe(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& s) {
  return (b->xe != nullptr && b->xe != b->x) ? launch_typed<TS, TE, FORM, GUIDE, true>(st, b, s)
                                            : launch_typed<TS, TE, FORM, GUIDE, false>(st, b, s);
}

template <typename TS, typename TE, int FORM>
int launch_guide(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& s) {
  switch (st->guidance) {
    case DPM_GUIDE_NONE: return launch_xe<TS, TE, FORM, DPM_GUIDE_NONE>(st, b, s);
    case DPM_GUIDE_CFG: return launch_xe<TS, TE, FORM, DPM_GUIDE_CFG>(st, b, s);
    case DPM_GUIDE_CLASSIFIER: return launch_xe<TS, TE, FORM, DPM_GUIDE_CLASSIFIER>(st, b, s);
  }
  return dpm_set_error(DPM_ERR_ARG, "unknown guidance %d", st->guidance);
}

// the single-request launchers of the update forms one translation unit instantiates (FORMS, dpm_internal.hpp: bit f =
// form f); a form outside them is an error here (dpm_kernels.hip hands every stage to the unit of its form)
template <typename TS, typename TE, unsigned FORMS>
int launch_form(const dpm_stage* st, const dpm_buffers* b, const LaunchCtx& s) {
  switch (st->form) {
#define DPM_FORM_CASE(F)                                                       \
  case F:                                                                      \
    if constexpr ((FORMS >> F) & 1u) return launch_guide<TS, TE, F>(st, b, s); \
    break;
    DPM_FORM_CASE(DPM_FORM_LIN1)
    DPM_FORM_CASE(DPM_FORM_TWO)
    DPM_FORM_CASE(DPM_FORM_MS3)
    DPM_FORM_CASE(DPM_FORM_SS3T)
    DPM_FORM_CASE(DPM_FORM_DENOISE)
    DPM_FORM_CASE(DPM_FORM_UNIPC)
#undef DPM_FORM_CASE
  }
  return dpm_set_error(DPM_ERR_ARG, "unknown update form %d", st->form);
}

}  // namespace

#ifdef DPM_CATCHALL_HOME
template <typename TS, typename TE>
const void* dpm_catchall_thresh() {
  return reinterpret_cast<const void*>(&stage_thresh_kernel<TS, TE, FORM_RT, GUIDE_RT, true, THR_THREADS, 0>);
}
template <typename TS, typename TE, bool DYN>
const void* dpm_catchall_scalar() {
  return reinterpret_cast<const void*>(&stage_kernel_scalar<TS, TE, DYN>);
}
template <typename TS, typename TE>
const void* dpm_catchall_scalar_noise() {
  return reinterpret_cast<const void*>(&stage_kernel_scalar_noise<TS, TE>);
}
template <typename TS, typename TE>
const void* dpm_catchall_scalar_unipc() {
  return reinterpret_cast<const void*>(&stage_kernel_scalar_unipc<TS, TE>);
}
#endif

// dpm_table_thresh.hpp -- thresholded rows of the table-driven launch (DPM_TABLE_THRESH): stage_thresh_kernel_table and its
// launcher (part of dpm_device.hpp; include that)
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A thresholded request used to leave continuous batching altogether: stage_thresh_kernel takes ONE stage record per launch
// (lockstep, ThrTab), so 256 staggered requests of [1,3,64,64] were 256 launches per tick, each of them a cluster of six
// workgroups with spin waits and a workspace.  A table row is one request of a few small samples, and a sample of at most
// THR_CHUNK_MAX elements fits the LDS of ONE workgroup: here one workgroup advances one sample of one row -- the body of
// stage_thresh_kernel (dpm_thresh_stage_body.inc) with TABLE = true, its cluster-free shape: no cluster barrier, no
// workspace, no hint word, no wait on anybody.  Everything per row comes from the row, read IN PLACE through the const
// __restrict__ table pointer with a wave-uniform index (scalar loads, as stage_kernel_table; the kernel never writes the
// table): the 8 pointers, the form (a run-time switch inside combine_any: LIN1 / TWO / MS3, and DENOISE, the thresholded
// last stage of denoise_to_zero), the coefficients, DPM_F_STORE_M, the duplicate store under classifier-free guidance, and
// the prologue -- division by the invariant alpha or the general one (row_prologue_ok), chosen once per sample as HOT = 3
// does.  What a group shares travels in the kernel arguments (ThrParams of thr_launch_plan for one workgroup per sample):
// per_sample, lo / hi / w, max_val, the top-K front end's topk / mrank, and bpr = the samples per row.
// Every sample gets the bits of its request's own launch: the order statistics are exact on every route, the arithmetic
// around them is the same source.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TE, int GUIDE>
__global__ __launch_bounds__(THR_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void stage_thresh_kernel_table(
    const TableRow* __restrict__ rows, ThrParams tp) {
  static_assert(GUIDE == DPM_GUIDE_NONE || GUIDE == DPM_GUIDE_CFG, "a table row: no classifier guidance");
  // the body's compile-time shape: run-time form, 16-byte accesses, no mask blend, the prologue chosen per sample (HOT = 3)
  constexpr int FORM = FORM_RT, T = THR_THREADS, HOT = 3;
  constexpr bool XE = false, TABLE = true;
  // The body's other names (dpm_thresh_stage_body.inc lists and checks them): s_only, p, tp, ext, tab, x_1 .. mo_1, g.
  // sample blockIdx.x of the group: sample s_only of row r, bpr samples per row (the grid is exactly the group's samples)
  const uint32_t bpr = (uint32_t)tp.bpr;
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / bpr));
  const int s_only = (int)(blockIdx.x - r * bpr);
  const TableRow& row = rows[r];
  const KParams& p = row.p;
  KExt ext = {};
  if constexpr (GUIDE == DPM_GUIDE_CFG) ext.xo2 = (void*)row.xo2;
  const ThrTab tab = {};  // (the kernel-argument pointer table of the lockstep launch: never read with TABLE = true)
  const TS* __restrict__ x_1 = (const TS*)row.x;
  const TS* __restrict__ xe_1 = x_1;
  const TE* __restrict__ e0_1 = (const TE*)row.e0;
  const TE* __restrict__ e1_1 = (const TE*)row.e1;
  const TE* __restrict__ g = nullptr;
  const TS* __restrict__ h1_1 = (const TS*)row.h1;
  const TS* __restrict__ h2_1 = (const TS*)row.h2;
  TS* __restrict__ xo_1 = (TS*)row.xo;
  TS* __restrict__ mo_1 = (TS*)row.mo;
#include "dpm_thresh_stage_body.inc"
}

// may a thresholded request own a table row (DPM_TABLE_THRESH)?  Today's fusable checks apart from the DPM_F_THRESH bit --
// form LIN1 / TWO / MS3, guidance none or CFG, a plain dense request of whole 8-element groups, 16-byte aligned buffers,
// x_out2 only under CFG, 2- and 4-byte pairs (the caller's pair_of) --, no mask blend, no noise, and a SAMPLE (n / batch) of
// whole 4-element groups that fits one workgroup's LDS: the kernel works per sample and always takes the 4-element accesses
// (launch_thresh's `vec` rule; n % 8 == 0 says nothing about a sample of a batch -- 4 x 10 elements).  The thresholded DENOISE stage (denoise_to_zero: x_out = the thresholded x0) is taken too -- the fused
// streaming families have no such form, but the kernel's run-time form does, and a pool of 12288-element rows has no
// workspace for that last stage's own clustered launch: its buffers are checked as LIN1's.
inline bool thresh_row_ok(const dpm_stage& st, const dpm_buffers& b) {
  if (!(st.flags & DPM_F_THRESH) || (st.flags & (DPM_F_BLEND | DPM_F_NOISE))) return false;
  if (st.form != DPM_FORM_LIN1 && st.form != DPM_FORM_TWO && st.form != DPM_FORM_MS3 && st.form != DPM_FORM_DENOISE) return false;
  dpm_stage plain = st;
  plain.flags &= ~(uint32_t)DPM_F_THRESH;
  if (st.form == DPM_FORM_DENOISE) plain.form = DPM_FORM_LIN1;
  const int64_t per_sample = b.n / b.batch;
  return fusable_request(plain, b) && per_sample % 4 == 0 && per_sample <= THR_CHUNK_MAX;
}
// ... and the two scalars a group of them shares besides het_same_group's keys: bit patterns, so that a NaN groups with itself
inline bool thresh_same_group(const dpm_stage& s0, const dpm_stage& s) {
  return std::memcmp(&s0.thr_ratio, &s.thr_ratio, sizeof s.thr_ratio) == 0 && std::memcmp(&s0.thr_max, &s.thr_max, sizeof s.thr_max) == 0;
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_THRESH: ONE launch over a group's run of rows (device memory: what table_fill_rows wrote
// for the same st / bs), one workgroup per sample, dynamic LDS sized from the group's per_sample.  No workspace, no
// occupancy query, no device-wide chain: the workgroups wait for nobody.  Tuning::force_generic is not read: as in the
// lockstep HOT = 3 kernel, whose ThrParams.fastdiv is x0_prologue_ok whatever the tuning (there the knob only picks HOT 3 over
// HOT 1), the prologue of a row is what its stage record says -- either way the same bits.
template <typename TS, typename TE>
int launch_table_thresh_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const LaunchCtx& c) {
  const int64_t batch = bs[0].batch, per_sample = bs[0].n / bs[0].batch;
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n) || (int64_t)n_req * batch > 0x7fffffff)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  for (int r = 0; r < n_req; ++r)
    if (!thresh_row_ok(st[r], bs[r]) || !thresh_same_group(st[0], st[r]) || bs[r].n != bs[0].n || bs[r].batch != bs[0].batch)
      return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a stage that is no thresholded row of this group in a table thresholding launch");
  ThrLaunchPlan lp = thr_launch_plan(st[0], (int64_t)n_req * batch, per_sample, 1, ThrKnobs{0, 0}, false, true, false, true);
  if (lp.err || lp.k != 1) return dpm_set_error(DPM_ERR_UNSUPPORTED, "thresholding: batch / sample size out of range");
  lp.tp.bpr = (int32_t)batch;
  lp.tp.groups = lp.tp.batch;
  const TableRow* tab = static_cast<const TableRow*>(rows);
  const dim3 grid((unsigned)lp.tp.batch), block(THR_THREADS);
  if (st[0].guidance == DPM_GUIDE_CFG)
    launch(stage_thresh_kernel_table<TS, TE, DPM_GUIDE_CFG>, grid, block, lp.lds_bytes, c, tab, lp.tp);
  else
    launch(stage_thresh_kernel_table<TS, TE, DPM_GUIDE_NONE>, grid, block, lp.lds_bytes, c, tab, lp.tp);
  return launch_status("table thresholding kernel launch failed");
}

}  // namespace

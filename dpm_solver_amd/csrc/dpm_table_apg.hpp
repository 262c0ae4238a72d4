// dpm_table_apg.hpp -- adaptive-projected-guidance rows of the table-driven launch (DPM_TABLE_APG): stage_apg_kernel_table and
// its launcher.  Included by unit F of dpm_stage_unit.hip behind dpm_sample_frame.hpp and dpm_apg_kernel.hpp and by nothing
// else.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A request under adaptive projected guidance used to leave continuous batching: stage_apg_kernel takes ONE stage record per
// launch, so 256 staggered single-image requests were 256 launches of one workgroup each per tick.  As for guidance rescale
// (dpm_table_rescale.hpp) a table row is one request of a few samples, and the lone kernel already gives a sample to ONE
// workgroup that waits for nobody: here workgroup blockIdx.x advances sample blockIdx.x - r * bpr of row r = blockIdx.x / bpr
// -- the SAME source, apg_sample, on the row's pointers, the row's stage scalars and the row's APG record.  Row and record
// are read IN PLACE through the two const __restrict__ table pointers with the wave-uniform r (scalar loads, as
// stage_kernel_table_blend reads its blend record; the kernel never writes the table, and no row is copied into a local
// KParams -- see the comment above HetArgs): the 8 pointers, the form, model type and prologue (FORM_RT, PM_RT), the
// coefficients, the guidance scale, DPM_F_STORE_M and the duplicate store from the row; eta, r, beta and the running average
// from the record (KApgTab, dpm_table_kernel.hpp: KParams does not carry the three scalars under the flag).  What APG has
// and rescale has not is state that persists per request: with a momentum the record points at the row's running average,
// [bpr, per] fp32, and the sample's workgroup reads, updates and stores its own slice of it (avg + sample * per) -- nobody
// else touches that slice in this launch.  A null average is a row without a momentum: MOM is workgroup-uniform, so rows with
// and without one share a launch, as the four forms do.  What a group shares travels in the kernel arguments: per = the
// elements of a sample, bpr = the samples per row (het_same_group keys on n and batch).  The grid is exactly the group's
// samples: no workgroup returns before the barrier, every thread reaches it.  Only the 16-byte access path exists here
// (VEC = true; apg_row_ok admits nothing else), with both the register and the re-read path.
// Every sample gets the bits of its request's own launch: the sums are added in the same order by the same source.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TE>
__global__ __launch_bounds__(SF_THREADS) void stage_apg_kernel_table(const TableRow* __restrict__ rows,
                                                                     const KApgTab* __restrict__ recs, int64_t per, uint32_t bpr) {
  __shared__ double red[SF_WAVES * 3];
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / bpr));
  const int64_t base = (int64_t)(blockIdx.x - r * bpr) * per;  // this workgroup's sample of row r
  const TableRow& row = rows[r];
  const KApgTab& rec = recs[r];
  const KParams& p = row.p;
  const ApgScalars a{rec.eta, rec.r, rec.beta};
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
  TS* xo2 = (TS*)row.xo2;
  float* avg = (float*)rec.avg;
  x += base;  // (a plain request: the state is there, and it is the evaluation state)
  e0 += base;
  e1 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  if (xo2) xo2 += base;
  if (avg) avg += base;
  if (per <= SF_KEEP_MAX) {
    if (avg) apg_sample<true, true, true>(x, x, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);
    else apg_sample<true, true, false>(x, x, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);
  } else {
    if (avg) apg_sample<true, false, true>(x, x, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);
    else apg_sample<true, false, false>(x, x, e0, e1, h1, h2, xo, mo, xo2, avg, per, p, a, red);
  }
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_APG: ONE launch over a group's run of rows and their records (device memory: what
// table_fill_rows and table_fill_apg wrote for the same st / bs), one workgroup per sample.  No workspace, no occupancy
// query, nothing to wait for.
template <typename TS, typename TE>
int launch_table_apg_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs,
                           const LaunchCtx& c) {
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n) || bs[0].batch < 1 || (int64_t)n_req * bs[0].batch > 0x7fffffff)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  for (int r = 0; r < n_req; ++r)
    if (!apg_row_ok(st[r], bs[r]) || bs[r].n != bs[0].n || bs[r].batch != bs[0].batch)
      return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a stage that is no adaptive-projected-guidance row of this group in a table APG launch");
  const int64_t batch = bs[0].batch, per = bs[0].n / batch;
  launch(stage_apg_kernel_table<TS, TE>, dim3((unsigned)((int64_t)n_req * batch)), dim3(SF_THREADS), 0, c,
         static_cast<const TableRow*>(rows), static_cast<const KApgTab*>(recs), per, (uint32_t)batch);
  return launch_status("table APG stage kernel launch failed");
}

}  // namespace

// dpm_table_zstar.hpp -- CFG-Zero* rows of the table-driven launch (DPM_TABLE_ZSTAR): stage_zstar_kernel_table and its
// launcher.  Included by unit G of dpm_stage_unit.hip behind dpm_sample_frame.hpp and dpm_zstar_kernel.hpp and by nothing
// else.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A request under CFG-Zero* used to leave continuous batching: stage_zstar_kernel takes ONE stage record per launch, so 256
// staggered single-image requests were 256 launches of one workgroup each per tick.  A table row is one request of a few
// samples, and the lone kernel already gives a sample to ONE workgroup that waits for nobody: here workgroup blockIdx.x
// advances sample blockIdx.x - r * bpr of row r = blockIdx.x / bpr -- the SAME source, zstar_sample, on the row's pointers
// and record.  Everything per row comes from the row, read IN PLACE through the const __restrict__ table pointer with the
// wave-uniform r (scalar loads, as stage_rescale_kernel_table; the kernel never writes the table, and no row is copied into
// a local KParams -- see the comment above HetArgs): the 8 pointers, the form, model type and prologue (FORM_RT, PM_RT), the
// coefficients, the guidance scale, DPM_F_STORE_M and the duplicate store.  The kind has no record: the flag carries no
// parameter of its own and no state from stage to stage.  What a group shares travels in the kernel arguments: per = the
// elements of a sample, bpr = the samples per row (het_same_group keys on n and batch).  The grid is exactly the group's
// samples: no workgroup returns before the barrier, every thread reaches it.  Only the 16-byte access path exists here
// (VEC = true; zstar_row_ok admits nothing else), with both the register and the re-read path.
// Every sample gets the bits of its request's own launch: the sums are added in the same order by the same source.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TE>
__global__ __launch_bounds__(SF_THREADS) void stage_zstar_kernel_table(const TableRow* __restrict__ rows, int64_t per, uint32_t bpr) {
  __shared__ double red[SF_WAVES * 2];
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / bpr));
  const int64_t base = (int64_t)(blockIdx.x - r * bpr) * per;  // this workgroup's sample of row r
  const TableRow& row = rows[r];
  const KParams& p = row.p;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
  TS* xo2 = (TS*)row.xo2;
  x += base;  // (a plain request: the state is there, and it is the evaluation state)
  e0 += base;
  e1 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  if (xo2) xo2 += base;
  if (per <= SF_KEEP_MAX) zstar_sample<true, true>(x, x, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
  else zstar_sample<true, false>(x, x, e0, e1, h1, h2, xo, mo, xo2, per, p, red);
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_ZSTAR: ONE launch over a group's run of rows (device memory: what table_fill_rows wrote
// for the same st / bs), one workgroup per sample.  No workspace, no occupancy query, nothing to wait for.
template <typename TS, typename TE>
int launch_table_zstar_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const LaunchCtx& c) {
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n) || bs[0].batch < 1 || (int64_t)n_req * bs[0].batch > 0x7fffffff)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  for (int r = 0; r < n_req; ++r)
    if (!zstar_row_ok(st[r], bs[r]) || bs[r].n != bs[0].n || bs[r].batch != bs[0].batch)
      return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a stage that is no CFG-Zero* row of this group in a table CFG-Zero* launch");
  const int64_t batch = bs[0].batch, per = bs[0].n / batch;
  launch(stage_zstar_kernel_table<TS, TE>, dim3((unsigned)((int64_t)n_req * batch)), dim3(SF_THREADS), 0, c,
         static_cast<const TableRow*>(rows), per, (uint32_t)batch);
  return launch_status("table CFG-Zero* stage kernel launch failed");
}

}  // namespace

// dpm_table_perp.hpp -- Perp-Neg rows of the table-driven launch (DPM_TABLE_PERP): stage_perp_kernel_table and its launcher.
// Included by unit J of dpm_stage_unit.hip behind dpm_sample_frame.hpp and dpm_perp_kernel.hpp and by nothing else.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A Perp-Neg request used to leave continuous batching: stage_perp_kernel takes ONE stage record per launch, so 256 staggered
// single-image requests were 256 launches of one workgroup each per tick, each behind a torch.cat([x] * 3).  Both halves of the
// answer are older: stage_zstar_kernel_table gives one workgroup to every sample of a row, and stage_pair_kernel_table has the
// pair record and the three stores of the state.  Here workgroup blockIdx.x advances sample blockIdx.x - r * bpr of row
// r = blockIdx.x / bpr -- the SAME source as the lone kernel, perp_sample, on the row's pointers and records.  Row and pair record
// (KPairTab, dpm_table_kernel.hpp: the third output and the third copy) are read IN PLACE through the two const __restrict__
// table pointers with the wave-uniform r (scalar loads; the kernel never writes the table, and no row is copied into a local
// KParams -- see the comment above HetArgs): the 8 pointers, the form, model type and prologue (FORM_RT, PM_RT), the
// coefficients, s and w (cfg_scale, cg_scale) and DPM_F_STORE_M from the row.  What a group shares travels in the kernel
// arguments: per = the elements of a sample, bpr = the samples per row (het_same_group keys on n and batch).  The grid is exactly
// the group's samples: no workgroup returns before the barrier, every thread reaches it.  LDS is the lone kernel's: the 64 KiB
// park and the 128 bytes of the reduction.  Only the 16-byte access path exists here (VEC = true; perp_row_ok admits nothing
// else), the shipped register path (PERP_PARK) and the re-read path.
// Stores: x_out; where the row's xo2 is not null (workgroup-uniform) the two duplicates, xo2 and the record's xo3 -- the other
// two thirds of the network's next [3S, ...] input --, all three advanced to the workgroup's sample, by the store x_out itself
// gets (sf_store: store_pack<false, true>); m_out under DPM_F_STORE_M.
// Every sample gets the bits of its request's own launch: the sums are added in the same order by the same source.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TE>
__global__ __launch_bounds__(SF_THREADS) void stage_perp_kernel_table(const TableRow* __restrict__ rows,
                                                                      const KPairTab* __restrict__ recs, int64_t per, uint32_t bpr) {
  __shared__ double red[SF_WAVES * 2];
  __shared__ perp_f4 park[SF_KEEP_CHUNKS * 2 * SF_THREADS];
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / bpr));
  const int64_t base = (int64_t)(blockIdx.x - r * bpr) * per;  // this workgroup's sample of row r
  const TableRow& row = rows[r];
  const KPairTab& rec = recs[r];
  const KParams& p = row.p;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TE* e2 = (const TE*)rec.g;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
  TS* xo2 = (TS*)row.xo2;
  TS* xo3 = (TS*)rec.xo3;
  x += base;  // (a plain request: the state is there, and it is the evaluation state)
  e0 += base;
  e1 += base;
  e2 += base;
  if (h1) h1 += base;
  if (h2) h2 += base;
  xo += base;
  if (mo) mo += base;
  if (xo2) {  // (the copies come together: check_pair_copies, launch_table_perp_typed)
    xo2 += base;
    xo3 += base;
  }
  if (per <= SF_KEEP_MAX) perp_sample<true, true, PERP_PARK>(x, x, e0, e1, e2, h1, h2, xo, mo, per, p, red, park, xo2, xo3);
  else perp_sample<true, false, PERP_PARK>(x, x, e0, e1, e2, h1, h2, xo, mo, per, p, red, park, xo2, xo3);
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_PERP: ONE launch over a group's run of rows and their pair records (device memory: what
// table_fill_rows and table_fill_pair wrote for the same st / bs), one workgroup per sample.  No workspace, no occupancy query,
// nothing to wait for.
template <typename TS, typename TE>
int launch_table_perp_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs,
                            const LaunchCtx& c) {
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n) || bs[0].batch < 1 || (int64_t)n_req * bs[0].batch > 0x7fffffff)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  for (int r = 0; r < n_req; ++r)
    if (!perp_row_ok(st[r], bs[r]) || bs[r].n != bs[0].n || bs[r].batch != bs[0].batch ||
        (bs[r].x_out2 != nullptr) != (bs[r].thr_hint != nullptr))
      return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a stage that is no Perp-Neg row of this group in a table Perp-Neg launch");
  const int64_t batch = bs[0].batch, per = bs[0].n / batch;
  launch(stage_perp_kernel_table<TS, TE>, dim3((unsigned)((int64_t)n_req * batch)), dim3(SF_THREADS), 0, c,
         static_cast<const TableRow*>(rows), static_cast<const KPairTab*>(recs), per, (uint32_t)batch);
  return launch_status("table Perp-Neg stage kernel launch failed");
}

}  // namespace

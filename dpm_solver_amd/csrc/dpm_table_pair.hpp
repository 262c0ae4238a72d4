// dpm_table_pair.hpp -- two-condition rows of the table-driven launch (DPM_TABLE_PAIR): stage_pair_kernel_table, its pair record
// and its launcher.  Included by unit H of dpm_stage_unit.hip behind dpm_pair_kernel.hpp and by nothing else.
#pragma once

namespace {

// (The pair record, KPairTab, and its fill are host-visible and sit beside the APG record's in dpm_table_kernel.hpp.)
// tiles per super-tile: 1 for every dtype pair.  TableShape's own value (2 for a 4-byte state) and 1 were both built and timed on
// an MI355X (profiles/r31_slab_pair.md, section 3): 1 is the faster for either state width.  -DDPM_TABLE_PAIR_U=<1|2> rebuilds
// the other for that comparison.
#ifndef DPM_TABLE_PAIR_U
#define DPM_TABLE_PAIR_U 1
#endif
constexpr int PAIR_TABLE_U = DPM_TABLE_PAIR_U;

// ------------------------------------------------------------------------------------------------
// A request under guidance over two conditions used to leave continuous batching: stage_pair_kernel takes ONE stage record
// per launch, so 256 staggered single-image requests were 256 launches per tick, each behind a torch.cat([x] * 3).  Here the
// launch has the plain table family's shape (stage_kernel_table): one n per launch, r = v / spr, one super-tile of U tiles per
// 256-lane group, no loop over the grid, the XCD-contiguous remap.  Row and pair record are read IN PLACE through the two const
// __restrict__ table pointers with the wave-uniform r (scalar loads; the kernel never writes the table, and no row is copied
// into a local KParams -- see the comment above HetArgs): the 8 pointers, the form, model type and prologue (FORM_RT, PM_RT), the
// coefficients, the two scales (cfg_scale, cg_scale) and DPM_F_STORE_M from the row; the third output and the third copy from
// the record.
// Per element the arithmetic is the lone kernel's 16-byte route: pair_model, then combine_any<FORM_RT> with hm = false, on
// load_pack<true> loads.  There is no reduction, so every element gets the bits of its request's own stage_pair_kernel launch
// whatever the tile shape.  Lanes past the end of the last tile load a clamped (valid) group and only skip the stores.
// Stores: x_out; where the row's xo2 is not null (wave-uniform) the two duplicates, xo2 and xo3 -- the other two thirds of the
// network's next [3S, ...] input --; m_out under DPM_F_STORE_M.  The duplicates take the policy stage_tiles gives its DUP store,
// which is the policy of x_out itself (nt mask bit 1 clear, written through where the build writes through): a 2-byte state
// leaves written through, a 4-byte state's two 16-byte halves stay cached stores that L2 merges (store_pack).
// A row is a plain request (pair_row_ok): the state is the evaluation state.  Only the 16-byte route exists here.
// ------------------------------------------------------------------------------------------------
template <typename TS, typename TE, int U>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_pair_kernel_table(const TableRow* __restrict__ rows,
                                                                             const KPairTab* __restrict__ recs, int64_t n,
                                                                             uint32_t nreq, uint32_t spr, uint32_t xcd_span) {
  const int64_t ngroups = n / EPT;
  const int64_t ntiles = (ngroups + 255) / 256;
  const uint32_t total = nreq * spr;
  const uint32_t per = blockDim.x >> 8;
  const uint32_t sub = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
  const uint32_t b = blockIdx.x;
  const uint32_t in_xcd = (b >> 3) * per + sub;
  if (xcd_span && in_xcd >= xcd_span) return;
  const uint32_t v = xcd_span ? (b & 7u) * xcd_span + in_xcd : b * per + sub;
  if (v >= total) return;
  const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v / spr));
  const int64_t t0 = (int64_t)(v - r * spr) * U;
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
  const bool need_xe = (p.flags & DPM_F_TO_X0) || p.model_type == DPM_MODEL_X_START || p.model_type == DPM_MODEL_V;
  const bool nx = form_needs_x<FORM_RT>(p), nh1 = form_needs_h1<FORM_RT>(p), nh2 = form_needs_h2<FORM_RT>(p);
  const bool store_m = (p.flags & DPM_F_STORE_M) != 0;
  const bool ld_x = nx || need_xe;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t t = t0 + u;
    if (t >= ntiles) break;  // (wave-uniform: the last super-tile of a row may be short)
    const int64_t gr = t * 256 + tile_lane();
    const int64_t gi = gr < ngroups ? gr : ngroups - 1;
    float vx[EPT], v0[EPT], v1[EPT], v2[EPT], vh1[EPT], vh2[EPT], ox[EPT], om[EPT];
    if (ld_x) load_pack<true>(x, gi, vx);
    load_pack<true>(e0, gi, v0);
    load_pack<true>(e1, gi, v1);
    load_pack<true>(e2, gi, v2);
    if (nh1) load_pack<true>(h1, gi, vh1);
    if (nh2) load_pack<true>(h2, gi, vh2);
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const float xv = ld_x ? vx[j] : 0.f;
      const float xev = need_xe ? xv : 0.f;
      const float mn = pair_model(v0[j], v1[j], v2[j], xev, p);
      om[j] = mn;
      ox[j] = combine_any<FORM_RT, float, TE>(nx ? xv : 0.f, mn, nh1 ? vh1[j] : 0.f, nh2 ? vh2[j] : 0.f, p, false);
    }
    if (gr < ngroups) {
      store_pack<false, true>(xo, gi, ox);
      if (xo2) {
        store_pack<false, true>(xo2, gi, ox);
        store_pack<false, true>(xo3, gi, ox);
      }
      if (store_m) store_pack<false, true>(mo, gi, om);
    }
  }
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_PAIR: ONE launch over a group's run of rows and their pair records (device memory: what
// table_fill_rows and table_fill_pair wrote for the same st / bs).  launch_table_rows' checks and fused_grid's shape at this
// kernel's own U; the kernel has one instantiation per dtype pair, so there is no prologue or guidance flag to dispatch on.
template <typename TS, typename TE>
int launch_table_pair_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs,
                            const LaunchCtx& c) {
  constexpr int U = PAIR_TABLE_U;
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  for (int r = 0; r < n_req; ++r)
    if (!pair_row_ok(st[r], bs[r]) || bs[r].n != bs[0].n || (bs[r].x_out2 != nullptr) != (bs[r].thr_hint != nullptr))
      return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: a stage that is no two-condition row of this group in a table pair launch");
  const FusedShape sh = fused_grid<TS, TE>(bs[0].n, n_req, U, tuning_for(bs[0].opts), false);
  launch(stage_pair_kernel_table<TS, TE, U>, sh.grid, sh.block, 0, c, static_cast<const TableRow*>(rows),
         static_cast<const KPairTab*>(recs), bs[0].n, (uint32_t)n_req, sh.spr, sh.xcd_span);
  return launch_status("table two-condition stage kernel launch failed");
}

}  // namespace

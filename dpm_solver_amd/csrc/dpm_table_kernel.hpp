// dpm_table_kernel.hpp -- the table-driven heterogeneous fused stage (dpm_launch_opts.table_mode): stage_kernel_het /
// stage_kernel_het_unipc / stage_kernel_het_noise with their per-request records in DEVICE memory instead of the kernel
// arguments, and their launchers (part of dpm_device.hpp; include that)
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// A server's common case is hundreds of requests of one or a few images each.  The heterogeneous kernels keep their records
// in the kernel arguments -- HET_MAX = 16 per launch, HIP's 4 KiB -- so 256 single-image requests advance as 16 launches of
// half a megabyte each, every one of them latency-bound.  Here request r's record is row r of a table in global memory: a
// kernel-argument pointer to fixed-size rows, the 8 pointers in HetArgs order, then the KParams (make_params, as for every
// other launch).  The host fills the table (DPM_TABLE_FILL, no HIP call), the CALLER copies it to the device, and
// DPM_TABLE_LAUNCH launches one kernel over a run of rows, whatever their number.
// Everything else is stage_kernel_het's: one n per launch, r = v / spr, one super-tile per 256-lane group, no loop, MultiShape's
// tiles and cache policy, the XCD-contiguous remap, stage_tiles called with the request's pointers and record -- every request
// gets the bits of its own single launch.
// The row is read IN PLACE through the const __restrict__ table pointer with the wave-uniform r: every field is a scalar
// load (the kernel never writes the table, and writes nothing with scalar instructions).  No row is expanded into a local
// KParams: see the comment above HetArgs on what the backend does with such a copy.
// ------------------------------------------------------------------------------------------------
// A pointer loaded from the kernarg segment is known to the compiler to be a global one; a plain `void*` loaded from a table
// in global memory is a flat one, and every access through it a flat_load / flat_store (two counters to wait on, an
// aperture check per access).  The rows hold device-memory pointers only, and their fields say so: the tile body's accesses
// are stage_kernel_het's global_load / global_store again.
#define DPM_GLOBAL_PTR __attribute__((address_space(1)))
struct TableRow {
  const DPM_GLOBAL_PTR void* x;
  const DPM_GLOBAL_PTR void* e0;
  const DPM_GLOBAL_PTR void* e1;
  const DPM_GLOBAL_PTR void* h1;
  const DPM_GLOBAL_PTR void* h2;
  DPM_GLOBAL_PTR void* xo;
  DPM_GLOBAL_PTR void* mo;
  DPM_GLOBAL_PTR void* xo2;  // classifier-free guidance: the second half of the [2B, ...] network input (or null)
  KParams p;
};
static_assert(sizeof(TableRow) == DPM_TABLE_ROW_BYTES && sizeof(TableRow) % 16 == 0,
              "include/dpm_hip.h documents the table row: 8 pointers, then 20 words of stage scalars");
// the smallest group that takes the table family: one more than the kernarg records hold.  Groups of 2..HET_MAX keep
// stage_kernel_het, whose records need no dependent global load in front of the tile's own.
constexpr int TABLE_MIN = HET_MAX + 1;
// an nt-mask bit stage_tiles does not read (see NT_SHAPES): these kernels get tile bodies of their own, and the kernels a
// pool without a table was measured with keep their listings
constexpr int NT_TABLE = 32;

// FORMS = HET_FORMS_2 or HET_FORMS_3, as stage_kernel_het
template <typename TS, typename TE, unsigned FORMS, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_table(const TableRow* __restrict__ rows, int64_t n,
                                                                        uint32_t nreq, uint32_t spr, uint32_t xcd_span) {
  const int64_t ngroups = n / EPT;
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
  const KParams& p = row.p;
  constexpr bool DUP = GUIDE == DPM_GUIDE_CFG;
  KExt ext = {};
  if constexpr (DUP) ext.xo2 = (void*)row.xo2;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
#define DPM_TABLE_TILES(F_) \
  stage_tiles<TS, TE, F_, GUIDE, false, SPEC, U, NT, DUP>(x, nullptr, e0, e1, nullptr, h1, h2, xo, mo, ngroups, t0, p, ext)
  switch (p.form) {
    case DPM_FORM_LIN1: DPM_TABLE_TILES(DPM_FORM_LIN1); break;
    case DPM_FORM_TWO: DPM_TABLE_TILES(DPM_FORM_TWO); break;
    case DPM_FORM_MS3:
      if constexpr ((FORMS >> DPM_FORM_MS3) & 1u) DPM_TABLE_TILES(DPM_FORM_MS3);
      break;
    default: break;  // (the host groups only forms of FORMS)
  }
#undef DPM_TABLE_TILES
}

// {LIN1, TWO, UNIPC}, as stage_kernel_het_unipc: the UniPC sub-shapes are wave-uniform bits of the row's record
template <typename TS, typename TE, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_table_unipc(const TableRow* __restrict__ rows, int64_t n,
                                                                              uint32_t nreq, uint32_t spr, uint32_t xcd_span) {
  static_assert(GUIDE != DPM_GUIDE_CLASSIFIER, "unipc: no classifier guidance");
  const int64_t ngroups = n / EPT;
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
  const KParams& p = row.p;
  constexpr bool DUP = GUIDE == DPM_GUIDE_CFG;
  KExt ext = {};
  if constexpr (DUP) ext.xo2 = (void*)row.xo2;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  const TS* h2 = (const TS*)row.h2;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
#define DPM_TABLE_TILES(F_) \
  stage_tiles<TS, TE, F_, GUIDE, false, SPEC, U, NT, DUP>(x, nullptr, e0, e1, nullptr, h1, h2, xo, mo, ngroups, t0, p, ext)
  switch (p.form) {
    case DPM_FORM_LIN1: DPM_TABLE_TILES(DPM_FORM_LIN1); break;
    case DPM_FORM_TWO: DPM_TABLE_TILES(DPM_FORM_TWO); break;
    case DPM_FORM_UNIPC: DPM_TABLE_TILES(DPM_FORM_UNIPC); break;
    default: break;  // (the host groups LIN1 / TWO / UNIPC only)
  }
#undef DPM_TABLE_TILES
}

// SDE rows (DPM_TABLE_NOISE): stage_kernel_table with the form set {LIN1, TWO} and stage_kernel_het_noise's epilogue.  The row
// has no room for the request's KNoise, so the noise records are a second array in device memory, record i beside row i --
// a second const __restrict__ kernel-argument pointer indexed by the same wave-uniform r: scalar loads, like the row.  The
// record carries what no kernel-argument launch can: the base g0 of the row's Philox block indices (KNoiseTab), which makes
// a row one SAMPLE of a request whose other samples sit in other, non-adjacent rows -- each with the z of its own elements.
// g0 = 0 gives the bits of stage_kernel_het_noise.  Its own family, so that stage_kernel_table stays as it is.
static_assert(sizeof(KNoiseTab) == DPM_TABLE_NOISE_BYTES, "include/dpm_hip.h publishes the noise record's size");
template <typename TS, typename TE, int GUIDE, int SPEC, int U, int NT>
__global__ __launch_bounds__(STAGE_MAX_THREADS) void stage_kernel_table_noise(const TableRow* __restrict__ rows,
                                                                              const KNoiseTab* __restrict__ nzs, int64_t n,
                                                                              uint32_t nreq, uint32_t spr, uint32_t xcd_span) {
  static_assert(GUIDE != DPM_GUIDE_CLASSIFIER, "noise: no classifier guidance");
  const int64_t ngroups = n / EPT;
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
  const KParams& p = row.p;
  const KNoise* nz = &nzs[r];
  constexpr bool DUP = GUIDE == DPM_GUIDE_CFG;
  KExt ext = {};
  if constexpr (DUP) ext.xo2 = (void*)row.xo2;
  const TS* x = (const TS*)row.x;
  const TE* e0 = (const TE*)row.e0;
  const TE* e1 = (const TE*)row.e1;
  const TS* h1 = (const TS*)row.h1;
  TS* xo = (TS*)row.xo;
  TS* mo = (TS*)row.mo;
#define DPM_TABLE_TILES(F_)                                                                                                   \
  stage_tiles<TS, TE, F_, GUIDE, false, SPEC, U, NT, DUP, false, true, true>(x, nullptr, e0, e1, nullptr, h1, nullptr, xo, mo, \
                                                                             ngroups, t0, p, ext, nullptr, nz)
  switch (p.form) {
    case DPM_FORM_LIN1: DPM_TABLE_TILES(DPM_FORM_LIN1); break;
    case DPM_FORM_TWO: DPM_TABLE_TILES(DPM_FORM_TWO); break;
    default: break;  // (the host groups LIN1 / TWO only)
  }
#undef DPM_TABLE_TILES
}

// the most members a table group of n-element requests may have: the launch's super-tiles (and its workgroups, eight
// XCD spans rounded up) stay below 2^31.  Counted at one tile per super-tile, whatever the pair's U: one rule for every dtype.
inline int64_t table_group_cap(int64_t n) {
  const int64_t spr = (n / EPT + 255) / 256;
  return std::max<int64_t>(1, (((int64_t)1 << 31) - 16) / std::max<int64_t>(spr, 1));
}

// ---- DPM_TABLE_FILL: the rows of one group (grouped by the caller as for launch_het_typed), members in call order.  Host
// memory, no HIP call.
inline void table_fill_rows(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* rows) {
  TableRow* out = static_cast<TableRow*>(rows);
  for (int r = 0; r < n_req; ++r) {
    TableRow row;
    std::memset(&row, 0, sizeof row);
    const void* const ptrs[8] = {bs[r].x, bs[r].e0, bs[r].e1, bs[r].h1, bs[r].h2, bs[r].x_out, bs[r].m_out, bs[r].x_out2};
    static_assert(offsetof(TableRow, p) == sizeof ptrs, "a row is its 8 pointers, then the stage scalars");
    std::memcpy(&row, ptrs, sizeof ptrs);
    row.p = make_params(&st[r]);
    std::memcpy(&out[r], &row, sizeof row);
  }
}

// ---- DPM_TABLE_FILL | DPM_TABLE_NOISE: the noise records of one group of SDE rows, beside its rows (same order).  The seed
// from the request's own options, counter and scale from its stage (noise_of), the base from dpm_buffers.noise_sample0 --
// checked by the caller: >= 0, a whole number of Philox blocks.
inline void table_fill_noise(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* recs) {
  KNoiseTab* out = static_cast<KNoiseTab*>(recs);
  for (int r = 0; r < n_req; ++r) {
    KNoiseTab nz;
    std::memset(&nz, 0, sizeof nz);
    static_cast<KNoise&>(nz) = noise_of(st[r], bs[r]);
    nz.g0 = (uint64_t)bs[r].noise_sample0 * (uint64_t)(bs[r].n / bs[r].batch) / 4u;
    std::memcpy(&out[r], &nz, sizeof nz);
  }
}

// ---- The APG record of a DPM_TABLE_APG call (include/dpm_hip.h, "Table mode"; read by stage_apg_kernel_table,
// dpm_table_apg.hpp): what a DPM_F_CFG_APG row needs beyond its row.  KParams does not carry cg_scale / thr_ratio / thr_max
// under the flag, so eta, r and beta travel here, with the running average -- declared in the global address space as
// KBlendTab's pointers are and for the same reason: a plain pointer loaded from the table would make every access to the
// average a flat one.  Null: the row has no momentum.
struct alignas(16) KApgTab {
  DPM_GLOBAL_PTR float* avg;
  float eta, r, beta;  // dpm_stage.cg_scale / thr_ratio / thr_max
  uint32_t pad[3];     // (zero)
};
static_assert(sizeof(KApgTab) == DPM_TABLE_APG_BYTES && alignof(KApgTab) == 16,
              "include/dpm_hip.h publishes the APG record's size: the average, 3 scalars, 3 zero words");

// ---- DPM_TABLE_FILL | DPM_TABLE_APG: the APG records of one group of APG rows, beside its rows (same order).  The average
// of such a call is the request's thr_hint (checked by the caller: not null where beta != 0).  Host memory, no HIP call.
inline void table_fill_apg(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* recs) {
  KApgTab* out = static_cast<KApgTab*>(recs);
  for (int r = 0; r < n_req; ++r) {
    KApgTab a;
    std::memset(&a, 0, sizeof a);
    const void* const avg = st[r].thr_max != 0.f ? bs[r].thr_hint : nullptr;
    static_assert(offsetof(KApgTab, eta) == sizeof avg, "an APG record starts with its pointer");
    std::memcpy(&a, &avg, sizeof avg);
    a.eta = st[r].cg_scale;
    a.r = st[r].thr_ratio;
    a.beta = st[r].thr_max;
    std::memcpy(&out[r], &a, sizeof a);
  }
}

// ---- The pair record of a DPM_TABLE_PAIR call (include/dpm_hip.h, "Table mode"; read by stage_pair_kernel_table,
// dpm_table_pair.hpp): what a DPM_GUIDE_CFG2 row needs beyond its row.  A row has 8 pointers; a two-condition stage reads a
// third network output and, in a slab pool, writes a third copy of the result (the network's next input is three copies of the
// state).  Both are declared in the global address space, as KApgTab's and KBlendTab's pointers are and for the reason given at
// DPM_GLOBAL_PTR: a plain pointer loaded from the table would make every access through it a flat one.
struct alignas(16) KPairTab {
  const DPM_GLOBAL_PTR void* g;  // the output under the second condition (dpm_buffers.g)
  DPM_GLOBAL_PTR void* xo3;      // the third copy of x_out (dpm_buffers.thr_hint in such a call), or null
};
static_assert(sizeof(KPairTab) == DPM_TABLE_PAIR_BYTES && alignof(KPairTab) == 16,
              "include/dpm_hip.h publishes the pair record's size: two pointers");

// ---- DPM_TABLE_FILL | DPM_TABLE_PAIR: the pair records of one group of two-condition rows, beside its rows (same order).  The
// third copy of such a call is the request's thr_hint (checked by the caller: set exactly where x_out2 is).  Host memory, no
// HIP call.
inline void table_fill_pair(const dpm_stage*, const dpm_buffers* bs, int n_req, void* recs) {
  KPairTab* out = static_cast<KPairTab*>(recs);
  for (int r = 0; r < n_req; ++r) {
    const void* const ptrs[2] = {bs[r].g, bs[r].thr_hint};
    static_assert(sizeof ptrs == sizeof(KPairTab), "a pair record is its two pointers");
    std::memcpy(&out[r], ptrs, sizeof ptrs);
  }
}

// ---- DPM_TABLE_LAUNCH: the skeleton of the streaming table launchers (plain / UniPC, noise and blend rows; the thresholded
// rows' launch has another shape, dpm_table_thresh.hpp).  The group's size against table_group_cap, the tuning, `row_ok(r)` for
// every member -- the kind's own argument check: `bad_row` is its error --, the prologue every member allows, the het kernels'
// launch shape (fused_grid), and ONE launch: `go(x0_, cfg_, shape)` names the kind's kernel for the two compile-time flags.
template <typename TS, typename TE>
struct TableShape {
  static constexpr int U = MultiShape<TS, TE>::U, NT = MultiShape<TS, TE>::NT | NT_TABLE;
};
template <typename TS, typename TE, typename RowOk, typename Go>
int launch_table_rows(const dpm_stage* st, const dpm_buffers* bs, int n_req, const char* bad_row, const char* failed, RowOk row_ok,
                      Go go) {
  if (n_req < 1 || (int64_t)n_req > table_group_cap(bs[0].n))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: %d requests in one table launch", n_req);
  const Tuning tn = tuning_for(bs[0].opts);
  bool x0 = !tn.force_generic;
  for (int r = 0; r < n_req; ++r) {
    if (!row_ok(r)) return dpm_set_error(DPM_ERR_ARG, "%s", bad_row);
    x0 = x0 && x0_prologue_ok(st[r]);
  }
  const FusedShape sh = fused_grid<TS, TE>(bs[0].n, n_req, TableShape<TS, TE>::U, tn, false);
  const bool cfg = st[0].guidance == DPM_GUIDE_CFG;
  with_flags(x0, cfg, [&](auto x0_, auto cfg_) { go(x0_, cfg_, sh); });
  return launch_status(failed);
}

// ---- DPM_TABLE_LAUNCH | DPM_TABLE_NOISE: ONE launch over a group of SDE rows and their noise records (device memory)
template <typename TS, typename TE>
int launch_table_noise_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs,
                             const LaunchCtx& c) {
  constexpr int U = TableShape<TS, TE>::U, NT = TableShape<TS, TE>::NT;
  const TableRow* tab = static_cast<const TableRow*>(rows);
  const KNoiseTab* nzs = static_cast<const KNoiseTab*>(recs);
  const int64_t n = bs[0].n;
  const uint32_t nreq = (uint32_t)n_req;
  return launch_table_rows<TS, TE>(
      st, bs, n_req, "stage_launch_multi: a stage that is no first- / second-order SDE stage in a table noise launch",
      "table noise stage kernel launch failed",
      [&](int r) { return (st[r].flags & DPM_F_NOISE) && (st[r].form == DPM_FORM_LIN1 || st[r].form == DPM_FORM_TWO); },
      [&](auto x0_, auto cfg_, const FusedShape& sh) {
        launch(stage_kernel_table_noise<TS, TE, guide_of(cfg_), spec_of(x0_), U, NT>, sh.grid, sh.block, 0, c, tab, nzs, n, nreq,
               sh.spr, sh.xcd_span);
      });
}

// ---- DPM_TABLE_LAUNCH: ONE launch over the group's run of rows (device memory: a byte copy of what table_fill_rows wrote for
// the same st / bs).  The prologue and the form set come from the host's records, as in launch_het_typed.  (The three
// families are named inside one with_flags body, so unit C's code object lays them out flag pair by flag pair.)
template <typename TS, typename TE>
int launch_table_typed(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const LaunchCtx& c) {
  constexpr int U = TableShape<TS, TE>::U, NT = TableShape<TS, TE>::NT;
  const TableRow* tab = static_cast<const TableRow*>(rows);
  const int64_t n = bs[0].n;
  const uint32_t nreq = (uint32_t)n_req;
  bool ms3 = false, unipc = false;
  return launch_table_rows<TS, TE>(
      st, bs, n_req, "stage_launch_multi: an SDE stage, or UniPC next to third-order stages, in a table launch",
      "table stage kernel launch failed",
      [&](int r) {
        ms3 = ms3 || st[r].form == DPM_FORM_MS3;
        unipc = unipc || st[r].form == DPM_FORM_UNIPC;
        return !(st[0].flags & DPM_F_NOISE) && !(unipc && ms3);
      },
      [&](auto x0_, auto cfg_, const FusedShape& sh) {
        constexpr int G = guide_of(cfg_), S = spec_of(x0_);
        if (unipc)
          launch(stage_kernel_table_unipc<TS, TE, G, S, U, NT>, sh.grid, sh.block, 0, c, tab, n, nreq, sh.spr, sh.xcd_span);
        else if (ms3)
          launch(stage_kernel_table<TS, TE, HET_FORMS_3, G, S, U, NT>, sh.grid, sh.block, 0, c, tab, n, nreq, sh.spr, sh.xcd_span);
        else
          launch(stage_kernel_table<TS, TE, HET_FORMS_2, G, S, U, NT>, sh.grid, sh.block, 0, c, tab, n, nreq, sh.spr, sh.xcd_span);
      });
}

}  // namespace

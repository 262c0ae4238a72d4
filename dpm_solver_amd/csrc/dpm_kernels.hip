// dpm_kernels.hip -- gfx950 (MI355X, CDNA4) device code of the DPM-Solver engine.
//
// C ABI entry points of the device side; the stage kernels live in dpm_device.hpp and are instantiated per dtype
// pair by dpm_stage_unit.hip.
#include "dpm_device.hpp"
#include "dpm_coef.hpp"

namespace dpmk {
// one context per device ordinal (dpm_device.hpp): the only state of the library that outlives a call
DeviceContext& device_context(int dev) {
  static DeviceContext ctx[64];
  return ctx[(dev < 0 ? 0 : dev) % 64];
}
uint32_t* cluster_fault_word(int dev, bool create) {
  DeviceContext& c = device_context(dev);
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.fault && create) {
    void* p = nullptr;
    // portable: a host of several devices (one thread per device) maps the word into every device's address space
    if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess && p) {
      c.fault = static_cast<uint32_t*>(p);
      *c.fault = 0u;
    }
  }
  return c.fault;
}
}  // namespace dpmk

namespace {
// The stage launchers of one dtype pair (dpm_stage_unit.hip, dpm_internal.hpp): unit A's and unit B's single-request
// launchers, unit A's fused multi-request one and unit B's heterogeneous ones.  One row per entry of DPM_PAIRS.
using UnitFn = int (*)(const dpm_stage*, const dpm_buffers*, void*, void*, void*, const dpm_stage*, const int32_t*,
                       const dpm_buffers*, int);
using FusedFn = int (*)(const dpm_stage*, const dpm_buffers*, int, void*, void*, void*);
using HetFn = int (*)(const dpm_stage*, const dpm_buffers*, int, void*);
// the one launch over a group's run of table rows and its records (null: the kind has none), both in device memory
using TableLaunchFn = int (*)(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
using SampleFn = int (*)(const dpm_stage*, const dpm_buffers*, void*, void*, void*);
struct PairUnits {
  int state_dtype, eps_dtype;
  UnitFn a, b;
  FusedFn fused;
  HetFn het;         // unit B's heterogeneous fused launcher (per-request stage records)
  HetFn het_shapes;  // ... and its mixed-shape sibling (dpm_launch_opts.fuse_shapes)
  // the table-driven launch (dpm_launch_opts.table_mode), one slot per row kind (kRowKinds): unit C's plain / UniPC, SDE and
  // thresholded rows, unit D's mask-blend rows, unit E's guidance-rescale rows, unit F's adaptive-projected-guidance rows,
  // unit G's CFG-Zero* rows
  TableLaunchFn table_launch, table_launch_noise, table_launch_thresh, table_launch_blend, table_launch_rescale, table_launch_apg,
      table_launch_zstar;
  // the per-sample guidance stages (kSampleGuidance): unit E's guidance rescale, unit F's adaptive projected guidance, unit G's
  // CFG-Zero*
  SampleFn rescale, apg, zstar;
  // unit H's stage under guidance over two conditions (DPM_GUIDE_CFG2): a streaming kernel of its own, and its rows of the
  // table (DPM_TABLE_PAIR)
  SampleFn pair;
  TableLaunchFn table_launch_pair;
  // unit I's Perp-Neg stage (DPM_F_CFG2_PERP under DPM_GUIDE_CFG2): one workgroup per sample, three network outputs, and
  // unit J's rows of the table for it (DPM_TABLE_PERP)
  SampleFn perp;
  TableLaunchFn table_launch_perp;
};
#define DPM_PAIR_ROW(name, TS, TE, SD, ED)                                                                  \
  {SD, ED, dpm_launch_unit<TS, TE, FORMS_A>, dpm_launch_unit<TS, TE, FORMS_B>, dpm_launch_fused<TS, TE>,   \
   dpm_launch_het<TS, TE>, dpm_launch_het_shapes<TS, TE>, dpm_table_launch<TS, TE>,                        \
   dpm_table_launch_noise<TS, TE>, dpm_table_launch_thresh<TS, TE>, dpm_table_launch_blend<TS, TE>,       \
   dpm_table_launch_rescale<TS, TE>, dpm_table_launch_apg<TS, TE>, dpm_table_launch_zstar<TS, TE>,         \
   dpm_launch_sample<TS, TE, DPM_F_CFG_RESCALE>, dpm_launch_sample<TS, TE, DPM_F_CFG_APG>,                 \
   dpm_launch_sample<TS, TE, DPM_F_CFG_ZSTAR>, dpm_launch_pair<TS, TE>, dpm_table_launch_pair<TS, TE>,  \
   dpm_launch_perp<TS, TE>, dpm_table_launch_perp<TS, TE>},
constexpr PairUnits kPairs[] = {DPM_PAIRS(DPM_PAIR_ROW)};
#undef DPM_PAIR_ROW

// the row of a (state, eps) dtype pair; nullptr: no stage kernels for it
const PairUnits* pair_of(int sd, int ed) {
  for (const PairUnits& p : kPairs)
    if (p.state_dtype == sd && p.eps_dtype == ed) return &p;
  return nullptr;
}

// the unit that builds a stage's update form: B for FORMS_B, A for every other value (A reports an unknown form)
UnitFn unit_for(const PairUnits& p, int form) {
  return form >= 0 && form < 32 && ((FORMS_B >> form) & 1u) ? p.b : p.a;
}

// one stage of n_req requests in one launch, or MULTI_NOT_BUILT (no error set) when it has no fused variant
int launch_fused(const PairUnits& p, const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, void* ev_start,
                 void* ev_stop) {
  if ((st->flags & DPM_F_THRESH) && !(st->flags & DPM_F_BLEND))  // one thresholding launch over all requests' samples
    return unit_for(p, st->form)(st, bs, stream, ev_start, ev_stop, nullptr, nullptr, bs, n_req);
  return p.fused(st, bs, n_req, stream, ev_start, ev_stop);
}

// The per-sample guidance flags (include/dpm_hip.h): a stage under one of them is a launch of its own kernel, one workgroup
// per sample (dpm_sample_frame.hpp), never fused and never with device-resident coefficients.  What dpm_stage_launch asks of
// such a stage is check_sample_guidance on the flag's row.
struct SampleGuidance {
  unsigned flag;
  const char* name;                                      // ... in every message
  int min_per;                                           // the smallest sample, in elements
  unsigned banned;                                       // the flags its kernel has no path for
  const char* banned_text;                               // ... as the message lists them
  bool needs_x0;                                         // defined on the data prediction: DPM_F_TO_X0 is required
  const char* f64_text;                                  // the double state's refusal, in brackets
  // the checks of the flag's own fields; `hint`: the call carries DPM_TABLE_APG (an APG average is thr_hint there)
  int (*scalars)(const dpm_stage*, const dpm_buffers*, bool hint);
  SampleFn PairUnits::*launch;
};
int check_rescale_scalars(const dpm_stage* st, const dpm_buffers*, bool) {
  if (!(st->cg_scale > 0.f && st->cg_scale <= 1.f))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG_RESCALE with phi=%g (dpm_stage.cg_scale), which is not in (0, 1]", (double)st->cg_scale);
  return DPM_OK;
}
int check_apg_scalars(const dpm_stage* st, const dpm_buffers* b, bool hint) {
  const float eta = st->cg_scale, r = st->thr_ratio, beta = st->thr_max;
  if (!(eta >= 0.f && eta <= 1.f))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG_APG with eta=%g (dpm_stage.cg_scale), which is not in [0, 1]", (double)eta);
  if (!(r >= 0.f))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG_APG with a norm threshold of %g (dpm_stage.thr_ratio), which is not >= 0", (double)r);
  if (!(beta > -1.f && beta < 1.f))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG_APG with a momentum of %g (dpm_stage.thr_max), which is not in (-1, 1)", (double)beta);
  if (beta != 0.f && hint && !b->thr_hint)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: DPM_F_CFG_APG with a momentum in a DPM_TABLE_APG call needs the running average in dpm_buffers.thr_hint");
  if (beta != 0.f && !hint && !b->workspace)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG_APG with a momentum needs the running average in dpm_buffers.workspace");
  return DPM_OK;
}
int check_no_scalars(const dpm_stage*, const dpm_buffers*, bool) { return DPM_OK; }  // (DPM_F_CFG_ZSTAR reads cfg_scale alone)
// DPM_F_CFG_ZSTAR first: a record that sets it together with one of the two older flags is reported by its checks, and a record
// without it meets the rows it always met.  Then DPM_F_CFG_APG: a record that sets both older flags (eta shares cg_scale with
// phi) is reported by that flag's checks
constexpr SampleGuidance kSampleGuidance[] = {
    {DPM_F_CFG_ZSTAR, "DPM_F_CFG_ZSTAR", 1, DPM_F_CFG_RESCALE | DPM_F_CFG_APG | DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE,
     "guidance rescale, adaptive projected guidance, thresholding, mask blend or noise", false, "no double kernel",
     check_no_scalars, &PairUnits::zstar},
    {DPM_F_CFG_APG, "DPM_F_CFG_APG", 1, DPM_F_CFG_RESCALE | DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE,
     "guidance rescale, thresholding, mask blend or noise", true, "no double kernel", check_apg_scalars, &PairUnits::apg},
    {DPM_F_CFG_RESCALE, "DPM_F_CFG_RESCALE", 2, DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE, "thresholding, mask blend or noise", false,
     "no double rescale kernel", check_rescale_scalars, &PairUnits::rescale},
};
// the row of a stage's per-sample guidance flag; nullptr: it has none
const SampleGuidance* sample_guidance(unsigned flags) {
  // (a request without any of them -- every request of a plain tick -- is decided by one test, whatever the number of rows)
  if (!(flags & (DPM_F_CFG_ZSTAR | DPM_F_CFG_APG | DPM_F_CFG_RESCALE))) return nullptr;
  for (const SampleGuidance& g : kSampleGuidance)
    if (flags & g.flag) return &g;
  return nullptr;
}

// the checks of a stage under g.flag, in the order they speak (b->batch >= 1, n a multiple of it)
int check_sample_guidance(const SampleGuidance& g, const dpm_stage* st, const dpm_buffers* b, bool hint) {
  auto fail = [&](int code, const char* fmt, auto... args) { return dpm_set_error(code, fmt, g.name, args...); };
  const int64_t per = b->n / b->batch;
  if (st->guidance != DPM_GUIDE_CFG)
    return fail(DPM_ERR_ARG, "stage_launch: %s is valid under classifier-free guidance only (guidance %d)", st->guidance);
  if (b->n > 0 && per < g.min_per)  // (an empty batch is DPM_OK, as for every stage; its record is still checked)
    return fail(DPM_ERR_ARG, "stage_launch: %s needs samples of at least %d element%s (got %lld)", g.min_per,
                g.min_per == 1 ? "" : "s", (long long)per);
  if (const int rc = g.scalars(st, b, hint)) return rc;
  // (the kernel dispatches the form at run time and has no launcher per form to report it, as the flag-less path has)
  const bool known = st->form >= DPM_FORM_LIN1 && st->form <= DPM_FORM_UNIPC;
  if (g.needs_x0) {  // what the flag is defined on comes before what it is combined with
    if (!known) return dpm_set_error(DPM_ERR_ARG, "unknown update form %d", st->form);
    if (!(st->flags & DPM_F_TO_X0)) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: %s without DPM_F_TO_X0 (it is defined on the data prediction)");
  }
  if (st->flags & g.banned) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: %s with %s (flags %u)", g.banned_text, st->flags);
  if (st->form == DPM_FORM_UNIPC) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: %s on a DPM_FORM_UNIPC stage");
  if (!known) return dpm_set_error(DPM_ERR_ARG, "unknown update form %d", st->form);
  if (b->state_dtype == DPM_DTYPE_F64 || b->eps_dtype == DPM_DTYPE_F64)
    return fail(DPM_ERR_UNSUPPORTED, "stage_launch: %s with a double state (%s)", g.f64_text);
  if (b->eps_stride != 0 && b->eps_stride != per)
    return fail(DPM_ERR_UNSUPPORTED, "stage_launch: %s with eps_stride=%lld (a channel slice of a wider output)", (long long)b->eps_stride);
  return DPM_OK;
}

// What dpm_stage_launch asks of a stage under guidance over two conditions (DPM_GUIDE_CFG2, include/dpm_hip.h) before anything
// else of the record is read: its two scales, then what stage_pair_kernel has no path for (b->batch >= 1, n a multiple of it).
// A remedy flag has been reported by check_sample_guidance ("valid under classifier-free guidance only").  `copies`: the call
// carries DPM_TABLE_PAIR or DPM_TABLE_PERP, where a row stores x_out2 and a third copy (check_pair_copies decides there).
int check_pair_guidance(const dpm_stage* st, const dpm_buffers* b, bool copies) {
  auto fail = [](int code, const char* fmt, auto... args) { return dpm_set_error(code, fmt, args...); };
  if (!std::isfinite(st->cfg_scale) || !std::isfinite(st->cg_scale))
    return fail(DPM_ERR_ARG, "stage_launch: DPM_GUIDE_CFG2 with s1=%g (dpm_stage.cfg_scale), s2=%g (dpm_stage.cg_scale): both must be finite",
                (double)st->cfg_scale, (double)st->cg_scale);
  if (st->flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_USER_X0))
    return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with thresholding, mask blend, noise or a split stage (flags %u)", st->flags);
  if (st->form == DPM_FORM_UNIPC) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 on a DPM_FORM_UNIPC stage");
  if (st->form < DPM_FORM_LIN1 || st->form > DPM_FORM_UNIPC) return fail(DPM_ERR_ARG, "unknown update form %d", st->form);
  if (st->flags & (DPM_F_UNIPC_DP | DPM_F_UNIPC_P2 | DPM_F_STORE_XC))
    return fail(DPM_ERR_ARG, "stage_launch: DPM_F_UNIPC_* / DPM_F_STORE_XC are valid on DPM_FORM_UNIPC stages only (form %d)", st->form);
  if (b->x_out2 && !copies) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)");
  if (b->state_dtype == DPM_DTYPE_F64 || b->eps_dtype == DPM_DTYPE_F64)
    return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with a double state (no double kernel)");
  if (b->eps_stride != 0 && b->eps_stride != b->n / b->batch)
    return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with eps_stride=%lld (a channel slice of a wider output)", (long long)b->eps_stride);
  return DPM_OK;
}

// What dpm_stage_launch asks of DPM_F_CFG2_PERP (include/dpm_hip.h), behind the remedy flags' checks and behind
// check_pair_guidance: a record that is refused without the flag is refused by the same line with it.  `table`: the call is a
// table-mode one without DPM_TABLE_PERP (DPM_TABLE_PAIR rows have no per-sample pass).
int check_perp_flag(const dpm_stage* st, const dpm_buffers* b, bool table) {
  if (st->guidance != DPM_GUIDE_CFG2)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_CFG2_PERP is valid under DPM_GUIDE_CFG2 only (guidance %d)", st->guidance);
  if (table)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch_multi: DPM_F_CFG2_PERP in a table-mode call (the table's rows have no per-sample pass)");
  if (b->batch > (int64_t)0x7fffffff)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_F_CFG2_PERP with a batch of %lld (one workgroup per sample)", (long long)b->batch);
  return DPM_OK;
}

// The argument checks of one request (st and b not null): DPM_OK, or the error (dpm_set_error) of the first check that fails.
// base_ok: the call is a DPM_TABLE_NOISE one, whose SDE rows honour dpm_buffers.noise_sample0 (checked there, check_noise_base);
// apg_hint: it is a DPM_TABLE_APG one, where the running average of a DPM_F_CFG_APG request is thr_hint, not workspace;
// pair_copies: it is a DPM_TABLE_PAIR or DPM_TABLE_PERP one, where a DPM_GUIDE_CFG2 request may carry x_out2 (checked there,
// check_pair_copies); table: it is a table-mode one without DPM_TABLE_PERP, which takes no DPM_F_CFG2_PERP request
int check_stage_buffers(const dpm_stage* st, const dpm_buffers* b, bool base_ok = false, bool apg_hint = false,
                        bool pair_copies = false, bool table = false) {
  auto fail = [](int code, const char* fmt, auto... args) { return dpm_set_error(code, fmt, args...); };
  if (b->n < 0 || b->batch < 1 || (b->n % b->batch) != 0)
    return fail(DPM_ERR_ARG, "stage_launch: n=%lld is not a multiple of batch=%lld", (long long)b->n, (long long)b->batch);
  if (b->noise_sample0 != 0 && !base_ok)
    return fail(DPM_ERR_ARG, "stage_launch: noise_sample0=%d (honoured by the SDE rows of a DPM_TABLE_NOISE call only)",
                b->noise_sample0);
  if (const SampleGuidance* g = sample_guidance(st->flags))
    if (const int rc = check_sample_guidance(*g, st, b, apg_hint)) return rc;
  if (st->guidance == DPM_GUIDE_CFG2)
    if (const int rc = check_pair_guidance(st, b, pair_copies)) return rc;
  if (st->flags & DPM_F_CFG2_PERP)
    if (const int rc = check_perp_flag(st, b, table)) return rc;
  if (b->n == 0) return DPM_OK;  // empty batch: nothing to do (torch allows zero-sized tensors)
  const bool needs_x = st->form != DPM_FORM_DENOISE;
  const bool unipc = st->form == DPM_FORM_UNIPC;
  const bool needs_h1 = st->form == DPM_FORM_TWO || st->form == DPM_FORM_MS3 || st->form == DPM_FORM_SS3T || unipc;
  const bool needs_h2 = st->form == DPM_FORM_MS3 || st->form == DPM_FORM_SS3T || (unipc && (st->flags & DPM_F_UNIPC_DP));
  const bool need_xe = (st->flags & DPM_F_TO_X0) || st->model_type == DPM_MODEL_X_START || st->model_type == DPM_MODEL_V;
  if (!b->e0 || !b->x_out) return fail(DPM_ERR_ARG, "stage_launch: e0 / x_out must not be null");
  if ((needs_x || need_xe) && !b->x && !b->xe) return fail(DPM_ERR_ARG, "stage_launch: x is null");
  if (needs_x && !b->x) return fail(DPM_ERR_ARG, "stage_launch: x is null");
  if (needs_h1 && !b->h1) return fail(DPM_ERR_ARG, "stage_launch: form %d needs h1", st->form);
  if (needs_h2 && !b->h2) return fail(DPM_ERR_ARG, "stage_launch: form %d needs h2", st->form);
  if ((st->flags & DPM_F_STORE_M) && !b->m_out) return fail(DPM_ERR_ARG, "stage_launch: STORE_M without m_out");
  if (st->guidance == DPM_GUIDE_CFG && !b->e1) return fail(DPM_ERR_ARG, "stage_launch: CFG needs e1");
  if (st->guidance == DPM_GUIDE_CLASSIFIER && !b->g) return fail(DPM_ERR_ARG, "stage_launch: classifier guidance needs g");
  if (st->guidance == DPM_GUIDE_CFG2 && (!b->e1 || !b->g)) return fail(DPM_ERR_ARG, "stage_launch: DPM_GUIDE_CFG2 needs e1 and g");
  if (st->flags & DPM_F_BLEND) {
    if (!b->mask || !b->blend_a || b->mask_period < 1)
      return fail(DPM_ERR_ARG, "stage_launch: DPM_F_BLEND needs mask, blend_a and mask_period >= 1");
    if (b->n % b->mask_period != 0)
      return fail(DPM_ERR_ARG, "stage_launch: n=%lld is not a multiple of mask_period=%lld", (long long)b->n,
                  (long long)b->mask_period);
    if (b->mask_period >= ((int64_t)1 << 31) && b->mask_period != b->n)
      return fail(DPM_ERR_UNSUPPORTED, "stage_launch: a broadcast mask of 2^31 or more elements");
  }
  if (st->flags & DPM_F_NOISE) {  // the SDE epilogue exists in the streaming family's LIN1 / TWO kernels only
    if (st->form != DPM_FORM_LIN1 && st->form != DPM_FORM_TWO)
      return fail(DPM_ERR_ARG, "stage_launch: DPM_F_NOISE is valid on LIN1 / TWO stages only (form %d)", st->form);
    if (st->flags & DPM_F_THRESH)
      return fail(DPM_ERR_ARG, "stage_launch: DPM_F_NOISE with DPM_F_THRESH (the thresholding kernel has no noise epilogue)");
    if (b->state_dtype == DPM_DTYPE_F64 || b->eps_dtype == DPM_DTYPE_F64)
      return fail(DPM_ERR_ARG, "stage_launch: DPM_F_NOISE with a double state (no double noise kernel)");
  }
  if (unipc) {  // the UniPC form exists in the streaming family only, in the data-prediction form, on 2- and 4-byte states
    if (st->flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE | DPM_F_USER_X0 | DPM_F_BASE_HIST))
      return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_FORM_UNIPC with thresholding, mask blend, noise or a split stage (flags %u)",
                  st->flags);
    if (!(st->flags & DPM_F_TO_X0)) return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_FORM_UNIPC is the data-prediction form (DPM_F_TO_X0)");
    if (b->state_dtype == DPM_DTYPE_F64 || b->eps_dtype == DPM_DTYPE_F64)
      return fail(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_FORM_UNIPC with a double state (no double UniPC kernel)");
    if ((st->flags & DPM_F_STORE_XC) && !b->x_out2) return fail(DPM_ERR_ARG, "stage_launch: DPM_F_STORE_XC without x_out2");
  } else if (st->flags & (DPM_F_UNIPC_DP | DPM_F_UNIPC_P2 | DPM_F_STORE_XC)) {
    return fail(DPM_ERR_ARG, "stage_launch: DPM_F_UNIPC_* / DPM_F_STORE_XC are valid on DPM_FORM_UNIPC stages only (form %d)", st->form);
  }
  if (b->eps_stride != 0 && b->eps_stride < b->n / b->batch)
    return fail(DPM_ERR_ARG, "stage_launch: eps_stride=%lld is smaller than a sample (%lld elements)",
                (long long)b->eps_stride, (long long)(b->n / b->batch));
  return DPM_OK;
}

// the auxiliary launchers' element type: f(float{}), f(__half{}) or f(bf16_t{}) for a DPM_DTYPE_* code; any other code is
// `what`'s unsupported-dtype error
template <class F>
int with_elem_type(int dtype, const char* what, F&& f) {
  switch (dtype) {
    case DPM_DTYPE_F32: f(float{}); return DPM_OK;
    case DPM_DTYPE_F16: f(__half{}); return DPM_OK;
    case DPM_DTYPE_BF16: f(bf16_t{}); return DPM_OK;
  }
  return dpm_set_error(DPM_ERR_UNSUPPORTED, "%s: unsupported dtype %d", what, dtype);
}
}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
int dpm_stage_launch_dyn(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop,
                         const dpm_stage* dyn, const int32_t* skip) {
  if (!st || !b) return dpm_set_error(DPM_ERR_ARG, "stage_launch: null pointer");
  if (const int rc = check_stage_buffers(st, b)) return rc;
  if (b->n == 0) return DPM_OK;
  if (dyn && (st->flags & DPM_F_NOISE))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch: DPM_F_NOISE with device-resident coefficients");
  if (dyn && st->form == DPM_FORM_UNIPC)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_FORM_UNIPC with device-resident coefficients");
  const SampleGuidance* const g = sample_guidance(st->flags);
  if (dyn && g) return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: %s with device-resident coefficients", g->name);
  if (dyn && st->guidance == DPM_GUIDE_CFG2)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with device-resident coefficients");
  dpm_buffers bb = *b;
  if (!bb.x) bb.x = bb.xe;  // DENOISE form: only the evaluation state exists
  const int sd = bb.state_dtype, ed = bb.eps_dtype;
  if (sd == DPM_DTYPE_F64 || ed == DPM_DTYPE_F64) {  // double-precision state: one run-time dispatched kernel (dpm_f64.hip)
    if (sd != ed) return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: a double state needs double network outputs (state=%d eps=%d)", sd, ed);
    if (dyn) return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: device-resident coefficients with a double state");
    return dpm_launch_f64(st, &bb, stream, ev_start, ev_stop);
  }
  const PairUnits* p = pair_of(sd, ed);
  if (!p) return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: unsupported dtype pair state=%d eps=%d", sd, ed);
  if (g) return (p->*g->launch)(st, &bb, stream, ev_start, ev_stop);
  if (st->guidance == DPM_GUIDE_CFG2)  // (before the fused-shape test)
    return ((st->flags & DPM_F_CFG2_PERP) ? p->perp : p->pair)(st, &bb, stream, ev_start, ev_stop);
  // A LARGE launch takes the fused multi-request kernel's shape -- one workgroup per super-tile instead of a grid capped at 8
  // workgroups per CU walking the tiles in a loop, an XCD-contiguous tile mapping for 2-byte states, two tiles per workgroup
  // for 4-byte states -- as a "group" of one request (Tuning::big_tiles; the same arithmetic, the same bits).  Stages the fused
  // family does not build (thresholding, mask blend, classifier guidance, SS3T / DENOISE, unaligned or strided operands)
  // come back MULTI_NOT_BUILT and take the single-request path below.  SDE stages (DPM_F_NOISE) do not take it: a lone SDE
  // stage keeps stage_kernel_noise (the fused noise kernels serve dpm_stage_launch_multi).
  if (!dyn && !(st->flags & (DPM_F_THRESH | DPM_F_BLEND | DPM_F_NOISE))) {
    const int big = tuning_for(bb.opts).big_tiles;
    if (lone_takes_fused_shape(bb.n, big)) {
      const int rc = launch_fused(*p, st, &bb, 1, stream, ev_start, ev_stop);
      if (rc != MULTI_NOT_BUILT) return rc;
    }
  }
  return unit_for(*p, st->form)(st, &bb, stream, ev_start, ev_stop, dyn, skip, nullptr, 0);
}

int dpm_stage_launch_ev(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop) {
  return dpm_stage_launch_dyn(st, b, stream, ev_start, ev_stop, nullptr, nullptr);
}

extern "C" int dpm_stage_launch(const dpm_stage* st, const dpm_buffers* b, void* stream) {
  return dpm_stage_launch_ev(st, b, stream, nullptr, nullptr);
}

// One stage of n_req requests.  ev_start / ev_stop (optional) are arrays of n_req events: a fused launch of the
// requests [r0, r1) is bracketed by ev_start[r0] / ev_stop[r0] and fused_first[r] = r0 for its members (a request
// launched on its own has fused_first[r] = r), so the caller can spread the duration.
int dpm_stage_launch_multi_ev(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, void** ev_start,
                              void** ev_stop, int* fused_first) {
  if (!st || !bs || n_req < 1) return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: bad arguments");
  // every request is checked as dpm_stage_launch checks it before anything is launched: a call that reports a request's
  // error has written nothing, also when the requests take the one-by-one path below
  for (int r = 0; r < n_req; ++r)
    if (const int rc = check_stage_buffers(st, &bs[r])) return rc;
  int done = 0;  // requests already advanced by fused launches
  // a group fuses when its requests agree in size and dtypes; otherwise every request is launched on its own
  const PairUnits* p = pair_of(bs[0].state_dtype, bs[0].eps_dtype);
  // (SDE stages fuse like the others: stage_kernel_multi_noise, each request with the seed of its own bs[r].opts)
  bool fuse = p && n_req > 1 && bs[0].n > 0 && tuning_for(bs[0].opts).multi_fuse != 0;
  for (int r = 0; r < n_req && fuse; ++r)
    fuse = bs[r].n == bs[0].n && bs[r].batch == bs[0].batch && bs[r].state_dtype == bs[0].state_dtype &&
           bs[r].eps_dtype == bs[0].eps_dtype;
  for (int r0 = 0; fuse && r0 < n_req; r0 += MULTI_MAX) {
    const int cnt = std::min(MULTI_MAX, n_req - r0);
    const int rc = launch_fused(*p, st, bs + r0, cnt, stream, ev_start ? ev_start[r0] : nullptr, ev_stop ? ev_stop[r0] : nullptr);
    if (rc == MULTI_NOT_BUILT) break;  // no fused variant for this stage, or a buffer of this group is unaligned
    if (rc) return rc;
    if (fused_first)
      for (int r = r0; r < r0 + cnt; ++r) fused_first[r] = r0;
    done = r0 + cnt;
  }
  for (int r = done; r < n_req; ++r) {
    const int rc = dpm_stage_launch_ev(st, &bs[r], stream, ev_start ? ev_start[r] : nullptr, ev_stop ? ev_stop[r] : nullptr);
    if (rc) return rc;
    if (fused_first) fused_first[r] = r;
  }
  return DPM_OK;
}

namespace {
// May a request that passes fusable_request (dpm_launch.hpp) join the heterogeneous fused launch (stage_kernel_het) of
// request 0 of a group?  They must agree on the fields that are template arguments or kernel-wide scalars.  (Which of MS3
// and UNIPC a group takes is decided as it fills: het_third_form.)  `shapes` (dpm_launch_opts.fuse_shapes): n and batch may
// differ -- the mixed-shape kernels give every request its own tile count.
bool het_same_group(const dpm_stage& s0, const dpm_buffers& b0, const dpm_stage& s, const dpm_buffers& b, bool shapes) {
  return b.state_dtype == b0.state_dtype && b.eps_dtype == b0.eps_dtype && (shapes || (b.n == b0.n && b.batch == b0.batch)) &&
         s.model_type == s0.model_type && s.guidance == s0.guidance &&
         (s.flags & (DPM_F_TO_X0 | DPM_F_NOISE)) == (s0.flags & (DPM_F_TO_X0 | DPM_F_NOISE));  // SDE stages apart from ODE ones
}

// MS3 and UNIPC records never share a group -- stage_kernel_het dispatches {LIN1, TWO, MS3}, stage_kernel_het_unipc {LIN1, TWO,
// UNIPC}: the form of the two a record brings, 0 for the forms every group takes
int het_third_form(const dpm_stage& s) { return s.form == DPM_FORM_MS3 || s.form == DPM_FORM_UNIPC ? s.form : 0; }

// dpm_buffers.noise_sample0 of one request of a DPM_TABLE_NOISE call: honoured by a request that will own a noise row (`row`),
// an error on every other; non-negative, a whole number of Philox blocks
int check_noise_base(const dpm_stage& st, const dpm_buffers& b, bool row) {
  const int32_t k = b.noise_sample0;
  if (k == 0) return DPM_OK;
  if (k < 0) return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: noise_sample0=%d is negative", k);
  if (!(st.flags & DPM_F_NOISE))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: noise_sample0=%d on a stage without DPM_F_NOISE", k);
  if (!row)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: noise_sample0=%d on a request that fits no fused group (dense, "
                         "16-byte aligned buffers of whole 8-element groups)", k);
  const int64_t per = b.n / b.batch;
  if (per > 0 && (int64_t)k > INT64_MAX / per)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: noise_sample0=%d times %lld elements overflows", k, (long long)per);
  if (((int64_t)k * per) % 4 != 0)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: noise_sample0=%d times %lld elements is not a multiple of 4 (a "
                         "row starts at a Philox block)", k, (long long)per);
  return DPM_OK;
}

// The copies of one DPM_GUIDE_CFG2 request of a DPM_TABLE_PAIR or DPM_TABLE_PERP call: x_out2 and the third copy,
// dpm_buffers.thr_hint, come together, and only a request that will own a pair row or a Perp-Neg row (`row`) has a kernel that
// stores them -- the lone kernels' refusal otherwise, before anything is written or launched.  `flag_name`: the flag the text
// names (DPM_TABLE_PERP where the call carries that one alone).
int check_pair_copies(const dpm_stage& st, const dpm_buffers& b, bool row, const char* flag_name) {
  if (st.guidance != DPM_GUIDE_CFG2 || b.n == 0) return DPM_OK;
  if ((b.x_out2 != nullptr) != (b.thr_hint != nullptr))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: DPM_GUIDE_CFG2 in a %s call needs x_out2 and the third copy "
                         "(dpm_buffers.thr_hint) both set or both null", flag_name);
  if (b.x_out2 && !row)
    return dpm_set_error(DPM_ERR_UNSUPPORTED, "stage_launch: DPM_GUIDE_CFG2 with x_out2 (the kernel has no second store)");
  return DPM_OK;
}

// The table of a table-mode call (include/dpm_hip.h, "Table mode"): the header, n_req rows, then n_req noise records if and only
// if the call carries DPM_TABLE_NOISE, then n_req blend records (DPM_TABLE_BLEND), then n_req APG records (DPM_TABLE_APG), then
// n_req pair records (DPM_TABLE_PAIR or DPM_TABLE_PERP: one section, present under either) -- record i of every section beside
// row i.
struct TableSections {
  char *rows, *noise, *blend, *apg, *pair;
};
TableSections table_sections(void* table, int64_t n_req, int flags) {
  TableSections t;
  t.rows = static_cast<char*>(table) + DPM_TABLE_HEADER_BYTES;
  t.noise = t.rows + n_req * (int64_t)DPM_TABLE_ROW_BYTES;
  t.blend = t.noise + ((flags & DPM_TABLE_NOISE) ? n_req * (int64_t)DPM_TABLE_NOISE_BYTES : 0);
  t.apg = t.blend + ((flags & DPM_TABLE_BLEND) ? n_req * (int64_t)DPM_TABLE_BLEND_BYTES : 0);
  t.pair = t.apg + ((flags & DPM_TABLE_APG) ? n_req * (int64_t)DPM_TABLE_APG_BYTES : 0);  // (DPM_TABLE_PAIR / DPM_TABLE_PERP)
  return t;
}

// ---- The kinds of request that may own table rows, in the walk's order of precedence: a request is of the first kind whose
// flag the call carries and whose `row_ok` it passes (row_kind).  A group of one kind agrees on het_same_group's keys and on
// `same_group`; from `min_group` members on it owns a run of rows, and a record each in `section`, in a table-mode call.
bool sde_row_ok(const dpm_stage& st, const dpm_buffers& b) { return (st.flags & DPM_F_NOISE) && fusable_request(st, b); }
struct RowKind {
  int flag;                                                // the DPM_TABLE_* flag a call needs for it (0: none)
  bool (*row_ok)(const dpm_stage&, const dpm_buffers&);    // may the request own such a row?  (row_kind's guards come first)
  bool (*same_group)(const dpm_stage&, const dpm_stage&);  // what a group shares besides het_same_group's keys (null: nothing)
  bool third_form;  // ... and MS3 and UNIPC records never share a group (het_third_form)
  bool per_sample;  // one workgroup per SAMPLE, not per super-tile: members x batch stay below 2^31, too
  int min_group;    // the smallest group that takes the table
  char* TableSections::*section;  // its records' section (null: a row is all there is) ...
  size_t rec_bytes;
  void (*fill_recs)(const dpm_stage*, const dpm_buffers*, int, void*);  // ... and what DPM_TABLE_FILL writes there
  TableLaunchFn PairUnits::*launch;                                     // ONE launch over the group (DPM_TABLE_LAUNCH)
};
const RowKind kRowKinds[] = {
    // thresholded requests whose sample fits one workgroup (dpm_table_thresh.hpp), from ONE member on: a lone launch of a small
    // batch is a cluster with a workspace, a row is one workgroup per sample.  Any of LIN1 / TWO / MS3 / DENOISE in one group.
    {DPM_TABLE_THRESH, thresh_row_ok, thresh_same_group, false, true, 1, nullptr, 0, nullptr, &PairUnits::table_launch_thresh},
    // DPM_F_BLEND requests (dpm_table_blend.hpp), from ONE member on -- fusable_request refuses the blend, so the alternative is
    // a launch per request.  Any of LIN1 / TWO / MS3 in one group.
    {DPM_TABLE_BLEND, blend_row_ok, nullptr, false, false, 1, &TableSections::blend, DPM_TABLE_BLEND_BYTES, table_fill_blend,
     &PairUnits::table_launch_blend},
    // SDE requests, from ONE member on: a row's noise_sample0 has no other way to the kernel
    {DPM_TABLE_NOISE, sde_row_ok, nullptr, false, false, 1, &TableSections::noise, DPM_TABLE_NOISE_BYTES, table_fill_noise,
     &PairUnits::table_launch_noise},
    // guidance-rescale requests (DPM_F_CFG_RESCALE; dpm_table_rescale.hpp), from ONE member on: the alternative is a launch of
    // one workgroup per sample per request.  Any of LIN1 / TWO / MS3 / DENOISE, any phi and guidance scale in one group.
    {DPM_TABLE_RESCALE, rescale_row_ok, nullptr, false, true, 1, nullptr, 0, nullptr, &PairUnits::table_launch_rescale},
    // adaptive-projected-guidance requests (DPM_F_CFG_APG; dpm_table_apg.hpp), from ONE member on, for the same reason.  Any of
    // LIN1 / TWO / MS3 / DENOISE, any eta, r, beta -- rows with and without a momentum -- and guidance scale in one group; the
    // record carries the running average (the request's thr_hint in such a call) and the three scalars.
    {DPM_TABLE_APG, apg_row_ok, nullptr, false, true, 1, &TableSections::apg, DPM_TABLE_APG_BYTES, table_fill_apg,
     &PairUnits::table_launch_apg},
    // CFG-Zero* requests (DPM_F_CFG_ZSTAR; dpm_table_zstar.hpp), from ONE member on, for the same reason.  Any of LIN1 / TWO /
    // MS3 / DENOISE and any guidance scale in one group; the flag has no parameter and no state, so a row is all there is.
    {DPM_TABLE_ZSTAR, zstar_row_ok, nullptr, false, true, 1, nullptr, 0, nullptr, &PairUnits::table_launch_zstar},
    // Perp-Neg requests (DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record; dpm_table_perp.hpp), from ONE member on, for the same reason.
    // Before the two-condition kind, which refuses the flag (pair_row_ok): a flagged request is never blended linearly.  Any of
    // LIN1 / TWO / MS3 / DENOISE, any s and w, rows with and without the copies in one group; the record is a pair record, in the
    // pair records' section.
    {DPM_TABLE_PERP, perp_row_ok, nullptr, false, true, 1, &TableSections::pair, DPM_TABLE_PAIR_BYTES, table_fill_pair,
     &PairUnits::table_launch_perp},
    // requests under guidance over two conditions (DPM_GUIDE_CFG2; dpm_table_pair.hpp), from ONE member on: the alternative is a
    // launch per request.  A streaming kind, one workgroup per super-tile.  Any of LIN1 / TWO / MS3 / DENOISE, any two scales,
    // rows with and without the copies in one group; the record carries the third output (g) and the third copy of x_out (the
    // request's thr_hint in such a call).
    {DPM_TABLE_PAIR, pair_row_ok, nullptr, false, false, 1, &TableSections::pair, DPM_TABLE_PAIR_BYTES, table_fill_pair,
     &PairUnits::table_launch_pair},
    // every other fusable request, in every call: groups of 2..HET_MAX keep the kernarg records (stage_kernel_het needs no
    // dependent load in front of its tile's own), larger ones take the table.  An SDE group of a call without DPM_TABLE_NOISE
    // is gathered here too -- het_same_group keeps it apart from the ODE groups -- and owns no rows (stage_launch_multi_het).
    {0, fusable_request, nullptr, true, false, TABLE_MIN, nullptr, 0, nullptr, &PairUnits::table_launch},
};

// the kind of one request in a call that carries `flags`, or nullptr: it is launched on its own.  `fuse`: Tuning::multi_fuse.
// For a request that has passed check_stage_buffers: thresh_row_ok divides by b.batch.
const RowKind* row_kind(const dpm_stage& st, const dpm_buffers& b, int flags, bool fuse) {
  if (!fuse || b.n <= 0 || !pair_of(b.state_dtype, b.eps_dtype)) return nullptr;
  for (const RowKind& k : kRowKinds)
    if ((k.flag & ~flags) == 0 && k.row_ok(st, b)) return &k;
  return nullptr;
}
// does the request own a row of the kind that needs `flag`?
bool owns_row(int flag, const dpm_stage& st, const dpm_buffers& b, int flags, bool fuse) {
  const RowKind* const k = row_kind(st, b, flags, fuse);
  return k && k->flag == flag;
}

// one request on its own inside a per-request-stage call that carries `flags`.  In a DPM_TABLE_APG call the running average of
// a DPM_F_CFG_APG request is its thr_hint (bs[0].workspace is the table): it is launched with a copy of its buffers whose
// workspace is that.
int launch_alone(const dpm_stage* st, const dpm_buffers* b, int flags, void* stream) {
  if ((flags & DPM_TABLE_APG) && (st->flags & DPM_F_CFG_APG) && st->thr_max != 0.f) {
    dpm_buffers bb = *b;
    bb.workspace = bb.thr_hint;
    return dpm_stage_launch_ev(st, &bb, stream, nullptr, nullptr);
  }
  return dpm_stage_launch_ev(st, b, stream, nullptr, nullptr);
}

// dpm_stage_launch_multi with per_request_stages: check every request, fuse the compatible ones in groups of up to
// HET_MAX (first come, first grouped; the first MS3 or UNIPC record to join a group closes it to the other form, whose
// records wait for a later group), launch the rest one by one.  With fuse_shapes a group may hold several n: one whose members
// all share one n still takes the kernels it always took, one with at least two takes the mixed-shape family -- or, should
// its tile space not fit that family's 32-bit index, single launches.
// table_mode (DPM_TABLE_FILL / DPM_TABLE_LAUNCH; `table` = bs[0].workspace, checked by the caller): the same walk without
// the cap of HET_MAX -- a group is bounded by its launch's 2^31 super-tiles only.  A group of its kind's min_group members or
// more owns a run of consecutive table rows (table_sections), members in call order, the runs in the order the groups open,
// ONE row counter across the kinds: FILL writes the rows, the kind's records beside them (host memory, no HIP call, nothing
// launched; the record slots of other rows are not touched) and the header, LAUNCH launches one table kernel per run; every
// smaller group and every lone request goes as in mode 0 (LAUNCH) or nowhere (FILL).  Both modes walk the requests in this
// one function, so their row order is the same.
int stage_launch_multi_het(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, int table_mode, void* table) {
  const int flags = table_mode & (DPM_TABLE_NOISE | DPM_TABLE_THRESH | DPM_TABLE_BLEND | DPM_TABLE_RESCALE | DPM_TABLE_APG |
                                  DPM_TABLE_ZSTAR | DPM_TABLE_PAIR | DPM_TABLE_PERP);
  const bool noise_rows = (flags & DPM_TABLE_NOISE) != 0, perp_rows = (flags & DPM_TABLE_PERP) != 0;
  const bool pair_rows = (flags & DPM_TABLE_PAIR) != 0 || perp_rows;  // (the calls whose DPM_GUIDE_CFG2 requests may carry copies)
  table_mode &= ~flags;
  for (int r = 0; r < n_req; ++r)  // (in a call with DPM_TABLE_PERP alone only a flagged request may carry copies)
    if (const int rc = check_stage_buffers(&st[r], &bs[r], noise_rows, (flags & DPM_TABLE_APG) != 0,
                                           (flags & DPM_TABLE_PAIR) || (perp_rows && (st[r].flags & DPM_F_CFG2_PERP)),
                                           table_mode != 0 && !perp_rows))
      return rc;
  const bool fuse = tuning_for(bs[0].opts).multi_fuse != 0;
  const bool shapes = bs[0].opts->fuse_shapes == 1;
  const bool fill = table_mode == DPM_TABLE_FILL;
  for (int r = 0; noise_rows && r < n_req; ++r)
    if (const int rc = check_noise_base(st[r], bs[r], owns_row(DPM_TABLE_NOISE, st[r], bs[r], flags, fuse))) return rc;
  for (int r = 0; pair_rows && r < n_req; ++r) {
    const RowKind* const k = row_kind(st[r], bs[r], flags, fuse);
    const bool row = k && (k->flag == DPM_TABLE_PAIR || k->flag == DPM_TABLE_PERP);
    if (const int rc = check_pair_copies(st[r], bs[r], row, (flags & DPM_TABLE_PAIR) ? "DPM_TABLE_PAIR" : "DPM_TABLE_PERP")) return rc;
  }
  const TableSections sec = table_mode ? table_sections(table, n_req, flags) : TableSections{};
  int64_t n_rows = 0;
  uint32_t n_runs = 0;
  std::vector<char> done((size_t)n_req, 0);
  std::vector<dpm_stage> gs((size_t)HET_MAX);
  std::vector<dpm_buffers> gb((size_t)HET_MAX);
  std::vector<int> gi((size_t)HET_MAX);
  for (int r0 = 0; r0 < n_req; ++r0) {
    if (done[r0]) continue;
    int cnt = 0, third = 0;
    auto join = [&](int r) {
      if ((size_t)cnt == gs.size()) {
        gs.resize(2 * gs.size());
        gb.resize(gs.size());
        gi.resize(gs.size());
      }
      gs[cnt] = st[r];
      gb[cnt] = bs[r];
      gi[cnt++] = r;
    };
    // the group r0 opens: every later request of its kind that agrees with it, in call order
    const RowKind* const kind = row_kind(st[r0], bs[r0], flags, fuse);
    if (kind) {
      int64_t cap = table_mode ? table_group_cap(bs[r0].n) : HET_MAX;
      if (kind->per_sample) cap = std::min<int64_t>(cap, 0x7fffffff / bs[r0].batch);
      for (int r = r0; r < n_req && cnt < cap; ++r) {
        if (done[r] || !kind->row_ok(st[r], bs[r]) || !het_same_group(st[r0], bs[r0], st[r], bs[r], shapes) ||
            (kind->same_group && !kind->same_group(st[r0], st[r])))
          continue;
        if (const int f = kind->third_form ? het_third_form(st[r]) : 0) {
          if (third && f != third) continue;
          third = f;
        }
        join(r);
      }
    }
    // (an SDE group of a call without DPM_TABLE_NOISE owns no rows: it goes as in mode 0, beyond HET_MAX members in launches
    // of HET_MAX)
    const bool sde = (st[r0].flags & DPM_F_NOISE) != 0;
    if (kind && table_mode && cnt >= kind->min_group && (!sde || noise_rows)) {
      const PairUnits& p = *pair_of(bs[r0].state_dtype, bs[r0].eps_dtype);
      void* const run = sec.rows + n_rows * (int64_t)DPM_TABLE_ROW_BYTES;
      void* const recs = kind->section ? sec.*(kind->section) + n_rows * (int64_t)kind->rec_bytes : nullptr;
      if (fill) {
        table_fill_rows(gs.data(), gb.data(), cnt, run);
        if (kind->fill_recs) kind->fill_recs(gs.data(), gb.data(), cnt, recs);
      } else if (const int rc = (p.*(kind->launch))(gs.data(), gb.data(), cnt, run, recs, stream)) {
        return rc;
      }
      n_rows += cnt;
      n_runs += 1;
      for (int k = 0; k < cnt; ++k) done[gi[k]] = 1;
    } else if (cnt > 1) {
      const PairUnits& p = *pair_of(bs[r0].state_dtype, bs[r0].eps_dtype);
      for (int k0 = 0; k0 < cnt && !fill; k0 += HET_MAX) {  // (mode 0: one round, cnt <= HET_MAX)
        const int m = std::min(HET_MAX, cnt - k0);
        const dpm_stage* ms = gs.data() + k0;
        const dpm_buffers* mb = gb.data() + k0;
        bool mixed = false;
        for (int k = 1; k < m; ++k) mixed = mixed || mb[k].n != mb[0].n;
        int rc = m < 2 ? MULTI_NOT_BUILT : mixed ? p.het_shapes(ms, mb, m, stream) : p.het(ms, mb, m, stream);
        if (rc == MULTI_NOT_BUILT) {
          rc = DPM_OK;
          for (int k = 0; k < m && !rc; ++k) rc = launch_alone(&ms[k], &mb[k], flags, stream);
        }
        if (rc) return rc;
      }
      for (int k = 0; k < cnt; ++k) done[gi[k]] = 1;
    } else {
      if (!fill)
        if (const int rc = launch_alone(&st[r0], &bs[r0], flags, stream)) return rc;
      done[r0] = 1;
    }
  }
  if (fill) {
    const uint32_t header[4] = {DPM_TABLE_MAGIC, (uint32_t)DPM_HIP_VERSION, (uint32_t)n_req, n_runs};
    static_assert(sizeof header == DPM_TABLE_HEADER_BYTES, "the table header is four words");
    std::memcpy(table, header, sizeof header);
  }
  return DPM_OK;
}

// the argument rules of dpm_launch_opts.table_mode (include/dpm_hip.h, "Table mode"); o = bs[0].opts
int check_table_mode(const dpm_launch_opts* o, const dpm_stage* st, const dpm_buffers* bs) {
  const int mode = o->table_mode & ~(DPM_TABLE_NOISE | DPM_TABLE_THRESH | DPM_TABLE_BLEND | DPM_TABLE_RESCALE | DPM_TABLE_APG |
                                     DPM_TABLE_ZSTAR | DPM_TABLE_PAIR | DPM_TABLE_PERP);
  if (o->table_mode < 0 || (mode != DPM_TABLE_FILL && mode != DPM_TABLE_LAUNCH))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode=%d (0, DPM_TABLE_FILL or DPM_TABLE_LAUNCH, with or "
                         "without DPM_TABLE_NOISE / DPM_TABLE_THRESH / DPM_TABLE_BLEND / DPM_TABLE_RESCALE / DPM_TABLE_APG / "
                         "DPM_TABLE_ZSTAR / DPM_TABLE_PAIR / DPM_TABLE_PERP)",
                         o->table_mode);
  if (o->per_request_stages != 1)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode needs per_request_stages == 1");
  if (o->fuse_shapes == 1)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode with fuse_shapes (the table kernels take one n per launch)");
  if (!bs[0].workspace || reinterpret_cast<uintptr_t>(bs[0].workspace) % 16 != 0)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode needs the table in bs[0].workspace, 16-byte aligned");
  // (a thresholded request 0 that owns a row of a DPM_TABLE_THRESH call needs no workspace of its own)
  // (st[0] has not passed check_stage_buffers yet: its batch is checked here)
  const bool row0 = bs[0].batch >= 1 && bs[0].n % bs[0].batch == 0 &&
                    owns_row(DPM_TABLE_THRESH, st[0], bs[0], o->table_mode, tuning_for(o).multi_fuse != 0);
  if ((st[0].flags & DPM_F_THRESH) && !row0)
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode with DPM_F_THRESH in st[0] (bs[0].workspace is the table)");
  // (its running average would be that workspace; in a DPM_TABLE_APG call it is thr_hint)
  if ((st[0].flags & DPM_F_CFG_APG) && st[0].thr_max != 0.f && !(o->table_mode & DPM_TABLE_APG))
    return dpm_set_error(DPM_ERR_ARG, "stage_launch_multi: table_mode with a DPM_F_CFG_APG momentum in st[0] (bs[0].workspace is the table)");
  return DPM_OK;
}
}  // namespace

extern "C" int dpm_stage_launch_multi(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream) {
  const dpm_launch_opts* o = st && bs && n_req >= 1 ? bs[0].opts : nullptr;
  if (o && o->table_mode != 0) {
    if (const int rc = check_table_mode(o, st, bs)) return rc;
    return stage_launch_multi_het(st, bs, n_req, stream, o->table_mode, bs[0].workspace);
  }
  if (o && o->per_request_stages == 1) return stage_launch_multi_het(st, bs, n_req, stream, 0, nullptr);
  return dpm_stage_launch_multi_ev(st, bs, n_req, stream, nullptr, nullptr, nullptr);
}

int dpm_timing_begin(int n, void*** starts, void*** stops) {
  void** a = new (std::nothrow) void*[2 * (size_t)n]();
  if (!a) return dpm_set_error(DPM_ERR_NOMEM, "out of memory");
  for (int i = 0; i < 2 * n; ++i) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(static_cast<hipEvent_t>(a[j]));
      delete[] a;
      return dpm_set_error((int)rc, "hipEventCreate: %s", hipGetErrorString(rc));
    }
    a[i] = e;
  }
  *starts = a;
  *stops = a + n;
  return DPM_OK;
}

// `recorded` (optional, n flags): event pairs that were never handed to a launch (members of a fused group other than its
// first) are skipped, their ms stays untouched
int dpm_timing_end(int n, void** starts, void** stops, void* stream, float* ms, const unsigned char* recorded) {
  int ret = DPM_OK;
  hipError_t rc = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (rc != hipSuccess) ret = dpm_set_error((int)rc, "hipStreamSynchronize: %s", hipGetErrorString(rc));
  for (int i = 0; i < n; ++i) {
    if (ms && ret == DPM_OK && (!recorded || recorded[i])) {
      rc = hipEventElapsedTime(&ms[i], static_cast<hipEvent_t>(starts[i]), static_cast<hipEvent_t>(stops[i]));
      if (rc != hipSuccess) ret = dpm_set_error((int)rc, "hipEventElapsedTime(stage %d): %s", i, hipGetErrorString(rc));
    }
  }
  for (int i = 0; i < 2 * n; ++i) (void)hipEventDestroy(static_cast<hipEvent_t>(starts[i]));
  delete[] starts;
  return ret;
}

extern "C" size_t dpm_threshold_workspace_bytes(int64_t batch, int64_t per_sample) {
  if (batch < 1 || per_sample < 1) return 0;
  const DeviceInfo& di = device_info();
  // 0 when one workgroup per sample is the plan (the sample lives in that workgroup's LDS); else the zeroed
  // per-sample histograms and barrier counters the clusters merge through
  return (size_t)thr_ws_bytes(batch, per_sample, di.n_cu > 0 ? di.n_cu : 256);
}

extern "C" int dpm_add_noise_launch_f64(const dpm_schedule* s, const double* t_host, int nt, const void* x, const void* noise,
                                        void* out, int64_t n, void* stream) {
  if (!s || !t_host || !x || !noise || !out || nt < 1 || n < 0) return dpm_set_error(DPM_ERR_ARG, "add_noise: bad arguments");
  if (n == 0) return DPM_OK;
  for (int j = 0; j < nt; ++j) {  // the schedule in double at the double time (fp32 tables are promoted exactly, ref :127-134)
    double a64 = 0., s64 = 0.;
    dpm_schedule_eval_f64(s, DPM_EVAL_ALPHA, &t_host[j], 1, &a64);
    dpm_schedule_eval_f64(s, DPM_EVAL_STD, &t_host[j], 1, &s64);
    const int rc = dpm_add_noise_f64(a64, s64, x, static_cast<const double*>(noise) + (int64_t)j * n,
                                     static_cast<double*>(out) + (int64_t)j * n, n, stream);
    if (rc) return rc;
  }
  return DPM_OK;
}

extern "C" int dpm_add_noise_launch(const dpm_schedule* s, const float* t_host, int nt, const void* x, const void* noise,
                                    void* out, int64_t n, int dtype, void* stream) {
  if (!s || !t_host || !x || !noise || !out || nt < 1 || n < 0) return dpm_set_error(DPM_ERR_ARG, "add_noise: bad arguments");
  if (n == 0) return DPM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == DPM_DTYPE_F64) {  // double state: alpha / sigma in double on a dtype=float64 schedule, else fp32 values promoted
    for (int j = 0; j < nt; ++j) {
      double a64 = 0., s64 = 0.;
      if (dpm_schedule_table_is_f64(s)) {
        const double tj = (double)t_host[j];
        dpm_schedule_eval_f64(s, DPM_EVAL_ALPHA, &tj, 1, &a64);
        dpm_schedule_eval_f64(s, DPM_EVAL_STD, &tj, 1, &s64);
      } else {
        float a = 0.f, sg = 0.f;
        dpm_schedule_eval(s, DPM_EVAL_ALPHA, &t_host[j], 1, &a);
        dpm_schedule_eval(s, DPM_EVAL_STD, &t_host[j], 1, &sg);
        a64 = a;
        s64 = sg;
      }
      const int rc = dpm_add_noise_f64(a64, s64, x, static_cast<const double*>(noise) + (int64_t)j * n,
                                       static_cast<double*>(out) + (int64_t)j * n, n, stream);
      if (rc) return rc;
    }
    return DPM_OK;
  }
  const DeviceInfo& di = device_info();
  const int n_cu = di.n_cu > 0 ? di.n_cu : 256;
  const int64_t blocks = aux_grid_blocks(n, n_cu, false);
  const bool v2 = n % EPT == 0;
  const int rc = with_elem_type(dtype, "add_noise", [&](auto t) {
    using T = decltype(t);
    for (int j = 0; j < nt; ++j) {
      float a = 0.f, sg = 0.f;
      dpm_schedule_eval(s, DPM_EVAL_ALPHA, &t_host[j], 1, &a);
      dpm_schedule_eval(s, DPM_EVAL_STD, &t_host[j], 1, &sg);
      const int64_t off = (int64_t)j * n;
      const T* xp = (const T*)x;
      const T* np_ = (const T*)noise + off;
      T* op = (T*)out + off;
      const size_t al = sizeof(T) * EPT;
      if (v2 && aligned(xp, al) && aligned(np_, al) && aligned(op, al)) {
        const int64_t bl = aux_grid_blocks(n, n_cu, true);
        hipLaunchKernelGGL((add_noise_kernel<T, true>), dim3((unsigned)bl), dim3(256), 0, st, xp, np_, op, n, a, sg);
      } else {
        hipLaunchKernelGGL((add_noise_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, xp, np_, op, n, a, sg);
      }
    }
  });
  return rc ? rc : launch_status("add_noise launch failed");
}

extern "C" int dpm_blend_launch(const void* x, const void* mask, const void* a, const void* b, float alpha, float sigma,
                                void* out, int64_t n, int64_t mask_period, int dtype, void* stream) {
  if (!x || !mask || !a || !out || n < 0 || mask_period < 1) return dpm_set_error(DPM_ERR_ARG, "blend: bad arguments");
  if (n == 0) return DPM_OK;
  if (dtype == DPM_DTYPE_F64) return dpm_blend_f64(x, mask, a, b, (double)alpha, (double)sigma, out, n, mask_period, stream);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DeviceInfo& di = device_info();
  const int64_t blocks = aux_grid_blocks(n, di.n_cu > 0 ? di.n_cu : 256, false);
  KExt ext;
  std::memset(&ext, 0, sizeof ext);
  ext.mask_period = mask_period;
  ext.blend_alpha = alpha;
  ext.blend_sigma = sigma;
  const int rc = with_elem_type(dtype, "blend", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(blend_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, (const T*)mask, (const T*)a,
                       (const T*)b, (T*)out, n, ext);
  });
  return rc ? rc : launch_status("blend launch failed");
}

extern "C" int dpm_adaptive_error_launch(const void* x_lower, const void* x_higher, const void* x_prev, float atol,
                                         float rtol, float* e_out, int64_t batch, int64_t per_sample, int dtype,
                                         void* stream) {
  if (!x_lower || !x_higher || !x_prev || !e_out || batch < 1 || per_sample < 1)
    return dpm_set_error(DPM_ERR_ARG, "adaptive_error: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t me = hipMemsetAsync(e_out + batch, 0, sizeof(float), st);  // the batch-maximum slot
  if (me != hipSuccess) return dpm_set_error((int)me, "hipMemsetAsync: %s", hipGetErrorString(me));
  const int rc = with_elem_type(dtype, "adaptive_error", [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(adaptive_error_kernel<T>, dim3((unsigned)batch), dim3(1024), 0, st, (const T*)x_lower,
                       (const T*)x_higher, (const T*)x_prev, atol, rtol, e_out, per_sample);
  });
  return rc ? rc : launch_status("adaptive_error launch failed");
}

// ------------------------------------------------------------------------------------------------
// adaptive solver, controller on the device (include/dpm_hip.h: dpm_adaptive_*; ref :956-1010)
// ------------------------------------------------------------------------------------------------
namespace {
struct AdaptiveDev {  // device-resident controller state
  float s, lambda_s, lambda_0, h, t_0, t_err, theta, t;
  int32_t order, nfe, done, iters, accept, accepted, pad0, pad1;
  dpm_stage st[5];  // 0, 1: the lower-order update's stages; 2, 3, 4: the higher-order update's
};
struct AdaptiveStatic {
  int32_t algo, solver, model_type, guidance;
  double scale;
};

// the stage records of one iteration s -> t (order 2: DPM-Solver-12, order 3: DPM-Solver-23, ref :976-993), in three
// independent pieces so that the device can run them on different wavefronts: the lower-order update's stages, the
// higher-order update's, and the prologue scalars (alpha, sigma, model time, guidance) of one stage
template <class S>
DPM_HD void adaptive_plan_lower(const S* sv, const AdaptiveStatic& c, int order, float s, float t, dpm_stage* st) {
  if (order == 2) {
    dpmc::singlestep_fill(sv, c.algo, c.solver, 1, s, t, 0., 0., 0, &st[0]);
    st[1] = st[0];
  } else {
    dpmc::singlestep_fill(sv, c.algo, c.solver, 2, s, t, 1. / 3., 0., 0, &st[0]);
  }
}
template <class S>
DPM_HD void adaptive_plan_higher(const S* sv, const AdaptiveStatic& c, int order, float s, float t, dpm_stage* st) {
  if (order == 2) {
    dpmc::singlestep_fill(sv, c.algo, c.solver, 2, s, t, 0.5, 0., 0, &st[2]);
    st[4] = st[3];
  } else {
    dpmc::singlestep_fill(sv, c.algo, c.solver, 3, s, t, 1. / 3., 2. / 3., 0, &st[2]);
  }
}
template <class S>
DPM_HD void adaptive_plan_prologue(const S* sv, const AdaptiveStatic& c, dpm_stage* st) {
  dpmc::set_prologue(sv, st->t_eval, c.model_type, c.guidance, c.scale, st);
}
template <class S>
DPM_HD void adaptive_plan(const S* sv, const AdaptiveStatic& c, int order, float s, float t, dpm_stage* st) {
  adaptive_plan_lower(sv, c, order, s, t, st);
  adaptive_plan_higher(sv, c, order, s, t, st);
  for (int i = 0; i < 5; ++i) adaptive_plan_prologue(sv, c, &st[i]);
}

__global__ void adaptive_reset_kernel(AdaptiveDev* S, float s, float lambda_s, float lambda_0, float h, float t_0,
                                      float t_err, float theta, int order, int32_t* status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  S->s = s;
  S->lambda_s = lambda_s;
  S->lambda_0 = lambda_0;
  S->h = h;
  S->t_0 = t_0;
  S->t_err = t_err;
  S->theta = theta;
  S->t = s;
  S->order = order;
  S->nfe = 0;
  S->iters = 0;
  S->accept = 0;
  S->accepted = 0;
  S->done = !(fabsf(s - t_0) > t_err);  // the loop condition of ref :995 before the first iteration
  for (int i = 0; i < 4; ++i) __hip_atomic_store(&status[i], i == 0 ? S->done : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// decision on the previous iteration (one thread), plan of the next one -- double-precision exp / log / expm1 chains,
// spread over the block's four wavefronts: lower-order stages on one, higher-order stages on another, then the five
// prologues round-robin --, then the time vectors of the network calls (all threads)
__global__ __launch_bounds__(256) void adaptive_begin_kernel(AdaptiveDev* S, dpmc::SchedView sv, AdaptiveStatic c,
                                                             float* e_dev, float* tvec, int64_t tv_len, int32_t* status) {
  __shared__ float te[3], ti[3];
  __shared__ int live;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) {
    const float E = *e_dev;
    if (S->iters > 0 && !S->done && E != E) {
      // a NaN estimate is never accepted and would turn h, t and the time vectors into NaN without ever ending the run
      // (ref :1002-1008 spins): reject and end the run with the verdict 2; s, h, nfe and the time vectors keep their values
      S->accept = 0;
      S->done = 2;
    } else if (S->iters > 0 && !S->done) {
      const int acc = E <= 1.f;  // ref :1002
      if (acc) {
        S->s = S->t;
        S->lambda_s = sv.lambda(S->s);
      }
      // ref :1007: h = min(theta * h * E^(-1/order), lambda_0 - lambda_s); the power in double like the reference's float()
      const float pw = (float)pow((double)E, -1.0 / (double)S->order);
      const float hn = (S->theta * S->h) * pw;
      const float room = S->lambda_0 - S->lambda_s;
      S->h = room < hn ? room : hn;
      S->nfe += S->order;
      S->accept = acc;
      S->accepted += acc;
      if (!(fabsf(S->s - S->t_0) > S->t_err)) S->done = 1;  // ref :995
    } else {
      S->accept = 0;
    }
    *e_dev = 0.f;
    live = !S->done;
    if (live) S->t = sv.inv_lambda(S->lambda_s + S->h);  // ref :996
  }
  __syncthreads();
  if (live && lane == 0) {
    if (wave == 0) adaptive_plan_lower(&sv, c, S->order, S->s, S->t, S->st);
    if (wave == 1) adaptive_plan_higher(&sv, c, S->order, S->s, S->t, S->st);
  }
  __syncthreads();
  if (live && lane == 0) {
    adaptive_plan_prologue(&sv, c, &S->st[wave]);
    if (wave == 0) adaptive_plan_prologue(&sv, c, &S->st[4]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (live)
      for (int j = 0; j < 3; ++j) {
        te[j] = S->st[2 + j].t_eval;
        ti[j] = S->st[2 + j].t_input;
      }
    // the verdict as of THIS begin, by its index: a host that looks at begin #j (after waiting for it) reads the same
    // value on every rank of a sharded run, however far its device has run ahead
    __hip_atomic_store(&status[8 + (S->iters & 31)], S->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    S->iters += 1;
    __hip_atomic_store(&status[1], S->nfe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&status[2], S->iters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&status[3], S->accepted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&status[0], S->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  if (!live) return;
  for (int j = 0; j < 3; ++j)
    for (int64_t i = threadIdx.x; i < tv_len; i += blockDim.x) {
      tvec[(int64_t)(2 * j) * tv_len + i] = te[j];
      tvec[(int64_t)(2 * j + 1) * tv_len + i] = ti[j];
    }
}

// an accepted step becomes the state: x <- x_higher, x_prev <- x_lower (ref :1003-1005)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void adaptive_commit_kernel(const AdaptiveDev* S, T* __restrict__ x, T* __restrict__ xp,
                                                              const T* __restrict__ xl, const T* __restrict__ xh, int64_t n) {
  if (!S->accept) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = n * (int64_t)sizeof(T) / 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
      reinterpret_cast<u32x4*>(x)[i] = ld16<true>(reinterpret_cast<const u32x4*>(xh) + i);
      reinterpret_cast<u32x4*>(xp)[i] = ld16<true>(reinterpret_cast<const u32x4*>(xl) + i);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      x[i] = xh[i];
      xp[i] = xl[i];
    }
  }
}

// error norm with G workgroups per sample: partial sums of squares in double, the last workgroup of a sample adds
// them in a fixed order (deterministic), E_b = sqrt(mean) and the batch maximum by atomicMax on the bit pattern
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void adaptive_error_kernel2(const T* __restrict__ xl, const T* __restrict__ xh,
                                                              const T* __restrict__ xp, float atol, float rtol,
                                                              int64_t per_sample, int G, double* __restrict__ partial,
                                                              uint32_t* __restrict__ counters, float* __restrict__ e_max,
                                                              const int32_t* skip) {
  if (skip && *skip) return;
  __shared__ double part[4];
  __shared__ int last;
  const int b = blockIdx.x / G, g = blockIdx.x % G;
  const int64_t chunk = ((per_sample + G - 1) / G + 7) / 8 * 8;
  const int64_t lo = (int64_t)g * chunk, hi = lo + chunk < per_sample ? lo + chunk : per_sample;
  const int64_t base = (int64_t)b * per_sample;
  double acc = 0.;
  auto term = [&](float l, float h, float pv) {
    const float delta = fmaxf(atol, rtol * fmaxf(fabsf(l), fabsf(pv)));
    const float v = (h - l) / delta;
    acc += (double)(v * v);
  };
  if (VEC) {
    for (int64_t i = lo + (int64_t)threadIdx.x * EPT; i < hi; i += (int64_t)blockDim.x * EPT) {
      float l[EPT], h[EPT], pv[EPT];
      load_pack<true>(xl, (base + i) / EPT, l);
      load_pack<true>(xh, (base + i) / EPT, h);
      load_pack<true>(xp, (base + i) / EPT, pv);
#pragma unroll
      for (int j = 0; j < EPT; ++j) term(l[j], h[j], pv[j]);
    }
  } else {
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
      term(to_f32(xl[base + i]), to_f32(xh[base + i]), to_f32(xp[base + i]));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
    __threadfence();
    last = atomicAdd(&counters[b], 1u) == (uint32_t)(G - 1);
    if (last) {
      __threadfence();
      double t = 0.;
      for (int q = 0; q < G; ++q) t += __hip_atomic_load(&partial[(int64_t)b * G + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float e = sqrtf((float)(t / (double)per_sample));
      atomicMax(reinterpret_cast<unsigned int*>(e_max), __float_as_uint(e));  // E >= 0: bit patterns order like values
      counters[b] = 0u;  // ready for the next launch
    }
  }
}
}  // namespace

struct dpm_adaptive {
  dpm_adaptive_desc d;
  AdaptiveStatic c;
  dpmc::SchedView sv;        // table pointers into `tables` (device)
  float* tables = nullptr;   // 4 x K floats
  AdaptiveDev* dev = nullptr;
  int32_t* status = nullptr; // host-mapped: done, nfe, iterations, accepted
  double* partial = nullptr; // error norm scratch, grown on demand
  uint32_t* counters = nullptr;
  int64_t scratch_blocks = 0, scratch_batch = 0;
  dpm_stage tmpl[5];
  float s0, lambda_s0, lambda_0;
};

extern "C" void dpm_adaptive_destroy(dpm_adaptive* a) {
  if (!a) return;
  if (a->tables) (void)hipFree(a->tables);
  if (a->dev) (void)hipFree(a->dev);
  if (a->status) (void)hipHostFree(a->status);
  if (a->partial) (void)hipFree(a->partial);
  if (a->counters) (void)hipFree(a->counters);
  delete a;
}

extern "C" int dpm_adaptive_create(const dpm_schedule* s, const dpm_adaptive_desc* d, dpm_adaptive** out) {
  if (!s || !d || !out) return dpm_set_error(DPM_ERR_ARG, "adaptive_create: null pointer");
  if (d->order != 2 && d->order != 3)
    return dpm_set_error(DPM_ERR_ARG, "For adaptive step size solver, order must be 2 or 3, got %d", d->order);
  if (d->algorithm_type < 0 || d->algorithm_type > 1 || d->solver_type < 0 || d->solver_type > 1 || d->model_type < 0 ||
      d->model_type > 3 || d->guidance < 0 || d->guidance > 2)
    return dpm_set_error(DPM_ERR_ARG, "adaptive_create: enumeration out of range");
  dpm_adaptive* a = new (std::nothrow) dpm_adaptive;
  if (!a) return dpm_set_error(DPM_ERR_NOMEM, "out of memory");
  a->d = *d;
  a->c = AdaptiveStatic{d->algorithm_type, d->solver_type, d->model_type, d->guidance, d->guidance_scale};
  const dpmc::SchedView hv = dpm_schedule_view(s);
  a->sv = hv;
  hipError_t e = hipSuccess;
  if (hv.discrete) {
    const size_t K = (size_t)hv.total_N;
    e = hipMalloc(&a->tables, 4 * K * sizeof(float));
    const float* src[4] = {hv.la, hv.t, hv.la_rev, hv.t_rev};
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
      e = hipMemcpy(a->tables + i * K, src[i], K * sizeof(float), hipMemcpyHostToDevice);
    a->sv.la = a->tables;
    a->sv.t = a->tables + K;
    a->sv.la_rev = a->tables + 2 * K;
    a->sv.t_rev = a->tables + 3 * K;
  } else {
    a->sv.la = a->sv.t = a->sv.la_rev = a->sv.t_rev = nullptr;
  }
  if (e == hipSuccess) e = hipMalloc(&a->dev, sizeof(AdaptiveDev));
  if (e == hipSuccess) e = hipMemset(a->dev, 0, sizeof(AdaptiveDev));
  void* st = nullptr;
  if (e == hipSuccess) e = hipHostMalloc(&st, 256, hipHostMallocMapped);
  if (e != hipSuccess) {
    dpm_adaptive_destroy(a);
    return dpm_set_error((int)e, "adaptive_create: %s", hipGetErrorString(e));
  }
  a->status = static_cast<int32_t*>(st);
  std::memset(a->status, 0, 256);
  // host copy of the plan for the static fields (form, flags, slots) and the initial scalars
  a->s0 = (float)d->t_start;
  a->lambda_s0 = hv.lambda(a->s0);
  a->lambda_0 = hv.lambda((float)d->t_end);
  const float t1 = hv.inv_lambda(a->lambda_s0 + (float)d->h_init);
  adaptive_plan(&hv, a->c, d->order, a->s0, t1, a->tmpl);
  *out = a;
  return DPM_OK;
}

extern "C" int dpm_adaptive_stage_template(const dpm_adaptive* a, int which, dpm_stage* out) {
  if (!a || !out || which < 0 || which > 4) return dpm_set_error(DPM_ERR_ARG, "adaptive_stage_template: bad arguments");
  *out = a->tmpl[which];
  return DPM_OK;
}

extern "C" int dpm_adaptive_reset(dpm_adaptive* a, void* stream) {
  if (!a) return dpm_set_error(DPM_ERR_ARG, "adaptive_reset: null handle");
  hipLaunchKernelGGL(adaptive_reset_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a->dev, a->s0,
                     a->lambda_s0, a->lambda_0, (float)a->d.h_init, (float)a->d.t_end, (float)a->d.t_err, (float)a->d.theta,
                     a->d.order, a->status);
  return launch_status("adaptive_reset");
}

extern "C" int dpm_adaptive_begin(dpm_adaptive* a, void* x, void* x_prev, const void* x_lower, const void* x_higher, int64_t n,
                                  int dtype, float* e_dev, float* t_vectors, int64_t tv_len, void* stream) {
  // n == 0: an empty shard of a batch-sharded run -- it still runs the controller (every rank must take the same
  // decisions and issue the same collectives) but has no state to commit, and its tensors have no storage
  if (!a || !e_dev || !t_vectors || n < 0 || tv_len < 1 || (n > 0 && (!x || !x_prev || !x_lower || !x_higher)))
    return dpm_set_error(DPM_ERR_ARG, "adaptive_begin: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adaptive_begin_kernel, dim3(1), dim3(256), 0, st, a->dev, a->sv, a->c, e_dev, t_vectors, tv_len, a->status);
  if (n > 0) {
    const DeviceInfo& di = device_info();
    const int64_t cap = (int64_t)(di.n_cu > 0 ? di.n_cu : 256) * 8;
    const int rc = with_elem_type(dtype, "adaptive_begin", [&](auto t) {
      using T = decltype(t);
      const bool v = (n * (int64_t)sizeof(T)) % 16 == 0 && aligned(x, 16) && aligned(x_prev, 16) && aligned(x_lower, 16) &&
                     aligned(x_higher, 16);
      int64_t bl = ((v ? n * (int64_t)sizeof(T) / 16 : n) + 255) / 256;
      if (bl > cap) bl = cap;
      if (v)
        hipLaunchKernelGGL((adaptive_commit_kernel<T, true>), dim3((unsigned)bl), dim3(256), 0, st, a->dev, (T*)x,
                           (T*)x_prev, (const T*)x_lower, (const T*)x_higher, n);
      else
        hipLaunchKernelGGL((adaptive_commit_kernel<T, false>), dim3((unsigned)bl), dim3(256), 0, st, a->dev, (T*)x,
                           (T*)x_prev, (const T*)x_lower, (const T*)x_higher, n);
    });
    if (rc) return rc;
  }
  return launch_status("adaptive_begin");
}

extern "C" int dpm_adaptive_stage_launch(dpm_adaptive* a, int which, const dpm_stage* st, const dpm_buffers* b, void* stream) {
  if (!a || !st || !b || which < 0 || which > 4) return dpm_set_error(DPM_ERR_ARG, "adaptive_stage_launch: bad arguments");
  return dpm_stage_launch_dyn(st, b, stream, nullptr, nullptr, &a->dev->st[which], &a->dev->done);
}

extern "C" int dpm_adaptive_error(dpm_adaptive* a, const void* x_lower, const void* x_higher, const void* x_prev,
                                  int64_t batch, int64_t per_sample, int dtype, float* e_dev, void* stream) {
  if (!a || !e_dev || batch < 0) return dpm_set_error(DPM_ERR_ARG, "adaptive_error: bad arguments");
  if (batch == 0) return DPM_OK;  // an empty shard contributes nothing to the maximum (begin left *e_dev = 0)
  if (!x_lower || !x_higher || !x_prev || per_sample < 1) return dpm_set_error(DPM_ERR_ARG, "adaptive_error: bad arguments");
  const DeviceInfo& di = device_info();
  const int n_cu = di.n_cu > 0 ? di.n_cu : 256;
  // enough workgroups to fill the chip twice, at least 8192 elements each
  int64_t G = std::max<int64_t>(1, std::min<int64_t>((2 * (int64_t)n_cu + batch - 1) / batch, per_sample / 8192));
  if (G > 64) G = 64;
  const int64_t blocks = batch * G;
  if (blocks > a->scratch_blocks || batch > a->scratch_batch) {  // grow the scratch (outside any capture: create-time sizes)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs);
    if (cs != hipStreamCaptureStatusNone)
      return dpm_set_error(DPM_ERR_UNSUPPORTED, "adaptive_error: run one iteration outside the capture first (scratch allocation)");
    (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (a->partial) (void)hipFree(a->partial);
    if (a->counters) (void)hipFree(a->counters);
    a->partial = nullptr;
    a->counters = nullptr;
    hipError_t e = hipMalloc(&a->partial, (size_t)blocks * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&a->counters, (size_t)batch * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(a->counters, 0, (size_t)batch * sizeof(uint32_t));
    if (e != hipSuccess) return dpm_set_error((int)e, "adaptive_error: %s", hipGetErrorString(e));
    a->scratch_blocks = blocks;
    a->scratch_batch = batch;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = with_elem_type(dtype, "adaptive_error", [&](auto t) {
    using T = decltype(t);
    const size_t al = sizeof(T) * EPT;
    const bool v = per_sample % EPT == 0 && aligned(x_lower, al) && aligned(x_higher, al) && aligned(x_prev, al);
    if (v)
      hipLaunchKernelGGL((adaptive_error_kernel2<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x_lower,
                         (const T*)x_higher, (const T*)x_prev, (float)a->d.atol, (float)a->d.rtol, per_sample, (int)G,
                         a->partial, a->counters, e_dev, &a->dev->done);
    else
      hipLaunchKernelGGL((adaptive_error_kernel2<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x_lower,
                         (const T*)x_higher, (const T*)x_prev, (float)a->d.atol, (float)a->d.rtol, per_sample, (int)G,
                         a->partial, a->counters, e_dev, &a->dev->done);
  });
  return rc ? rc : launch_status("adaptive_error");
}

extern "C" int dpm_adaptive_done_at(const dpm_adaptive* a, int begin_index) {
  if (!a || begin_index < 0) return -1;
  const volatile int32_t* s = a->status;
  return s[8 + (begin_index & 31)];
}

extern "C" int dpm_adaptive_poll(const dpm_adaptive* a, int* done, int* nfe, int* iterations, int* accepted) {
  if (!a) return dpm_set_error(DPM_ERR_ARG, "adaptive_poll: null handle");
  const volatile int32_t* s = a->status;
  if (done) *done = s[0];
  if (nfe) *nfe = s[1];
  if (iterations) *iterations = s[2];
  if (accepted) *accepted = s[3];
  return DPM_OK;
}

// ------------------------------------------------------------------------------------------------
// hipGraph capture of a trajectory (dpm_plan_run under stream capture)
// ------------------------------------------------------------------------------------------------
struct dpm_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int result = -1;
  int nodes = 0;
};

extern "C" int dpm_graph_create(const dpm_plan* p, const dpm_run_buffers* rb, dpm_model_cb model, void* user, void* stream,
                                dpm_graph** out) {
  if (!p || !rb || !out) return dpm_set_error(DPM_ERR_ARG, "graph_create: null pointer");
  if (!stream) return dpm_set_error(DPM_ERR_ARG, "graph_create: capture needs a non-null stream");
  hipStream_t st = static_cast<hipStream_t>(stream);
  (void)device_info();  // query device properties before the capture starts
  dpm_graph* g = new (std::nothrow) dpm_graph;
  if (!g) return dpm_set_error(DPM_ERR_NOMEM, "out of memory");
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) {
    delete g;
    return dpm_set_error((int)e, "hipStreamBeginCapture: %s", hipGetErrorString(e));
  }
  const int rc = dpm_plan_run(p, rb, model, user, stream, &g->result);
  e = hipStreamEndCapture(st, &g->graph);  // always end the capture, also after a failed launch
  if (rc) {
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return rc;
  }
  if (e != hipSuccess) {
    delete g;
    return dpm_set_error((int)e, "hipStreamEndCapture: %s", hipGetErrorString(e));
  }
  size_t nn = 0;
  if (hipGraphGetNodes(g->graph, nullptr, &nn) == hipSuccess) g->nodes = (int)nn;
  e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g->graph);
    delete g;
    return dpm_set_error((int)e, "hipGraphInstantiate: %s", hipGetErrorString(e));
  }
  *out = g;
  return DPM_OK;
}

extern "C" int dpm_graph_launch(dpm_graph* g, void* stream) {
  if (!g || !g->exec) return dpm_set_error(DPM_ERR_ARG, "graph_launch: null graph");
  hipError_t e = hipGraphLaunch(g->exec, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return dpm_set_error((int)e, "hipGraphLaunch: %s", hipGetErrorString(e));
  return DPM_OK;
}

extern "C" int dpm_graph_result(const dpm_graph* g) { return g ? g->result : -1; }
extern "C" int dpm_graph_num_nodes(const dpm_graph* g) { return g ? g->nodes : 0; }

extern "C" void dpm_graph_destroy(dpm_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
}

extern "C" int dpm_cluster_timeout_poll(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  uint32_t* w = cluster_fault_word(dev, false);
  if (!w || !*w) return 0;
  *w = 0u;
  return 1;
}

extern "C" int dpm_device_info(int* n_cu, int* lds_bytes, char* arch, int arch_len) {
  const DeviceInfo& di = device_info();
  if (!di.ok) return dpm_set_error((int)hipErrorNoDevice, "no HIP device available");
  if (n_cu) *n_cu = di.n_cu;
  if (lds_bytes) *lds_bytes = di.lds;
  if (arch && arch_len > 0) {
    std::strncpy(arch, di.arch, arch_len - 1);
    arch[arch_len - 1] = 0;
  }
  return DPM_OK;
}

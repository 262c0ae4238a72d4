// dpm_stage_unit.hip -- the stage kernels of one (state dtype, network-output dtype) pair, half of its update forms per
// translation unit: compiled fifty times, with -DDPM_PAIR=<row of DPM_PAIRS> -DDPM_UNIT=<0|1|2|3|4|5|6|7|8|9> (__graft_entry__.py).
//   unit A (0): the TWO and SS3T forms (FORMS_A), the fused multi-request launcher and the pair's catch-all kernels
//   unit B (1): the LIN1, MS3, DENOISE and UNIPC forms (FORMS_B) and the heterogeneous fused launcher (stage_kernel_het,
//               stage_kernel_het_noise, stage_kernel_het_unipc) with its mixed-shape sibling (stage_kernel_shapes,
//               stage_kernel_shapes_noise, stage_kernel_shapes_unipc)
//   unit C (2): the launches of the table's plain / UniPC, SDE and thresholded rows (stage_kernel_table, stage_kernel_table_unipc,
//               stage_kernel_table_noise, stage_thresh_kernel_table) and nothing else -- a unit of its own, so that units A and
//               B compile to the code they compiled to before it existed
//   unit D (3): the launch of the table's mask-blend rows (stage_kernel_table_blend, DPM_TABLE_BLEND) and nothing else --
//               again a unit of its own: units A, B and C compile to the code they compiled to before it existed
//   unit E (4): the launch of a guidance-rescale stage (stage_rescale_kernel, DPM_F_CFG_RESCALE; dpm_rescale_kernel.hpp, which
//               no other unit includes) and of the table's guidance-rescale rows (stage_rescale_kernel_table, DPM_TABLE_RESCALE;
//               dpm_table_rescale.hpp) and nothing else -- units A to D compile to the code they compiled to before it existed
//   unit F (5): the launch of an adaptive-projected-guidance stage (stage_apg_kernel, DPM_F_CFG_APG; dpm_apg_kernel.hpp, which
//               no other unit includes) and of the table's adaptive-projected-guidance rows (stage_apg_kernel_table,
//               DPM_TABLE_APG; dpm_table_apg.hpp) and nothing else -- units A to E compile to the code they compiled to before
//               it existed
//   unit G (6): the launch of a CFG-Zero* stage (stage_zstar_kernel, DPM_F_CFG_ZSTAR; dpm_zstar_kernel.hpp, which no other unit
//               includes) and of the table's CFG-Zero* rows (stage_zstar_kernel_table, DPM_TABLE_ZSTAR; dpm_table_zstar.hpp) and
//               nothing else -- units A to F compile to the code they compiled to before it existed
//   unit H (7): the launch of a stage under guidance over two conditions (stage_pair_kernel, DPM_GUIDE_CFG2; dpm_pair_kernel.hpp,
//               which no other unit includes) and of the table's two-condition rows (stage_pair_kernel_table, DPM_TABLE_PAIR;
//               dpm_table_pair.hpp) and nothing else -- units A to G compile to the code they compiled to before it existed
//   unit I (8): the launch of a Perp-Neg stage (stage_perp_kernel, DPM_F_CFG2_PERP on a DPM_GUIDE_CFG2 record;
//               dpm_perp_kernel.hpp) and nothing else -- units A to H compile to the code they compiled to before it existed
//   unit J (9): the launch of the table's Perp-Neg rows (stage_perp_kernel_table, DPM_TABLE_PERP; dpm_table_perp.hpp, on
//               dpm_perp_kernel.hpp's perp_sample) and nothing else.  Not in unit I, where units E to H keep their table
//               siblings: with the table kernel beside it in one module the compiler schedules the lone stage_perp_kernel
//               differently (same instructions, another order and register assignment), and the lone kernel keeps the code
//               it had (profiles/r33_slab_perp_neg.md)
// Units E, F, G, I and J are the kernels that own a whole sample; they share dpm_sample_frame.hpp, which no other unit includes.
// Filling a table (DPM_TABLE_FILL) is host code without a dtype and lives in no unit: dpm_kernels.hip calls it directly.
#if !defined(DPM_PAIR) || !defined(DPM_UNIT)
#error "dpm_stage_unit.hip is compiled with -DDPM_PAIR=<row> -DDPM_UNIT=<0|1|2|3|4|5|6|7|8|9>"
#endif
#if DPM_UNIT == 0
#define DPM_CATCHALL_HOME
#endif
#include "dpm_device.hpp"
#if DPM_UNIT == 4
#include "dpm_sample_frame.hpp"
#include "dpm_rescale_kernel.hpp"
#include "dpm_table_rescale.hpp"
#endif
#if DPM_UNIT == 5
#include "dpm_sample_frame.hpp"
#include "dpm_apg_kernel.hpp"
#include "dpm_table_apg.hpp"
#endif
#if DPM_UNIT == 6
#include "dpm_sample_frame.hpp"
#include "dpm_zstar_kernel.hpp"
#include "dpm_table_zstar.hpp"
#endif
#if DPM_UNIT == 7
#include "dpm_pair_kernel.hpp"
#include "dpm_table_pair.hpp"
#endif
#if DPM_UNIT == 8
#include "dpm_sample_frame.hpp"
#include "dpm_perp_kernel.hpp"
#endif
#if DPM_UNIT == 9
#include "dpm_sample_frame.hpp"
#include "dpm_perp_kernel.hpp"
#include "dpm_table_perp.hpp"
#endif

#include <tuple>
#include <utility>

#define DPM_PAIR_TYPES(name, TS, TE, SD, ED) std::pair<TS, TE>,
using Pair = std::tuple_element_t<DPM_PAIR, std::tuple<DPM_PAIRS(DPM_PAIR_TYPES) void>>;
#undef DPM_PAIR_TYPES
using State = Pair::first_type;  // the pair's state dtype
using Eps = Pair::second_type;   // ... and network-output dtype

#if DPM_UNIT == 0
template const void* dpm_catchall_thresh<State, Eps>();
template const void* dpm_catchall_scalar<State, Eps, false>();
template const void* dpm_catchall_scalar<State, Eps, true>();
template const void* dpm_catchall_scalar_noise<State, Eps>();
template const void* dpm_catchall_scalar_unipc<State, Eps>();
#endif

#if DPM_UNIT < 2
template <typename TS, typename TE, unsigned FORMS>
int dpm_launch_unit(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop,
                    const dpm_stage* dyn, const int32_t* skip, const dpm_buffers* multi, int n_multi) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop),
                    dyn, skip, multi, n_multi};
  return launch_form<TS, TE, FORMS>(st, b, s);
}
template int dpm_launch_unit<State, Eps, DPM_UNIT == 0 ? FORMS_A : FORMS_B>(const dpm_stage*, const dpm_buffers*, void*,
                                                                             void*, void*, const dpm_stage*, const int32_t*,
                                                                             const dpm_buffers*, int);
#endif

#if DPM_UNIT == 0
template <typename TS, typename TE>
int dpm_launch_fused(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, void* ev_start, void* ev_stop) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)};
  return launch_multi_typed<TS, TE>(st, bs, n_req, s);
}
template int dpm_launch_fused<State, Eps>(const dpm_stage*, const dpm_buffers*, int, void*, void*, void*);
#endif

#if DPM_UNIT == 1
template <typename TS, typename TE>
int dpm_launch_het(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_het_typed<TS, TE>(st, bs, n_req, s);
}
template int dpm_launch_het<State, Eps>(const dpm_stage*, const dpm_buffers*, int, void*);

template <typename TS, typename TE>
int dpm_launch_het_shapes(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_het_shapes_typed<TS, TE>(st, bs, n_req, s);
}
template int dpm_launch_het_shapes<State, Eps>(const dpm_stage*, const dpm_buffers*, int, void*);
#endif

// The launches of the table's row kinds (dpm_kernels.hip: kRowKinds), all of one signature: the group's run of rows and, for a
// kind that has them, its records, both in DEVICE memory.  (DPM_TABLE_FILL needs no dtype: the walk calls table_fill_rows and the
// kind's record fill itself.)
#if DPM_UNIT == 2
template <typename TS, typename TE>
int dpm_table_launch(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void*, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_typed<TS, TE>(st, bs, n_req, rows, s);
}
template int dpm_table_launch<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);

template <typename TS, typename TE>
int dpm_table_launch_noise(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_noise_typed<TS, TE>(st, bs, n_req, rows, recs, s);
}
template int dpm_table_launch_noise<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);

template <typename TS, typename TE>
int dpm_table_launch_thresh(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void*, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_thresh_typed<TS, TE>(st, bs, n_req, rows, s);
}
template int dpm_table_launch_thresh<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

#if DPM_UNIT == 3
template <typename TS, typename TE>
int dpm_table_launch_blend(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_blend_typed<TS, TE>(st, bs, n_req, rows, recs, s);
}
template int dpm_table_launch_blend<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

// The launch of a per-sample guidance stage (dpm_kernels.hip: kSampleGuidance), FLAG the unit's own.
#if DPM_UNIT == 4 || DPM_UNIT == 5 || DPM_UNIT == 6
template <typename TS, typename TE, unsigned FLAG>
int dpm_launch_sample(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)};
  return launch_sample_typed<TS, TE>(st, b, s);  // (the one of the unit's kernel header)
}
template int dpm_launch_sample<State, Eps, DPM_UNIT == 4 ? DPM_F_CFG_RESCALE : DPM_UNIT == 5 ? DPM_F_CFG_APG : DPM_F_CFG_ZSTAR>(
    const dpm_stage*, const dpm_buffers*, void*, void*, void*);
#endif

#if DPM_UNIT == 4
template <typename TS, typename TE>
int dpm_table_launch_rescale(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void*, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_rescale_typed<TS, TE>(st, bs, n_req, rows, s);
}
template int dpm_table_launch_rescale<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

#if DPM_UNIT == 5
template <typename TS, typename TE>
int dpm_table_launch_apg(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_apg_typed<TS, TE>(st, bs, n_req, rows, recs, s);
}
template int dpm_table_launch_apg<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

#if DPM_UNIT == 6
template <typename TS, typename TE>
int dpm_table_launch_zstar(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void*, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_zstar_typed<TS, TE>(st, bs, n_req, rows, s);
}
template int dpm_table_launch_zstar<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

// The launch of a stage under guidance over two conditions (DPM_GUIDE_CFG2), checked by dpm_stage_launch.
#if DPM_UNIT == 7
template <typename TS, typename TE>
int dpm_launch_pair(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)};
  return launch_pair_typed<TS, TE>(st, b, s);
}
template int dpm_launch_pair<State, Eps>(const dpm_stage*, const dpm_buffers*, void*, void*, void*);
#endif

#if DPM_UNIT == 7
template <typename TS, typename TE>
int dpm_table_launch_pair(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_pair_typed<TS, TE>(st, bs, n_req, rows, recs, s);
}
template int dpm_table_launch_pair<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

// The launch of a Perp-Neg stage (DPM_F_CFG2_PERP under DPM_GUIDE_CFG2), checked by dpm_stage_launch.
#if DPM_UNIT == 8
template <typename TS, typename TE>
int dpm_launch_perp(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)};
  return launch_perp_typed<TS, TE>(st, b, s);
}
template int dpm_launch_perp<State, Eps>(const dpm_stage*, const dpm_buffers*, void*, void*, void*);
#endif

#if DPM_UNIT == 9
template <typename TS, typename TE>
int dpm_table_launch_perp(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream) {
  const LaunchCtx s{static_cast<hipStream_t>(stream), nullptr, nullptr};
  return launch_table_perp_typed<TS, TE>(st, bs, n_req, rows, recs, s);
}
template int dpm_table_launch_perp<State, Eps>(const dpm_stage*, const dpm_buffers*, int, const void*, const void*, void*);
#endif

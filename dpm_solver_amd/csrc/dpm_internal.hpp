// dpm_internal.hpp -- what the library's translation units share with each other and nothing else: the list of
// (state dtype, network-output dtype) pairs the stage kernels are built for, and ONE declaration of every function that
// is defined in one translation unit and called from another.  Included by dpm_device.hpp and by dpm_host.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dpm_hip.h"

// The dtype pairs: name (the build's object files dpm_stage_<name>.o / dpm_stage_<name>_b.o), state type, network-output
// type, their DPM_DTYPE_* codes.  Row i is compiled by dpm_stage_unit.hip with -DDPM_PAIR=i, so the order is the one of
// __graft_entry__._PAIRS (the slowest units first).  The types are those of dpm_device.hpp.
#define DPM_PAIRS(X)                                                         \
  X(f32_bf16, float, dpmk::bf16_t, DPM_DTYPE_F32, DPM_DTYPE_BF16)            \
  X(f32_f16, float, __half, DPM_DTYPE_F32, DPM_DTYPE_F16)                    \
  X(f32_f32, float, float, DPM_DTYPE_F32, DPM_DTYPE_F32)                     \
  X(bf16_bf16, dpmk::bf16_t, dpmk::bf16_t, DPM_DTYPE_BF16, DPM_DTYPE_BF16)   \
  X(f16_f16, __half, __half, DPM_DTYPE_F16, DPM_DTYPE_F16)

// The single-request launchers of one dtype pair are spread over two translation units (compile time: the build is the
// slowest unit), split by update form (bit f = form f).  Unit A also holds the fused multi-request launcher and the
// pair's catch-all kernels, unit B the heterogeneous fused launchers, unit C (2) the table-driven ones, unit D (3) the
// table-driven launch's mask-blend rows, unit E (4) the guidance-rescale stage, unit F (5) the adaptive-projected-guidance stage,
// unit G (6) the CFG-Zero* stage, unit H (7) the stage under guidance over two conditions, unit I (8) the Perp-Neg stage.
constexpr unsigned FORMS_A = (1u << DPM_FORM_TWO) | (1u << DPM_FORM_SS3T);
constexpr unsigned FORMS_B = (1u << DPM_FORM_LIN1) | (1u << DPM_FORM_MS3) | (1u << DPM_FORM_DENOISE) | (1u << DPM_FORM_UNIPC);

// ---- dpm_stage_unit.hip, instantiated once per pair and unit
// one stage of the forms in FORMS; `multi` / n_multi: a thresholded stage of n_multi requests fused into one launch
template <typename TS, typename TE, unsigned FORMS>
int dpm_launch_unit(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop,
                    const dpm_stage* dyn, const int32_t* skip, const dpm_buffers* multi, int n_multi);
// one stage of n_req requests in one launch of the streaming family; MULTI_NOT_BUILT when it has no fused variant
template <typename TS, typename TE>
int dpm_launch_fused(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, void* ev_start, void* ev_stop);
// (unit B) one heterogeneous fused launch: request r advanced by st[r]; the requests are grouped by the caller
template <typename TS, typename TE>
int dpm_launch_het(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream);
// (unit B) the same for a group whose members differ in n (dpm_launch_opts.fuse_shapes); MULTI_NOT_BUILT when the group's
// tile space does not fit the kernel's 32-bit index
template <typename TS, typename TE>
int dpm_launch_het_shapes(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream);

// (unit C) the table of dpm_launch_opts.table_mode (include/dpm_hip.h): a 16-byte header, then rows of 8 pointers and the
// kernels' 80-byte stage scalars (TableRow, dpm_table_kernel.hpp)
constexpr size_t DPM_TABLE_HEADER_BYTES = 16, DPM_TABLE_ROW_BYTES = 8 * 8 + 80;
// Behind the rows: the noise records of a DPM_TABLE_NOISE call (DPM_TABLE_NOISE_BYTES each: KNoiseTab, dpm_stage_kernel.hpp),
// behind those the blend records of a DPM_TABLE_BLEND call (DPM_TABLE_BLEND_BYTES each: KBlendTab, dpm_table_blend.hpp),
// behind those the APG records of a DPM_TABLE_APG call (DPM_TABLE_APG_BYTES each: KApgTab, dpm_table_kernel.hpp).
// DPM_TABLE_FILL is host code without a dtype (table_fill_rows and
// the record fills, called by dpm_kernels.hip itself); DPM_TABLE_LAUNCH is ONE launch per group, one launcher per row kind, all of
// one signature: the group's run of rows and its records (null for a kind without records) in DEVICE memory.
// plain and UniPC rows
template <typename TS, typename TE>
int dpm_table_launch(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (DPM_TABLE_NOISE) SDE rows and their noise records
template <typename TS, typename TE>
int dpm_table_launch_noise(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (DPM_TABLE_THRESH) thresholded rows -- rows like any other, no records --, one workgroup per sample
template <typename TS, typename TE>
int dpm_table_launch_thresh(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (unit D, DPM_TABLE_BLEND) DPM_F_BLEND rows and their blend records
template <typename TS, typename TE>
int dpm_table_launch_blend(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);

// one classifier-free stage under a per-sample guidance FLAG, one workgroup per sample: DPM_F_CFG_RESCALE (unit E, guidance
// rescale, stage_rescale_kernel), DPM_F_CFG_APG (unit F, adaptive projected guidance, stage_apg_kernel) or DPM_F_CFG_ZSTAR
// (unit G, CFG-Zero*, stage_zstar_kernel)
template <typename TS, typename TE, unsigned FLAG>
int dpm_launch_sample(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop);
// (unit E, DPM_TABLE_RESCALE) DPM_F_CFG_RESCALE rows -- rows like any other, no records --, one workgroup per sample
template <typename TS, typename TE>
int dpm_table_launch_rescale(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (unit F, DPM_TABLE_APG) DPM_F_CFG_APG rows and their APG records, one workgroup per sample
template <typename TS, typename TE>
int dpm_table_launch_apg(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (unit G, DPM_TABLE_ZSTAR) DPM_F_CFG_ZSTAR rows -- rows like any other, no records --, one workgroup per sample
template <typename TS, typename TE>
int dpm_table_launch_zstar(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (unit H) one stage under guidance over two conditions (DPM_GUIDE_CFG2, stage_pair_kernel): three network outputs, streaming
template <typename TS, typename TE>
int dpm_launch_pair(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop);
// (unit H, DPM_TABLE_PAIR) DPM_GUIDE_CFG2 rows and their pair records (DPM_TABLE_PAIR_BYTES each: KPairTab, dpm_table_kernel.hpp;
// behind the APG records), one super-tile per 256-lane group as the plain rows
template <typename TS, typename TE>
int dpm_table_launch_pair(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);
// (unit I) one Perp-Neg stage (DPM_F_CFG2_PERP under DPM_GUIDE_CFG2, stage_perp_kernel): three network outputs, one workgroup
// per sample
template <typename TS, typename TE>
int dpm_launch_perp(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop);
// (unit J, DPM_TABLE_PERP) DPM_F_CFG2_PERP rows and their pair records (the pair records' section), one workgroup per sample
template <typename TS, typename TE>
int dpm_table_launch_perp(const dpm_stage* st, const dpm_buffers* bs, int n_req, const void* rows, const void* recs, void* stream);

// ---- dpm_f64.hip
int dpm_launch_f64(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop);
int dpm_add_noise_f64(double alpha, double sigma, const void* x, const void* noise, void* out, int64_t n, void* stream);
int dpm_blend_f64(const void* x, const void* mask, const void* a, const void* b, double alpha, double sigma, void* out,
                  int64_t n, int64_t mask_period, void* stream);

// ---- dpm_kernels.hip
int dpm_stage_launch_dyn(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop,
                         const dpm_stage* dyn, const int32_t* skip);
int dpm_stage_launch_ev(const dpm_stage* st, const dpm_buffers* b, void* stream, void* ev_start, void* ev_stop);
int dpm_stage_launch_multi_ev(const dpm_stage* st, const dpm_buffers* bs, int n_req, void* stream, void** ev_start,
                              void** ev_stop, int* fused_first);
int dpm_timing_begin(int n, void*** starts, void*** stops);
int dpm_timing_end(int n, void** starts, void** stops, void* stream, float* ms, const unsigned char* recorded);

// ---- dpm_host.cpp
namespace dpmc {
template <class T>
struct SchedViewT;
}
int dpm_set_error(int code, const char* fmt, ...);
int dpm_schedule_table_is_f64(const dpm_schedule* s);
dpmc::SchedViewT<float> dpm_schedule_view(const dpm_schedule* s);

// dpm_thresh_plan.hpp -- the host-side plan of a thresholded stage (stage_thresh_kernel): the constants it reads, ThrParams,
// the cluster shape, the workspace size and thr_launch_plan, every number the launch works out before it chooses a kernel.
// Plain C++17: the standard library and include/dpm_hip.h, nothing of HIP -- so that a host compiler and a CPU test
// (tests/test_thr_plan_host.py) reach it.  Included by dpm_thresh_common.hpp, where the layout constants are explained.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "dpm_hip.h"

#ifndef DPM_LAB
#define DPM_LAB 0
#endif

namespace {

constexpr int THR_THREADS = 512;
constexpr int THR_NB = 2048;                 // bins per radix level
// workspace words per sample (k > 1): 3 level histograms, the histogram of the per-thread maxima and the candidate list
// of the top-K front end, counters (a 256-byte multiple)
constexpr int THR_WS_WORDS = 5 * THR_NB + 64;
constexpr int THR_CHUNK_MAX = 12288;         // elements of a sample one workgroup keeps in LDS (48 KiB)
constexpr int THR_CAP = 4096;                // candidates (elements sharing the selected top digit) kept compacted
constexpr int THR_KMAX = 256;                // largest cluster the single-exchange route serves
constexpr int THR_MISC = 32 + 2 * THR_KMAX;  // scalar LDS words of the thresholding kernel (see stage_thresh_kernel)
constexpr int THR_SLOT_CAP = 256;            // values one workgroup may publish
constexpr int THR_SLOT_HDR = 8;              // [0] tag | count (or overflow), [1] tag | bound, [2] tag | chunk maximum
constexpr int THR_SLOTW = THR_SLOT_CAP + THR_SLOT_HDR;  // (128-byte aligned slots, 288 words, were measured: no difference)

struct ThrParams {
  int64_t per_sample;
  int32_t lo, hi;  // floor / ceil of the fp32 rank (ascending order)
  float w;         // fractional part
  float max_val;
  int32_t chunk;   // elements per workgroup of a cluster (multiple of 4 when the vector path is on)
  int32_t k;       // workgroups per cluster
  int32_t groups;  // clusters in the grid
  int32_t batch;
  int32_t vec;     // 1: 4-element vector accesses are legal for every tensor of this launch
  int32_t topk;    // > 0: K = per_sample - lo is small enough for the top-K front end of the select
  int32_t mrank;   // top-K: ascending rank of the K-th largest per-thread maximum among the contributing threads
  int32_t fastdiv; // 1: noise-prediction network + eps -> x0 with a divisor that passes div_invariant_ok (see div_by_alpha)
  int32_t quota;   // > 0: single-exchange cluster route; values beyond this rank of the per-thread maxima are not published
  int32_t kbig;    // K = per_sample - lo (the wanted element is the K-th largest of the sample)
  int32_t bpr;      // > 0: the launch fuses several requests of bpr samples each (ThrTab); sample s belongs to request s / bpr
  int32_t slot_pub; // entries of a slot that are always written (values, then the bare tag)
  int32_t slot_cap; // values per workgroup slot: a power of two <= THR_SLOT_CAP with k * slot_cap <= THR_CAP
  int32_t slot_shift; // log2(slot_cap)
  int32_t debug_reject; // testing: run the single-exchange select but always take the general route afterwards
  int64_t ws_stride; // words per sample in ws
  uint32_t* ws;    // k > 1: batch x ws_stride words, all zero between launches (the kernel cleans up after itself)
  uint32_t* fault; // host-mapped word: set when a cluster wait timed out and was recovered from (diagnostics only:
                   // dpm_cluster_timeout_poll; the launch's results are correct either way)
  uint32_t spin_limit;  // polls before a wait on a peer gives up (THR_SPIN_LIMIT)
#if DPM_LAB
  int32_t debug_fault;  // LAB build only (DPM_TUNE_THR_DEBUG_FAULT): 2 / 3 = workgroup 1 of every cluster takes no part in its cluster
  int32_t elect;        // LAB build only (DPM_TUNE_THR_ELECT): workgroup 0 of a cluster reads the k slots, selects on the union
                        // and publishes the verdict; its peers make one wait and read three words -- k slot reads per sample
                        // instead of k^2 (profiles/r05_thresholding.md)
  int32_t stagger;      // LAB build only (DPM_TUNE_THR_STAGGER): cluster g starts (g % groups) * ticks of 0.1 us late -- low 16
                        // bits = ticks, high bits = groups (0 = 2): clusters that walk several large samples stay out of
                        // phase, so that one group streams while another selects (profiles/r05_thresholding.md)
#endif
  float* hint;     // dpm_buffers.thr_hint (THR_HINT_W floats per sample) or null: the selected order statistic of the
                   // previous two stages -> predicted select bound of this one (cluster_select_once, `pbound`)
  int32_t hint_reset; // this is the first stage of a trajectory: the stored values are stale, overwrite without reading
  int32_t hint_predict; // 0: maintain the hint but do not use it (DPM_TUNE_THR_PREDICT)
#ifdef DPM_THR_TIMING  // (lab build only)
  uint64_t* tdbg;  // 16 timestamps per workgroup (tools/thr_timeline.py)
#endif
};

// cluster shape of the thresholding kernel: k workgroups per sample, `chunk` elements each.  Depends only on the
// batch, the sample size and the CU count, so dpm_threshold_workspace_bytes() and the launch agree.
struct ThrPlan {
  int64_t k, chunk;
};
inline ThrPlan thr_plan(int64_t batch, int64_t per_sample, int n_cu) {
  const int64_t kmin = (per_sample + THR_CHUNK_MAX - 1) / THR_CHUNK_MAX;        // what LDS allows
  const int64_t kfill = (2 * (int64_t)n_cu) / (batch < 1 ? 1 : batch);          // spread a small batch over the chip
  const int64_t kmax = std::max<int64_t>(1, per_sample / 2048);                 // but keep >= 2 elements per lane
  int64_t k = std::max(kmin, std::min(std::min(kfill, kmax), (int64_t)n_cu));
  if (k < 1) k = 1;
  int64_t chunk = (per_sample + k - 1) / k;
  chunk = (chunk + 3) / 4 * 4;
  return ThrPlan{k, chunk};
}
// words per sample: the merged histograms / lists / counters of the general route + one slot per workgroup of the cluster
// (two slot areas: the attempt with a predicted bound and the one with a searched bound each publish into their own)
inline int64_t thr_ws_stride(int64_t k) { return (int64_t)THR_WS_WORDS + 2 * k * (int64_t)THR_SLOTW; }
inline int64_t thr_ws_bytes(int64_t batch, int64_t per_sample, int n_cu) {
  const ThrPlan pl = thr_plan(batch, per_sample, n_cu);
  return pl.k > 1 ? batch * thr_ws_stride(pl.k) * 4 : 0;
}

// the two tuning parameters the plan reads (Tuning, dpm_device.hpp)
struct ThrKnobs {
  int cluster_in_graph, cluster_one_hop;
};

// what thr_launch_plan works out: the numeric fields of ThrParams (the pointers, groups, bpr, spin_limit and the LAB
// fields stay zero: launch_thresh sets them), the cluster shape in 64 bits, the dynamic LDS size; err != 0: batch /
// sample size out of range, nothing else is filled in
struct ThrLaunchPlan {
  ThrParams tp;
  int64_t k, chunk;
  size_t lds_bytes;
  int err;
};

// The plan of one thresholded launch of `batch` samples of `per_sample` elements: cluster shape, quantile rank, select
// route (top-K front end, single-exchange quota and slot geometry), workspace stride.  `vec`: 4-element accesses are
// legal for every tensor; `fastdiv`: x0_prologue_ok of the stage.  `one_wg`: the caller's kernel has no clusters (the table
// rows of DPM_TABLE_THRESH) -- one workgroup per sample whatever the batch; per_sample beyond THR_CHUNK_MAX is out of range.
inline ThrLaunchPlan thr_launch_plan(const dpm_stage& st, int64_t batch, int64_t per_sample, int n_cu, ThrKnobs tn,
                                     bool capturing, bool vec, bool fastdiv, bool one_wg = false) {
  ThrLaunchPlan lp;
  std::memset(&lp, 0, sizeof lp);
  if (batch > 0x7fffffff || per_sample > ((int64_t)1 << 40)) {
    lp.err = 1;
    return lp;
  }
  ThrPlan pl = thr_plan(batch, per_sample, n_cu);
  // Clusters wait for each other inside the kernel, which is only safe while no OTHER clustered launch can hold part of
  // the chip at the same time.  Eager launches of this process are chained device-wide (launch_thresh); a captured graph is
  // replayed outside that chain, possibly next to another graph on another stream.  Under capture a sample that fits
  // one workgroup's LDS therefore takes the cluster-free shape (one workgroup per sample) unless the caller opts in
  // (dpm_launch_opts.cluster_in_graph); larger samples have no such shape and keep their clusters, with bounded waits.
  if (((capturing && !tn.cluster_in_graph) || one_wg) && pl.k > 1 && per_sample <= THR_CHUNK_MAX) {
    pl.k = 1;
    pl.chunk = (per_sample + 3) / 4 * 4;
  }
  if (one_wg && pl.k > 1) {
    lp.err = 1;
    return lp;
  }
  ThrParams& tp = lp.tp;
  tp.per_sample = per_sample;
  // torch.quantile: rank = q * (n - 1) evaluated in fp32 (q is an fp32 tensor)
  const float rank = st.thr_ratio * (float)(per_sample - 1);
  tp.lo = (int32_t)floorf(rank);
  tp.hi = (int32_t)ceilf(rank);
  tp.w = rank - (float)tp.lo;
  tp.max_val = st.thr_max;
  tp.chunk = (int32_t)pl.chunk;
  tp.k = (int32_t)pl.k;
  tp.batch = (int32_t)batch;
  tp.fastdiv = fastdiv;
  tp.vec = vec;
  {
    // top-K front end: a = the K-th largest element.  It needs at most one wanted element per contributing thread and
    // pays when the K-th largest per-thread maximum sits in the sparse upper tail (K a small part of the threads) and
    // the candidates (a small multiple of K) fit the rank-counting finish (<= THR_THREADS of them).
    const int64_t K = per_sample - (int64_t)tp.lo;
    int64_t P = 0;
    for (int64_t c = 0; c < pl.k; ++c) {
      const int64_t n_c = std::max<int64_t>(0, std::min<int64_t>(pl.chunk, per_sample - c * pl.chunk));
      P += std::min<int64_t>(THR_THREADS, tp.vec ? (n_c + 3) / 4 : n_c);
    }
    if (K >= 1 && K <= P / 4 && K <= THR_THREADS / 4) {  // beyond: the candidates outgrow the rank-counting finish
      tp.topk = (int32_t)K;
      tp.mrank = (int32_t)(P - K);
    }
    // single-exchange cluster route (cluster_select_once): a chunk's share of the K largest is ~ K/k; publishing the
    // ~quota = K/k + 6 sigma + 8 largest values of every chunk makes the one-hop answer exact except for samples whose
    // large values sit in one chunk (those fall back inside the kernel).  Needs room in the slots for the 14-bit digit's
    // granularity (x1.5) and a union that fits the LDS list.
    if (pl.k > 1 && pl.k <= THR_KMAX && K >= 1 && K < ((int64_t)1 << 30)) {
      const double mu = (double)K / (double)pl.k;
      const int64_t quota = (int64_t)std::ceil(mu + 6.0 * std::sqrt(mu) + 8.0);
      // slot size: the smallest power of two >= 64 with room for the quota and the digit granularity (fewer words to
      // fetch per slot); at most THR_SLOT_CAP and THR_CAP / k
      int slot_shift = 6;
      while (((int64_t)1 << slot_shift) < quota * 3 / 2 && slot_shift < 8) ++slot_shift;
      while (slot_shift > 0 && ((int64_t)1 << slot_shift) > std::min<int64_t>(THR_SLOT_CAP, THR_CAP / pl.k)) --slot_shift;
      const int64_t slot_cap = (int64_t)1 << slot_shift;
      if (quota * 3 / 2 <= slot_cap && tn.cluster_one_hop) {
        tp.quota = (int32_t)quota;
        tp.kbig = (int32_t)K;
        tp.slot_cap = (int32_t)slot_cap;
        tp.slot_pub = (int32_t)std::min<int64_t>(slot_cap, quota + quota / 4 + 4);
        tp.slot_shift = slot_shift;
        tp.debug_reject = tn.cluster_one_hop == 2;
      }
    }
  }
  if (pl.k > 1) tp.ws_stride = thr_ws_stride(pl.k);
  lp.k = pl.k;
  lp.chunk = pl.chunk;
  lp.lds_bytes = (size_t)pl.chunk * 4 + THR_NB * 4 + THR_MISC * 4 + (THR_CAP + 32) * 4;
  return lp;
}

}  // namespace

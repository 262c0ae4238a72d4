// thr_plan_driver.cpp -- stand-alone host program around thr_launch_plan (csrc/dpm_thresh_plan.hpp), built and run by
// tests/test_thr_plan_host.py.  One case per line of standard input:
//   batch per_sample thr_ratio thr_max n_cu cluster_in_graph cluster_one_hop capturing vec fastdiv
// one line of "name=value" pairs per case on standard output (floats as their bit patterns).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dpm_thresh_plan.hpp"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    long long batch, per_sample;
    float ratio, max_val;
    int n_cu, in_graph, one_hop, capturing, vec, fastdiv;
    if (std::sscanf(line, "%lld %lld %f %f %d %d %d %d %d %d", &batch, &per_sample, &ratio, &max_val, &n_cu, &in_graph, &one_hop,
                    &capturing, &vec, &fastdiv) != 10)
      continue;
    dpm_stage st;
    std::memset(&st, 0, sizeof st);
    st.thr_ratio = ratio;
    st.thr_max = max_val;
    const ThrLaunchPlan lp = thr_launch_plan(st, batch, per_sample, n_cu, ThrKnobs{in_graph, one_hop}, capturing != 0, vec != 0,
                                             fastdiv != 0);
    const ThrParams& tp = lp.tp;
    std::printf("err=%d k=%" PRId64 " chunk=%" PRId64 " lds_bytes=%zu per_sample=%" PRId64 " lo=%d hi=%d w=%u max_val=%u tp_chunk=%d "
                "tp_k=%d groups=%d batch=%d vec=%d topk=%d mrank=%d fastdiv=%d quota=%d kbig=%d bpr=%d slot_pub=%d slot_cap=%d "
                "slot_shift=%d debug_reject=%d ws_stride=%" PRId64 " ws_bytes=%" PRId64 "\n",
                lp.err, lp.k, lp.chunk, lp.lds_bytes, tp.per_sample, tp.lo, tp.hi, bits(tp.w), bits(tp.max_val), tp.chunk, tp.k,
                tp.groups, tp.batch, tp.vec, tp.topk, tp.mrank, tp.fastdiv, tp.quota, tp.kbig, tp.bpr, tp.slot_pub, tp.slot_cap,
                tp.slot_shift, tp.debug_reject, tp.ws_stride, lp.err ? 0 : thr_ws_bytes(batch, per_sample, n_cu));
  }
  return 0;
}

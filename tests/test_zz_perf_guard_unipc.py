"""Performance guard of the fused UniPC stage (the rule of profiles/r06_perf_guard.md: worst figure measured + 8 %).

Two figures of the PRODUCT library: 32 requests of [256,4,64,64] at the steady UniPC-2 stage (second-order corrector and
second-order predictor) advanced by ONE stage_kernel_multi launch (tools/unipc_stage.py: dpm_plan_run_multi, kernel-only HIP
events, inputs from HBM) -- microseconds per request-stage.  Measured (profiles/r11_unipc.md): fp16 7.05-7.35 us over 21
repeats in three processes, next to 7.14-7.42 for the third-order multistep stage with the same six streams, and 7.56 in a
fourth process on another GPU call (this guard's own first run); fp32
16.18-16.29 us over 7 repeats in one process (16.15-16.31 for the third-order stage).  Request by request the same stage takes
7.8-8.0 us (fp16) with its inputs still cache-resident, and more from HBM, so a launch layer that stops fusing UniPC stages
shows here.  Best of three repeats, up to three attempts (a shared box can be slower than any regression); the figures are
printed (`pytest -s`).  Sorts last, like test_zz_perf_guard.py.
"""
import ctypes as C
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FUSED_UNIPC_MAX_US = {"fp16": 8.16,      # 7.05-7.56 measured; worst + 8 %
                      "fp32": 17.60}     # 16.18-16.29 measured; worst + 8 %


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_fused_unipc_request_stage(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import unipc_stage as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    plans, steady, rbs, keep = T.build(dev, dtype, 32)
    T.run(plans, steady, rbs, 32, "unipc2", stream)            # warm-up

    def measure():
        return min(T.run(plans, steady, rbs, 32, "unipc2", stream) for _ in range(3))
    us = None
    for _ in range(3):
        us = measure()
        if us <= FUSED_UNIPC_MAX_US[dtype]:
            break
        time.sleep(1.0)
    del keep
    print("\n[perf guard] fused UniPC-2 request-stage, 32 x [256,4,64,64] %s: %.2f us" % (dtype, us))
    assert us <= FUSED_UNIPC_MAX_US[dtype], "fused UniPC request-stage: %.2f us > %.2f" % (us, FUSED_UNIPC_MAX_US[dtype])

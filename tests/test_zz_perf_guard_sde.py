"""Performance guard of the fused SDE stage (the rule of profiles/r06_perf_guard.md: worst figure measured + 8 %).

One figure of the PRODUCT library: 32 requests of [256,4,64,64] fp16 at the same "DPM++ 2M SDE" stage, every request with its own
seed, advanced by ONE stage_kernel_multi_noise launch per tick (tools/sde_requests.py, mode a: HIP events around back-to-back
ticks, inputs from HBM) -- microseconds per request-stage.  Measured 6.94-7.09 us in nine runs over three GPU calls, and 7.03-7.21
with the requests staggered (profiles/r10_sde_requests.md); request by request the same stage takes 9.7-9.8 us, so a launch
layer that stops fusing SDE stages fails here whatever the box.  Best of three short regions, up to three attempts (a shared box can be
slower than any regression), and the figure is printed (`pytest -s`).  Sorts last, like test_zz_perf_guard.py.
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

FUSED_SDE_MAX_US = 7.66         # 6.94-7.09 measured (nine runs, three GPU calls); worst + 8 %


def test_fused_sde_request_stage():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import sde_requests as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, recs = T.build(dev, "fp16", True)

    def measure():
        return min(T.run("a", recs, 20, 100, stream)["us_per_request_stage"] for _ in range(3))
    us = None
    for _ in range(3):
        us = measure()
        if us <= FUSED_SDE_MAX_US:
            break
        time.sleep(1.0)
    del keep
    print("\n[perf guard] fused SDE 2M request-stage, 32 x [256,4,64,64] fp16: %.2f us" % us)
    assert us <= FUSED_SDE_MAX_US, "fused SDE request-stage: %.2f us > %.2f" % (us, FUSED_SDE_MAX_US)

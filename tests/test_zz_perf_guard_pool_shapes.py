"""Performance guard of the mixed-shape fused launch (dpm_launch_opts.fuse_shapes), against the parent's behaviour measured in
the same run -- not against a figure of the new code's own.

16 DPM-Solver++(2M) requests `[b,4,64,64]`, b = 16 .. 256, all shapes different, at 16 positions of their 20-step plans, inputs
from HBM (tools/pool_shapes.py).  One tick through dpm_stage_launch_multi with per-request stage records and
  fuse_shapes = 1: one stage_kernel_shapes launch,
  fuse_shapes = 0: what every commit before the flag does with this call -- no two requests agree on n: 16 lone launches.
The fused tick must not be slower than the unfused one by more than 8 %, the noise margin of the project's other guards
(profiles/r06_perf_guard.md).  Measured: profiles/r15_pool_shapes.md.  Best of three short regions per mode, alternating, up to
three attempts (a shared box can be slower than any regression); the figures are printed (`pytest -s`).  The timed regions are
2 x 3 x 60 ticks of 356 MB (fp16) / 713 MB (fp32) of streams; building the 16 requests' records and buffers comes on top.
Sorts last, like test_zz_perf_guard.py.
"""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARGIN = 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_fused_mixed_tick_is_not_slower_than_sixteen_lone_launches(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_shapes as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep, recs = T.build(dev, dtype, "mixed")

    def measure():
        fused, lone = [], []
        for _ in range(3):
            fused.append(T.run(recs, 1, 20, 60, stream)["us_per_tick"])
            lone.append(T.run(recs, 0, 20, 60, stream)["us_per_tick"])
        return min(fused), min(lone)
    fused = lone = None
    for _ in range(3):
        fused, lone = measure()
        if fused <= MARGIN * lone:
            break
    del keep
    print("\n[perf guard] tick of 16 x [16..256,4,64,64] %s: fused %.1f us, 16 lone launches %.1f us (ratio %.3f)"
          % (dtype, fused, lone, fused / lone))
    assert fused <= MARGIN * lone, "mixed-shape tick: fused %.1f us > %.2f x %.1f us request by request" % (fused, MARGIN, lone)

"""Performance guard of mask-blend stages in the table-driven launch (DPM_TABLE_BLEND, stage_kernel_table_blend), pinned at what
was measured.

256 inpainting requests `[1,4,64,64]` at 256 positions of their 20-step 2M plans, every stage with a mask blend -- a full-size
mask, a known image and a noise tensor per row --, rows of slabs, eight sets of slabs in rotation so that every tick's inputs
come from HBM (tools/pool_table_blend.py).  One tick = ONE stage_kernel_table_blend launch (DPM_TABLE_LAUNCH | DPM_TABLE_BLEND on
a device table filled and copied beforehand), HIP events around 600 back-to-back ticks.  The pin is the worst value of the
measuring session's runs + 8 %, the rule and the margin of the project's other guards (profiles/r06_perf_guard.md: box-to-box
spread); the measured values and the pin stand next to each other in profiles/r19_slab_inpaint.md.  Best of three regions, up
to three attempts (a shared box can be slower than any regression); the figures -- and the ODE table tick of the same rows,
for the record -- are printed (`pytest -s`).  Sorts last, like test_zz_perf_guard.py.
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

# us per tick: worst of the session's runs x 1.08 (profiles/r19_slab_inpaint.md)
PIN = {"fp16": 13.74, "fp32": 25.66}      # 12.72 x 1.08, 23.76 x 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_table_blend_tick_of_256_single_image_inpainting_requests_stays_at_its_measured_cost(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_table_blend as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.BlendSlabs(dev, dtype, 256, 8)
    ticks, ode_ticks = slabs.ticks(), slabs.ticks(blend=False)
    T.prefill(ticks, T.BLEND, stream)
    T.prefill(ode_ticks, 0, stream)

    def measure():
        return min(T.run("B", ticks, ode_ticks, 40, 600, stream)["us_per_tick"] for _ in range(3))
    table = None
    for _ in range(3):
        table = measure()
        if table <= PIN[dtype]:
            break
    ode = min(T.run("T", ticks, ode_ticks, 40, 600, stream)["us_per_tick"] for _ in range(3))
    del ticks, ode_ticks, slabs
    print("\n[perf guard] tick of 256 inpainting x [1,4,64,64] %s: one table blend launch %.2f us (pin %.2f), the ODE table tick "
          "of the same rows %.2f us" % (dtype, table, PIN[dtype], ode))
    assert table <= PIN[dtype], "table blend tick: %.2f us > the pinned %.2f us" % (table, PIN[dtype])

"""Performance guard of adaptive-projected-guidance stages in the table-driven launch (DPM_TABLE_APG, stage_apg_kernel_table),
pinned at what was measured.

256 DPM-Solver++(2M) requests `[1,4,64,64]` under classifier-free guidance 7.5 with cfg_apg(fn, 0, 15, -0.5) -- and the same
without a momentum -- at 256 positions of their 20-step plans, rows of slabs, the running averages in an fp32 slab, eight sets
of slabs in rotation so that every tick's inputs come from HBM (tools/pool_table_apg.py).  One tick = ONE
stage_apg_kernel_table launch (DPM_TABLE_LAUNCH | DPM_TABLE_APG on a device table filled and copied beforehand), HIP events
around 600 back-to-back ticks.  The pin is the worst value of the measuring session's runs + 8 %, the rule and the margin of the
project's other guards (profiles/r06_perf_guard.md: box-to-box spread); the measured values and the pin stand next to each
other in profiles/r26_slab_apg.md.  Best of three regions, up to three attempts (a shared box can be slower than any
regression); the figures -- and one lockstep launch of the same bytes, for the record -- are printed (`pytest -s`).  Sorts
last, like test_zz_perf_guard.py.
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

# us per tick: worst of the session's runs x 1.08 (profiles/r26_slab_apg.md)
PIN = {("fp16", -0.5): 27.98, ("fp16", 0.0): 24.55,      # 25.91 x 1.08, 22.73 x 1.08
       ("fp32", -0.5): 41.57, ("fp32", 0.0): 35.57}      # 38.49 x 1.08, 32.94 x 1.08


@pytest.mark.parametrize("momentum", [-0.5, 0.0], ids=["momentum", "no-momentum"])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_table_apg_tick_of_256_single_image_requests_stays_at_its_measured_cost(dtype, momentum):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_table_apg as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.ApgSlabs(dev, dtype, 256, 8, momentum)
    ticks, lone = slabs.ticks(), slabs.lone()
    T.prefill(ticks, stream)
    pin = PIN[dtype, momentum]

    def measure():
        return min(T.run("H", ticks, lone, 40, 600, stream)["us_per_tick"] for _ in range(3))
    table = None
    for _ in range(3):
        table = measure()
        if table <= pin:
            break
    lock = min(T.run("b", ticks, lone, 40, 600, stream)["us_per_tick"] for _ in range(3))
    del ticks, lone, slabs
    print("\n[perf guard] tick of 256 APG x [1,4,64,64] %s, momentum %g: one table APG launch %.2f us (pin %.2f), one lockstep "
          "launch of [256,4,64,64] %.2f us" % (dtype, momentum, table, pin, lock))
    assert table <= pin, "table APG tick: %.2f us > the pinned %.2f us" % (table, pin)

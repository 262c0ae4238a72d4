"""Performance guard of SDE stages in the table-driven launch (DPM_TABLE_NOISE, stage_kernel_table_noise), pinned at what was
measured.

256 SDE-DPM-Solver++ (2M) requests `[1,4,64,64]` at 256 positions of their 20-step plans, each with its own seed, rows of slabs,
eight sets of slabs in rotation so that every tick's inputs come from HBM (tools/pool_table_sde.py).  One tick = ONE
stage_kernel_table_noise launch (DPM_TABLE_LAUNCH | DPM_TABLE_NOISE on a device table filled and copied beforehand), HIP events
around 600 back-to-back ticks.  The pin is the worst value of the measuring session's runs + 8 %, the rule and the margin of
the project's other guards (profiles/r06_perf_guard.md: box-to-box spread); the measured values and the pin stand next to each
other in profiles/r17_slab_sde.md.  Best of three regions, up to three attempts (a shared box can be slower than any
regression); the figures -- and the same arrays as 16 stage_kernel_het_noise launches, for the record -- are printed
(`pytest -s`).  Sorts last, like test_zz_perf_guard.py.
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

# us per tick: worst of the session's runs x 1.08 (profiles/r17_slab_sde.md)
PIN = {"fp16": 13.07, "fp32": 17.78}      # 12.10 x 1.08, 16.46 x 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_table_noise_tick_of_256_single_image_sde_requests_stays_at_its_measured_cost(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_table_sde as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.SdeSlabs(dev, dtype, 256, 8)
    ticks = slabs.ticks()
    T.prefill(ticks, T.NOISE, stream)

    def measure():
        return min(T.run("N", ticks, None, 40, 600, stream)["us_per_tick"] for _ in range(3))
    table = None
    for _ in range(3):
        table = measure()
        if table <= PIN[dtype]:
            break
    het = min(T.run("2", ticks, None, 40, 600, stream)["us_per_tick"] for _ in range(3))
    del ticks, slabs
    print("\n[perf guard] tick of 256 SDE x [1,4,64,64] %s: one table noise launch %.2f us (pin %.2f), 16 het noise launches %.2f us"
          % (dtype, table, PIN[dtype], het))
    assert table <= PIN[dtype], "table noise tick: %.2f us > the pinned %.2f us" % (table, PIN[dtype])

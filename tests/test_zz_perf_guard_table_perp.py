"""Performance guard of Perp-Neg stages in the table-driven launch (DPM_TABLE_PERP, stage_perp_kernel_table), pinned at what was
measured.

256 DPM-Solver++(2M) requests `[1,4,64,64]` under Perp-Neg guidance (cfg_perp_neg: s = 7.5, w = 1.0) at 256 positions of their
20-step plans, rows of slabs, eight sets of slabs in rotation so that every tick's inputs come from HBM
(tools/pool_table_perp.py).  One tick = ONE stage_perp_kernel_table launch, both duplicate stores included (DPM_TABLE_LAUNCH |
DPM_TABLE_PERP on a device table filled and copied beforehand), HIP events around 600 back-to-back ticks.  The pin is the worst
value of the measuring session's runs + 8 %, the rule and the margin of the project's other guards (profiles/r06_perf_guard.md:
box-to-box spread); the measured values and the pin stand next to each other in profiles/r33_slab_perp_neg.md.  Best of three
regions, up to three attempts (a shared box can be slower than any regression); the figures -- and one lockstep launch of the
same inputs with the `torch.cat([x] * 3)` it needs, for the record -- are printed (`pytest -s`).  Sorts last, like
test_zz_perf_guard.py.
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

# us per tick: worst of the session's runs x 1.08 (profiles/r33_slab_perp_neg.md)
PIN = {"fp16": 21.16, "fp32": 38.14}      # 19.59 x 1.08, 35.31 x 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_table_perp_tick_of_256_single_image_requests_stays_at_its_measured_cost(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_table_perp as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.PerpSlabs(dev, dtype, 256, 8)
    ticks, lone = slabs.ticks(), slabs.lone()
    T.prefill(ticks, stream)

    def measure():
        return min(T.run("H", ticks, lone, 40, 600, stream)["us_per_tick"] for _ in range(3))
    table = None
    for _ in range(3):
        table = measure()
        if table <= PIN[dtype]:
            break
    lock = min(T.run("c", ticks, lone, 40, 600, stream)["us_per_tick"] for _ in range(3))
    del ticks, lone, slabs
    print("\n[perf guard] tick of 256 Perp-Neg x [1,4,64,64] %s: one table Perp-Neg launch %.2f us (pin %.2f), one lockstep "
          "launch of [256,4,64,64] plus its cat %.2f us" % (dtype, table, PIN[dtype], lock))
    assert table <= PIN[dtype], "table Perp-Neg tick: %.2f us > the pinned %.2f us" % (table, PIN[dtype])

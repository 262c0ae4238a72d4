"""Performance guard of two-condition stages in the table-driven launch (DPM_TABLE_PAIR, stage_pair_kernel_table), pinned at what
was measured.

256 DPM-Solver++(2M) requests `[1,4,64,64]` under guidance over two conditions (cfg_pair: s = 7.5, scale2 = 1.5, nested) at 256
positions of their 20-step plans, rows of slabs, eight sets of slabs in rotation so that every tick's inputs come from HBM
(tools/pool_table_pair.py).  One tick = ONE stage_pair_kernel_table launch, both duplicate stores included (DPM_TABLE_LAUNCH |
DPM_TABLE_PAIR on a device table filled and copied beforehand), HIP events around 600 back-to-back ticks.  The pin is the worst
value of the measuring session's runs + 8 %, the rule and the margin of the project's other guards (profiles/r06_perf_guard.md:
box-to-box spread); the measured values and the pin stand next to each other in profiles/r31_slab_pair.md.  Best of three
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

# us per tick: worst of the session's runs x 1.08 (profiles/r31_slab_pair.md)
PIN = {"fp16": 17.63, "fp32": 35.72}      # 16.32 x 1.08, 33.07 x 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_table_pair_tick_of_256_single_image_requests_stays_at_its_measured_cost(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import pool_table_pair as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.PairSlabs(dev, dtype, 256, 8)
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
    print("\n[perf guard] tick of 256 two-condition x [1,4,64,64] %s: one table pair launch %.2f us (pin %.2f), one lockstep "
          "launch of [256,4,64,64] plus its cat %.2f us" % (dtype, table, PIN[dtype], lock))
    assert table <= PIN[dtype], "table pair tick: %.2f us > the pinned %.2f us" % (table, PIN[dtype])

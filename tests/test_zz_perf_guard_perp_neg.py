"""Performance guard of the Perp-Neg stage kernel (DPM_F_CFG2_PERP, stage_perp_kernel), pinned at what was measured.

One lone `[256,4,64,64]` launch per stage of a 20-step DPM-Solver++(2M) plan under cfg_perp_neg (guidance scale 7.5, negative
scale 1), one workgroup per sample, eight sets of slabs in rotation so that every launch reads its inputs from HBM
(tools/perp_in_loop.py), HIP events around 600 back-to-back launches after 40.  The pin is the worst region of the measuring
session + 8 %, the rule and the margin of the project's other guards (profiles/r06_perf_guard.md: box-to-box spread); the
measured values and the pin stand next to each other in profiles/r32_cfg_perp_neg.md.  Best of three regions in ONE run, no
second attempt; the figure -- and stage_zstar_kernel's over the same slabs, the yardstick, for the record -- is printed
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

# us per stage: worst region of the session x 1.08 (profiles/r32_cfg_perp_neg.md, section 1)
PIN = {"fp16": 19.89, "fp32": 29.34}      # 18.41 x 1.08, 27.16 x 1.08


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_lone_perp_neg_launch_stays_at_its_measured_cost(dtype):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dpm_solver_amd import _lib as L
    if L.IS_LAB:
        pytest.skip("the guard times the product library")
    import perp_in_loop as T
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = T.Slabs(dev, dtype, 256, 8)
    perp = slabs.launches(T.stages("perp", slabs.td), "perp")
    zstar = slabs.launches(T.stages("zstar", slabs.td), "zstar")
    got = min(T.region(perp, 40, 600, stream) for _ in range(3))
    ref = min(T.region(zstar, 40, 600, stream) for _ in range(3))
    del perp, zstar, slabs
    print("\n[perf guard] lone [256,4,64,64] %s Perp-Neg stage: %.2f us (pin %.2f); stage_zstar_kernel on the same slabs %.2f us, "
          "ratio %.3f (bytes: 14 / 12)" % (dtype, got, PIN[dtype], ref, got / ref))
    assert got <= PIN[dtype], "Perp-Neg stage: %.2f us > the pinned %.2f us" % (got, PIN[dtype])

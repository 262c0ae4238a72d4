#!/usr/bin/env python3
"""What a CFG-Zero* stage costs next to a guidance-rescale and an adaptive-projected-guidance stage
(profiles/r27_cfg_zero_star.md).

One lone launch of `[256,4,64,64]` per stage -- 256 workgroups, one per sample -- of the three per-sample stage kernels, in
the same process, over the same slabs:
  zstar     stage_zstar_kernel,    cfg_zero_star(model_fn): rescale's bytes, two sums instead of four
  rescale   stage_rescale_kernel,  cfg_rescale(model_fn, 0.7): the yardstick
  apg       stage_apg_kernel,      cfg_apg(model_fn, 0.5, 10.0, 0.0): one read stream more than rescale (the state, in pass 1)
The stage records are those of a 20-step DPM-Solver++(2M) plan under classifier-free guidance 7.5, walked in order; eight
sets of slabs in rotation, so every launch reads its inputs from HBM.  HIP events around `--launches` back-to-back launches
after `--warmup`, `--repeat` rounds over the three kinds, alternating; us per stage = region / launches.

    python tools/zstar_in_loop.py --dtype fp16 [--out DIR/events.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dpm_solver_amd as D  # noqa: E402
from dpm_solver_amd import _lib as L  # noqa: E402

STEPS, SHAPE, SCALE = 20, (4, 64, 64), 7.5
PER = SHAPE[0] * SHAPE[1] * SHAPE[2]
DTYPES = {"fp16": (torch.float16, L.DTYPE_F16), "fp32": (torch.float32, L.DTYPE_F32)}
KINDS = {"zstar": D.cfg_zero_star, "rescale": lambda fn: D.cfg_rescale(fn, 0.7), "apg": lambda fn: D.cfg_apg(fn, 0.5, 10.0, 0.0)}
FLAGS = {"zstar": L.F_CFG_ZSTAR, "rescale": L.F_CFG_RESCALE, "apg": L.F_CFG_APG}


def stages(kind, td):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(lambda x, t, c: x, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    dpm = D.DPM_Solver(KINDS[kind](fn), ns, algorithm_type="dpmsolver++", state_dtype=td)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    out = [dpm._prep_stage(st.copy()) for st in plan.stages]
    assert all(st.flags & FLAGS[kind] for st in out)
    return out


class Slabs:
    """`sets` sets of slabs: state in [R, 4, 64, 64], state out [2R, ...] (the duplicate store's half behind the first), the two
    frozen network outputs, three cached model values"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = DTYPES[dtype]
        self.R = R
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), out=torch.empty((2 * R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()])
                     for _ in range(sets)]
        self.bytes = R * PER * torch.empty((), dtype=self.td).element_size()

    def launches(self, sts):
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st, S = sts[k % STEPS], self.sets[k % len(self.sets)]
            b = L.Buffers()
            b.x, b.e0, b.e1 = S["x"].data_ptr(), S["e0"].data_ptr(), S["e1"].data_ptr()
            b.x_out, b.x_out2 = S["out"].data_ptr(), S["out"].data_ptr() + self.bytes
            if st.h1_slot >= 0:
                b.h1 = S["h"][st.h1_slot].data_ptr()
            if st.h2_slot >= 0:
                b.h2 = S["h"][st.h2_slot].data_ptr()
            if st.flags & L.F_STORE_M:
                b.m_out = S["h"][st.m_slot].data_ptr()
            b.n, b.batch, b.state_dtype, b.eps_dtype = self.R * PER, self.R, self.code, self.code
            out.append((st, b))
        return out


def region(launches, warmup, n, stream):
    def go(k):
        st, b = launches[k % len(launches)]
        L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
    for k in range(warmup):
        go(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(warmup, warmup + n):
        go(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp16")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--launches", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zstar_in_loop.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = Slabs(dev, a.dtype, a.samples, a.sets)
    todo = {kind: slabs.launches(stages(kind, slabs.td)) for kind in KINDS}
    rows = [dict(kind=kind, us_per_stage=region(todo[kind], a.warmup, a.launches, stream))
            for _ in range(a.repeat) for kind in KINDS]
    res = {"workload": "one [%d,4,64,64] %s launch per stage, 2M + CFG %.1f, 20-step plan, frozen outputs, %d slab sets"
                       % (a.samples, a.dtype, SCALE, a.sets),
           "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "launches": a.launches, "rows": rows}
    for kind in KINDS:
        v = [r["us_per_stage"] for r in rows if r["kind"] == kind]
        res[kind] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a stage under guidance over two conditions costs (profiles/r30_cfg_pair.md).

One lone launch of `[256,4,64,64]` per stage, three ways, alternating in the same process over the same rotating slab sets:
  pair    stage_pair_kernel, cfg_pair(model_fn, c2, 1.5, nested=True): five reads (x, e0, e1, g, h1) and two writes per 2M stage
  cfg     the flag-less classifier-free stage kernel on (e0, e1), no duplicate store: four reads and two writes -- the yardstick
  torch   what a caller had without cfg_pair: the three-way blend in torch, e1 + s1 * (e0 - e1) + s2 * (g - e1) -- five
          elementwise kernels --, then the unguided stage kernel on the result
and, next to them, what the network input costs: `torch.cat([x] * 3)` per stage (`cat`).
The stage records are those of a 20-step DPM-Solver++(2M) plan, walked in order; eight sets of slabs in rotation, so every
launch reads its inputs from HBM.  HIP events around `--launches` back-to-back stages after `--warmup`, `--repeat` rounds over
the kinds, alternating; us per stage = region / launches.

    python tools/pair_in_loop.py --dtype fp16 [--out DIR/events.jsonl]
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

STEPS, SHAPE, S1, SCALE2 = 20, (4, 64, 64), 7.5, 1.5
S2 = SCALE2 - S1
PER = SHAPE[0] * SHAPE[1] * SHAPE[2]
DTYPES = {"fp16": (torch.float16, L.DTYPE_F16), "fp32": (torch.float32, L.DTYPE_F32)}
KINDS = ("pair", "cfg", "torch", "cat")


def stages(kind, td):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    if kind == "torch":
        fn = D.model_wrapper(lambda x, t: x, ns)
    else:
        fn = D.model_wrapper(lambda x, t, c: x, ns, guidance_type="classifier-free", guidance_scale=S1, condition=torch.ones(1),
                             unconditional_condition=torch.zeros(1))
        if kind == "pair":
            fn = D.cfg_pair(fn, torch.full((1,), 2.0), SCALE2, nested=True)
    dpm = D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", state_dtype=td)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    out = [dpm._prep_stage(st.copy()) for st in plan.stages]
    want = {"pair": "classifier-free-2", "cfg": "classifier-free", "torch": "uncond"}[kind]
    assert all(st.guidance == L.GUIDE[want] for st in out) and (kind != "pair" or all(st.cg_scale == S2 for st in out))
    return out


class Slabs:
    """`sets` sets of slabs: state in and out, the three frozen network outputs, the blend's result, three cached model values"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = DTYPES[dtype]
        self.R = R
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), g=mk(0.5), out=torch.empty((R,) + SHAPE, dtype=self.td, device=dev),
                          blend=torch.empty((R,) + SHAPE, dtype=self.td, device=dev), h=[mk(), mk(), mk()])
                     for _ in range(sets)]

    def launches(self, kind, sts):
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st, S = sts[k % STEPS], self.sets[k % len(self.sets)]
            b = L.Buffers()
            b.x, b.x_out = S["x"].data_ptr(), S["out"].data_ptr()
            if kind == "torch":
                b.e0 = S["blend"].data_ptr()
            else:
                b.e0, b.e1 = S["e0"].data_ptr(), S["e1"].data_ptr()
            if kind == "pair":
                b.g = S["g"].data_ptr()
            if st.h1_slot >= 0:
                b.h1 = S["h"][st.h1_slot].data_ptr()
            if st.h2_slot >= 0:
                b.h2 = S["h"][st.h2_slot].data_ptr()
            if st.flags & L.F_STORE_M:
                b.m_out = S["h"][st.m_slot].data_ptr()
            b.n, b.batch, b.state_dtype, b.eps_dtype = self.R * PER, self.R, self.code, self.code
            out.append((st, b, S))
        return out


def region(kind, launches, warmup, n, stream):
    def go(k):
        st, b, S = launches[k % len(launches)]
        if kind == "cat":
            torch.cat([S["x"]] * 3)
            return
        if kind == "torch":                    # the caller's blend inside its model callable: five elementwise kernels
            e0, e1, g = S["e0"], S["e1"], S["g"]
            torch.add(e1 + S1 * (e0 - e1), g - e1, alpha=S2, out=S["blend"])
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
        sys.exit("pair_in_loop.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = Slabs(dev, a.dtype, a.samples, a.sets)
    todo = {kind: slabs.launches(kind, stages("cfg" if kind == "cat" else kind, slabs.td)) for kind in KINDS}
    rows = [dict(kind=kind, us_per_stage=region(kind, todo[kind], a.warmup, a.launches, stream))
            for _ in range(a.repeat) for kind in KINDS]
    res = {"workload": "one [%d,4,64,64] %s launch per stage, 2M, s1 %.1f s2 %.1f, 20-step plan, frozen outputs, %d slab sets"
                       % (a.samples, a.dtype, S1, S2, a.sets),
           "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "launches": a.launches, "rows": rows}
    for kind in KINDS:
        v = [r["us_per_stage"] for r in rows if r["kind"] == kind]
        res[kind] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    res["pair_over_cfg"] = res["pair"]["median"] / res["cfg"]["median"]
    res["pair_below_torch_in_every_region"] = all(
        p["us_per_stage"] < t["us_per_stage"] for p, t in zip([r for r in rows if r["kind"] == "pair"],
                                                              [r for r in rows if r["kind"] == "torch"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

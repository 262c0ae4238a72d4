#!/usr/bin/env python3
"""What a Perp-Neg stage costs next to a CFG-Zero* stage, a two-condition stage and what a caller had before it
(profiles/r32_cfg_perp_neg.md).

One lone launch of `[256,4,64,64]` per stage -- for the per-sample kernels 256 workgroups, one per sample -- in the same
process, over the same slabs:
  perp      stage_perp_kernel,   cfg_perp_neg(model_fn, c_neg, 1.0): three read streams of network outputs; the body the
            library ships (dpm_perp_kernel.hpp: PERP_PARK)
  perp_lds  the same kernel with the third operand's difference parked in LDS between the passes      } lab build only
  perp_l2   ... with the third output read again from L2 in pass 2                                    } (DPM_TUNE_PERP_REREAD)
  zstar     stage_zstar_kernel,  cfg_zero_star(model_fn): the yardstick -- the same frame, one read stream less
  pair      stage_pair_kernel,   cfg_pair(model_fn, c2, 1.0): the same three outputs, streaming, no per-sample pass
  torch     what a caller has without the flag: the Perp-Neg reduction and blend in torch over the three outputs (fp32 sums,
            the tensors' own dtype otherwise -- the cheapest honest version), then the UNGUIDED stage kernel on the result
The stage records are those of a 20-step DPM-Solver++(2M) plan at guidance scale 7.5, walked in order; eight sets of slabs in
rotation, so every launch reads its inputs from HBM.  No kind stores a duplicate state (the two-condition records take none):
seven streams for perp and pair, six for zstar -- the byte ratio is 14 / 12 in either dtype.  HIP events around `--launches`
back-to-back launches after `--warmup`, `--repeat` rounds over the kinds, alternating; us per stage = region / launches.

    python tools/perp_in_loop.py --dtype fp16 [--out DIR/events.jsonl]
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
C2 = torch.ones(1) * 0.5
KINDS = {"perp": lambda fn: D.cfg_perp_neg(fn, C2, 1.0), "zstar": D.cfg_zero_star, "pair": lambda fn: D.cfg_pair(fn, C2, 1.0),
         "torch": lambda fn: fn}
BODIES = {"perp_lds": 0, "perp_l2": 1}           # DPM_TUNE_PERP_REREAD


def stages(kind, td):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(lambda x, t, c: x, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    dpm = D.DPM_Solver(KINDS[kind](fn), ns, algorithm_type="dpmsolver++", state_dtype=td)
    plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                         lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / ns.total_N)
    out = [dpm._prep_stage(st.copy()) for st in plan.stages]
    if kind == "torch":                          # the blend is torch's: the stage kernel sees ONE output
        for st in out:
            st.guidance = L.GUIDE["uncond"]
    assert all(bool(st.flags & L.F_CFG2_PERP) == (kind == "perp") and bool(st.flags & L.F_CFG_ZSTAR) == (kind == "zstar") for st in out)
    return out


class Slabs:
    """`sets` sets of slabs: state in and out [R, 4, 64, 64], the three frozen network outputs, the torch path's blended output,
    three cached model values"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = DTYPES[dtype]
        self.R = R
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), e2=mk(0.5), gd=mk(0.5), out=torch.empty((R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()])
                     for _ in range(sets)]

    def launches(self, sts, kind):
        out = []
        for k in range(max(STEPS, len(self.sets))):
            st, S = sts[k % STEPS], self.sets[k % len(self.sets)]
            b = L.Buffers()
            b.x, b.x_out = S["x"].data_ptr(), S["out"].data_ptr()
            if kind == "torch":
                b.e0 = S["gd"].data_ptr()
            else:
                b.e0, b.e1 = S["e0"].data_ptr(), S["e1"].data_ptr()
                if kind != "zstar":
                    b.g = S["e2"].data_ptr()
            if st.h1_slot >= 0:
                b.h1 = S["h"][st.h1_slot].data_ptr()
            if st.h2_slot >= 0:
                b.h2 = S["h"][st.h2_slot].data_ptr()
            if st.flags & L.F_STORE_M:
                b.m_out = S["h"][st.m_slot].data_ptr()
            b.n, b.batch, b.state_dtype, b.eps_dtype = self.R * PER, self.R, self.code, self.code
            out.append((st, b, S))
        return out


def perp_neg_torch(S, s=SCALE, w=1.0):
    """the reduction and the blend a caller writes today, into the slab the unguided stage kernel reads"""
    o_c, o_u, o_n = S["e0"], S["e1"], S["e2"]
    d0, d2 = o_c - o_u, o_n - o_u
    s_nd = (d2.float() * d0.float()).sum(dim=(1, 2, 3), keepdim=True)
    s_dd = (d0.float() * d0.float()).sum(dim=(1, 2, 3), keepdim=True)
    a = (s_nd / s_dd).to(d0.dtype)
    torch.add(o_u, d0 - w * (d2 - a * d0), alpha=s, out=S["gd"])


def region(launches, warmup, n, stream, before=None):
    def go(k):
        st, b, S = launches[k % len(launches)]
        if before is not None:
            before(S)
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
        sys.exit("perp_in_loop.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slabs = Slabs(dev, a.dtype, a.samples, a.sets)
    todo = {kind: slabs.launches(stages(kind, slabs.td), kind) for kind in KINDS}
    order = list(KINDS) + (list(BODIES) if L.IS_LAB else [])
    rows = []
    for _ in range(a.repeat):
        for kind in order:
            if kind in BODIES:
                L.check(L.lib.dpm_tuning_set(L.TUNE_PERP_REREAD, BODIES[kind]))
            us = region(todo["perp" if kind in BODIES else kind], a.warmup, a.launches, stream,
                        before=perp_neg_torch if kind == "torch" else None)
            if kind in BODIES:
                L.check(L.lib.dpm_tuning_set(L.TUNE_PERP_REREAD, -1))
            rows.append(dict(kind=kind, us_per_stage=us))
    res = {"workload": "one [%d,4,64,64] %s launch per stage, 2M at scale %.1f, 20-step plan, frozen outputs, %d slab sets"
                       % (a.samples, a.dtype, SCALE, a.sets),
           "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "lab": bool(L.IS_LAB),
           "launches": a.launches, "rows": rows}
    for kind in order:
        v = [r["us_per_stage"] for r in rows if r["kind"] == kind]
        res[kind] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    z = res["zstar"]
    res["perp_over_zstar"] = res["perp"]["median"] / z["median"]
    res["zstar_spread"] = (z["max"] - z["min"]) / z["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Many small CFG-Zero* requests in flight: what a stage tick of R single-image requests under classifier-free guidance with
the CFG-Zero* projection costs as ONE table CFG-Zero* launch.

tools/pool_table_rescale.py's method on DPM-Solver++(2M) plans of a solver built on `cfg_zero_star(model_fn)` at guidance scale
7.5: R (default 256) requests `[1,4,64,64]` -- 16384 elements, the largest sample the kernel's register path holds --, 20 steps,
order 2, request r at stage (k + 20 r / R) mod 20 of tick k, frozen network outputs (conditional and unconditional); the rows
live in slabs as a slab pool lays them out (the duplicate store of a stage goes to row R + r of the output slab), `--sets` (8)
sets in rotation so that every tick's inputs come from HBM.  Modes:

    H  DPM_TABLE_LAUNCH | DPM_TABLE_ZSTAR alone, on device tables filled and copied beforehand: the one stage_zstar_kernel_table
       launch
    h  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_ZSTAR: the whole stage side of a CFG-Zero* slab pool's
       tick
    a  the same call WITHOUT the flag (DPM_TABLE_LAUNCH alone, per-request stages: what version 216 runs): R stage_zstar_kernel
       launches of one workgroup each
    b  ONE lockstep stage_zstar_kernel launch of `[R,4,64,64]`: the same grid and the same bytes at one stage -- what the rows
       would cost if they marched in step.  The yardstick: code of the version before the table rows
    p  the plain ODE table tick of the same rows (classifier-free guidance alone), one stage_kernel_table launch

HIP events around `--ticks` back-to-back ticks after `--warmup` (mode a: a tenth of either, it is two orders slower),
`--repeat` rounds over the modes, alternating.  `--wall` times whole pool ticks on the host instead: a SlabPool(zero_star=True) of
R rows whose requests each bring a guidance scale and a choice of their own against a plain classifier-free SlabPool of R rows.

    python tools/pool_table_zstar.py --dtype fp16 --out DIR/events.jsonl
    python tools/pool_table_zstar.py --wall
"""
import argparse
import ctypes as C
import json
import sys

import numpy as np
import torch

import pool_table as T
import pool_table_rescale as TR
import dpm_solver_amd as D
from dpm_solver_amd import _lib as L

STEPS, SHAPE, PER = T.STEPS, T.SHAPE, T.PER
ZSTAR = L.TABLE_ZSTAR
SCALE = TR.SCALE


def solver(td, zstar=True, net=lambda x, t, c: x):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    return D.DPM_Solver(D.cfg_zero_star(fn) if zstar else fn, ns, algorithm_type="dpmsolver++", state_dtype=td)


class ZstarSlabs(TR.RescaleSlabs):
    """RescaleSlabs' sets of slabs; the stage records of the rows under `cfg_zero_star` (`stages`) and without it (`plain`)"""

    def __init__(self, dev, dtype, R, sets):
        self.td, self.code = T.DTYPES[dtype]
        self.R, self.dev = R, dev
        self.stages, self.plain = [], []
        for zstar, into in ((True, self.stages), (False, self.plain)):
            dpm = solver(self.td, zstar)
            plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                                 lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
            into += [dpm._prep_stage(st.copy()) for st in plan.stages]
        assert all(st.flags & L.F_CFG_ZSTAR for st in self.stages) and not any(st.flags & L.F_CFG_ZSTAR for st in self.plain)
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), out=torch.empty((2 * R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()]) for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()


def prefill(ticks, stream, flag=ZSTAR):
    TR.prefill(ticks, stream, flag)


def run(mode, ticks, lone, warmup, n_ticks, stream, plain=None):
    """plain: the ticks of mode p (ZstarSlabs.ticks(plain=True), prefilled with flag 0)"""
    if mode == "a":
        warmup, n_ticks = max(2, warmup // 10), max(5, n_ticks // 10)
    flag = 0 if mode in "pa" else ZSTAR

    def tick(k):
        if mode == "b":
            st, b = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            return
        sts, bufs, o, host, dev, R = (plain if mode == "p" else ticks)[k % len(ticks)]
        if mode == "h":
            o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
            T._call(L.lib, sts, bufs, R, stream)
            dev.copy_(host, non_blocking=True)
        # (mode a: the flagged rows of the device table are not read -- without the flag every request is its own launch)
        o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH | flag, dev.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        o.table_mode, bufs[0].workspace = 0, None
    for k in range(warmup):
        tick(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(warmup, warmup + n_ticks):
        tick(k)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1e3
    return dict(ticks=n_ticks, region_s=sec, us_per_tick=sec * 1e6 / n_ticks)


def wall(dev, dtype, R, ticks):
    """host wall time per tick, steady state: a SlabPool(zero_star=True) of R rows on a classifier-free solver, every request
    with a guidance scale (three in rotation) and a choice (on, on, off in rotation) of its own, against the plain
    classifier-free SlabPool of R rows under the wrapper's guidance"""
    def pool(td, **kw):
        return solver(td, False, net=lambda x, t, c: x * 0.5).request_pool(slots=R, **kw)

    def own(n):
        return dict(guidance_scale=(1.5, 3.0, SCALE)[n % 3], zero_star=(True, True, False)[n // 3 % 3])
    return T.wall(dev, dtype, R, ticks, {"slab_zstar": lambda td, g: (pool(td, zero_star=True), own),
                                         "slab_plain": lambda td, g: (pool(td), T.no_kwargs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="Hhabp")
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_zstar.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M + CFG %.1f + CFG-Zero*, 20 steps, staggered, frozen outputs, %d slab sets"
                       % (a.requests, a.dtype, SCALE, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks,
           "dtype": a.dtype}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 400))
    else:
        slabs = ZstarSlabs(dev, a.dtype, a.requests, a.sets)
        ticks, lone, plain = slabs.ticks(), slabs.lone(), slabs.ticks(plain=True)
        prefill(ticks, stream)
        prefill(plain, stream, flag=0)
        rows = []
        for _ in range(a.repeat):
            for m in a.modes:
                rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, lone, a.warmup, a.ticks, stream, plain)))
        res["rows"] = rows
        for m in sorted({r["mode"] for r in rows}):
            v = [r["us_per_tick"] for r in rows if r["mode"] == m]
            res["%s@%d" % (m, a.requests)] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

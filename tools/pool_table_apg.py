#!/usr/bin/env python3
"""Many small adaptive-projected-guidance requests in flight: what a stage tick of R single-image requests under
classifier-free guidance with APG costs as ONE table APG launch.

tools/pool_table_rescale.py's method on DPM-Solver++(2M) plans of a solver built on `cfg_apg(model_fn, 0, 15, -0.5)` at guidance
scale 7.5 (`--momentum 0`: the same without a momentum): R (default 256) requests `[1,4,64,64]` -- 16384 elements, the largest
sample the kernel's register path holds --, 20 steps, order 2, request r at stage (k + 20 r / R) mod 20 of tick k, frozen
network outputs (conditional and unconditional); the rows live in slabs as a slab pool lays them out (the duplicate store of a
stage goes to row R + r of the output slab, the running averages in one fp32 slab per set), `--sets` (8) sets in rotation so
that every tick's inputs come from HBM.  Modes:

    H  DPM_TABLE_LAUNCH | DPM_TABLE_APG alone, on device tables filled and copied beforehand: the one stage_apg_kernel_table
       launch
    h  FILL + the pinned host-to-device copy + LAUNCH, both with DPM_TABLE_APG: the whole stage side of an APG slab pool's tick
    a  the same requests WITHOUT the flag (table_mode 0, per-request stages, the average in workspace: what version 214 runs):
       R stage_apg_kernel launches of one workgroup each
    b  ONE lockstep stage_apg_kernel launch of `[R,4,64,64]`: the same grid and the same bytes at one stage -- what the rows
       would cost if they marched in step.  The yardstick: code of the version before the table rows
    r  the guidance-rescale table tick of the same rows (cfg_rescale 0.7 in place of APG), one stage_rescale_kernel_table launch
    p  the plain ODE table tick of the same rows (classifier-free guidance alone), one stage_kernel_table launch

HIP events around `--ticks` back-to-back ticks after `--warmup` (mode a: a tenth of either, it is two orders slower),
`--repeat` rounds over the modes, alternating.  `--wall` times whole pool ticks on the host instead: a SlabPool(apg=True) of R
rows whose requests each bring a guidance scale and parameters of their own against a plain classifier-free SlabPool of R rows.

    python tools/pool_table_apg.py --dtype fp16 --out DIR/events.jsonl
    python tools/pool_table_apg.py --momentum 0
    python tools/pool_table_apg.py --wall
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
APG = L.TABLE_APG
SCALE, ETA, NORM, MOMENTUM = 7.5, 0.0, 15.0, -0.5
FLAG = {"apg": APG, "rescale": L.TABLE_RESCALE, "plain": 0}


def solver(td, apg=(ETA, NORM, MOMENTUM), phi=0.0, net=lambda x, t, c: x):
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    ns = D.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - betas).astype(np.float32)))
    fn = D.model_wrapper(net, ns, guidance_type="classifier-free", guidance_scale=SCALE, condition=torch.ones(1),
                         unconditional_condition=torch.zeros(1))
    fn = D.cfg_rescale(fn, phi) if phi else (fn if apg is None else D.cfg_apg(fn, *apg))
    return D.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", state_dtype=td)


class ApgSlabs(TR.RescaleSlabs):
    """RescaleSlabs' sets of slabs plus one fp32 slab [R, 4, 64, 64] of running averages per set; the stage records of three
    kinds of the same rows: "apg" (cfg_apg(fn, 0, 15, momentum)), "rescale" (cfg_rescale 0.7) and "plain" """

    def __init__(self, dev, dtype, R, sets, momentum=MOMENTUM):
        self.td, self.code = T.DTYPES[dtype]
        self.R, self.dev, self.momentum = R, dev, momentum
        self.kinds = {}
        for kind, kw in (("apg", dict(apg=(ETA, NORM, momentum))), ("rescale", dict(apg=None, phi=TR.PHI)), ("plain", dict(apg=None))):
            dpm = solver(self.td, **kw)
            plan = dpm._get_plan(method="multistep", order=2, steps=STEPS, skip_type="time_uniform", solver_type="dpmsolver",
                                 lower_order_final=True, denoise_to_zero=False, t_T=1.0, t_0=1.0 / dpm.noise_schedule.total_N)
            self.kinds[kind] = [dpm._prep_stage(st.copy()) for st in plan.stages]
        assert all(st.flags & L.F_CFG_APG and st.thr_max == np.float32(momentum) for st in self.kinds["apg"])
        assert all(st.flags & L.F_CFG_RESCALE for st in self.kinds["rescale"])
        assert not any(st.flags & (L.F_CFG_APG | L.F_CFG_RESCALE) for st in self.kinds["plain"])
        self.stages = self.kinds["apg"]
        g = torch.Generator(device=dev).manual_seed(0)
        mk = lambda s=1.0: (s * torch.randn((R,) + SHAPE, generator=g, device=dev)).to(self.td)
        self.sets = [dict(x=mk(), e0=mk(0.5), e1=mk(0.5), out=torch.empty((2 * R,) + SHAPE, dtype=self.td, device=dev),
                          h=[mk(), mk(), mk()], avg=torch.zeros((R,) + SHAPE, dtype=torch.float32, device=dev))
                     for _ in range(sets)]
        self.rowb = PER * torch.empty((), dtype=self.td).element_size()

    def buffers(self, S, r, st, n=PER, batch=1):
        """RescaleSlabs.buffers plus the row's average with a momentum: in thr_hint, which a DPM_TABLE_APG call reads, and in
        workspace, which every other call reads (a table call's request 0: see ticks)"""
        b = super().buffers(S, r, st, n, batch)
        if (st.flags & L.F_CFG_APG) and st.thr_max != 0.0:
            b.thr_hint = b.workspace = S["avg"].data_ptr() + r * PER * 4
        return b

    def ticks(self, kind="apg"):
        """the distinct ticks of the rows under `kind`: (stages, buffers, options, host table, device table, R, request 0's own
        workspace)"""
        R, stages = self.R, self.kinds[kind]
        out = []
        for k in range(max(STEPS, len(self.sets))):
            S = self.sets[k % len(self.sets)]
            pos = [(k + (STEPS * r) // R) % STEPS for r in range(R)]
            sts = (L.Stage * R)(*[stages[p] for p in pos])
            bufs = (L.Buffers * R)(*[self.buffers(S, r, stages[pos[r]]) for r in range(R)])
            o = L.LaunchOpts()
            o.per_request_stages = 1
            bufs[0].opts = C.pointer(o)
            nb = L.table_bytes(R, FLAG[kind])
            host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
            out.append((sts, bufs, o, host, torch.empty(nb, dtype=torch.uint8, device=self.dev), R, bufs[0].workspace))
        return out


def prefill(ticks, stream, flag=APG):
    for sts, bufs, o, host, dev, R, ws0 in ticks:
        o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        assert host[:16].view(torch.int32).tolist()[2:] == [R, 1], "the tick is not one run of rows"
        dev.copy_(host)
        o.table_mode, bufs[0].workspace = 0, ws0
    torch.cuda.synchronize()


def run(mode, ticks, lone, warmup, n_ticks, stream, others=None):
    """others: {"r": the rescale ticks, "p": the plain ticks}, prefilled with their flags"""
    if mode == "a":
        warmup, n_ticks = max(2, warmup // 10), max(5, n_ticks // 10)
    flag = {"r": L.TABLE_RESCALE, "p": 0}.get(mode, APG)

    def tick(k):
        if mode == "b":
            st, b = lone[k % len(lone)]
            L.check(L.lib.dpm_stage_launch(C.byref(st), C.byref(b), stream))
            return
        src = others[mode] if mode in "rp" else ticks
        sts, bufs, o, host, dev, R, ws0 = src[k % len(src)]
        if mode == "a":
            T._call(L.lib, sts, bufs, R, stream)
            return
        if mode == "h":
            o.table_mode, bufs[0].workspace = L.TABLE_FILL | flag, host.data_ptr()
            T._call(L.lib, sts, bufs, R, stream)
            dev.copy_(host, non_blocking=True)
        o.table_mode, bufs[0].workspace = L.TABLE_LAUNCH | flag, dev.data_ptr()
        T._call(L.lib, sts, bufs, R, stream)
        o.table_mode, bufs[0].workspace = 0, ws0
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
    """host wall time per tick, steady state: a SlabPool(apg=True) of R rows on a classifier-free solver, every request with a
    guidance scale (three in rotation) and parameters (with a momentum, without, (1, 0, 0) in rotation) of its own, against the
    plain classifier-free SlabPool of R rows under the wrapper's guidance"""
    def pool(td, **kw):
        return solver(td, None, net=lambda x, t, c: x * 0.5).request_pool(slots=R, **kw)

    def own(n):
        return dict(guidance_scale=(1.5, 3.0, SCALE)[n % 3],
                    apg=((ETA, NORM, MOMENTUM), (0.5, 0.0, 0.0), (1.0, 0.0, 0.0))[n // 3 % 3])
    return T.wall(dev, dtype, R, ticks, {"slab_apg": lambda td, g: (pool(td, apg=True), own),
                                         "slab_plain": lambda td, g: (pool(td), T.no_kwargs)})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtype", choices=sorted(T.DTYPES), default="fp16")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--modes", default="Hhabrp")
    ap.add_argument("--momentum", type=float, default=MOMENTUM)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_table_apg.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "%d x [1,4,64,64] %s, 2M + CFG %.1f + APG (%g, %g, %g), 20 steps, staggered, frozen outputs, %d slab sets"
                       % (a.requests, a.dtype, SCALE, ETA, NORM, a.momentum, a.sets),
           "label": a.label, "device": torch.cuda.get_device_name(0), "version": int(L.lib.dpm_version()), "ticks": a.ticks,
           "dtype": a.dtype, "momentum": a.momentum}
    if a.wall:
        res["wall"] = wall(dev, a.dtype, a.requests, min(a.ticks, 400))
    else:
        slabs = ApgSlabs(dev, a.dtype, a.requests, a.sets, a.momentum)
        ticks, lone = slabs.ticks(), slabs.lone()
        others = {"r": slabs.ticks("rescale"), "p": slabs.ticks("plain")}
        prefill(ticks, stream)
        prefill(others["r"], stream, L.TABLE_RESCALE)
        prefill(others["p"], stream, 0)
        rows = []
        for _ in range(a.repeat):
            for m in a.modes:
                rows.append(dict(mode=m, requests=a.requests, **run(m, ticks, lone, a.warmup, a.ticks, stream, others)))
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
